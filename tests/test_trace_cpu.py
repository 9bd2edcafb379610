"""CPU-side checks of the ensemble trace surface (ca3d_ensemble_step_until_trace, Ensemble.step_trace / stepTrace, host.trace_samples):
declared, bound, exported, a NULL handle refused without touching a device or the outputs, and wrapped for Python and JavaScript."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ca3d_ensemble_step_until_trace"


def test_the_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int " + NAME + r"\(", header, flags=re.M)
    assert NAME in bound and hasattr(lib, NAME)
    assert len(bound[NAME]) == len(bound["ca3d_ensemble_step_until"]) + 3  # + samples, samples_per_universe, n_samples
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only


def test_a_null_handle_is_refused_with_the_outputs_untouched():
    lib = _capi.load()
    done, reason, count = (C.c_uint32 * 2)(77, 77), (C.c_uint32 * 2)(78, 78), (C.c_uint32 * 2)(79, 79)
    samples = (C.c_uint32 * 30)(*([80] * 30))
    assert lib.ca3d_ensemble_step_until_trace(None, 4, 1, 3, done, reason, samples, 5, count) == -1
    assert b"NULL" in lib.ca3d_last_error()
    assert list(done) == [77, 77] and list(reason) == [78, 78] and list(count) == [79, 79] and list(samples) == [80] * 30


def test_python_surface():
    from cellularautomatons3d_amd import Ensemble

    p = inspect.signature(Ensemble.step_trace).parameters
    assert list(p) == ["self", "max_steps", "check_every", "stop_mask"]
    assert (p["check_every"].default, p["stop_mask"].default) == (8, 0)


@pytest.mark.parametrize("max_steps,every,k", [(0, 8, 1), (192, 4, 49), (192, 5, 40), (7, 8, 2)])
def test_trace_samples(max_steps, every, k):
    assert host.trace_samples(max_steps, every) == k


def test_trace_samples_refuses_check_every_zero():
    with pytest.raises(ValueError):
        host.trace_samples(8, 0)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_wrapper_exposes_the_trace():
    r = subprocess.run([shutil.which("node"), "-e",
                        "const c=require('./cellularautomatons3d_amd/js/ca3d.js');"
                        "const ok=typeof c.Ensemble.prototype.stepTrace==='function'&&c.traceSamples(0,8)===1&&c.traceSamples(192,4)===49"
                        "&&c.traceSamples(192,5)===40&&c.traceSamples(7,8)===2;console.log(ok?'ok':'missing')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert NAME + "(" in napi and '"ensembleStepUntilTrace"' in napi
