"""CPU-side checks of the cycle-detection surface (CA3D_STOP_PERIODIC, ca3d_step_until_cycle, ca3d_ensemble_step_until_cycle): declared,
bound, exported, NULL handles refused without touching a device or the outputs, and wrapped for Python and JavaScript."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from cellularautomatons3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ca3d_step_until_cycle", "ca3d_ensemble_step_until_cycle"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in bound, name
        assert hasattr(lib, name), name
    assert len(bound["ca3d_step_until_cycle"]) == len(bound["ca3d_step_until"]) + 1  # + period
    assert len(bound["ca3d_ensemble_step_until_cycle"]) == len(bound["ca3d_ensemble_step_until"]) + 1
    assert re.search(r"\bCA3D_STOP_PERIODIC = 4\b", header)
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # additions only
    assert _capi.STOP_PERIODIC == 4


def test_null_handles_are_refused_with_the_outputs_untouched():
    lib = _capi.load()
    rec = _capi.SummaryStruct()
    done, reason, period = (C.c_uint32 * 2)(77, 77), (C.c_uint32 * 2)(78, 78), (C.c_uint32 * 2)(79, 79)
    for call in (lambda: lib.ca3d_ensemble_step_until_cycle(None, 4, 1, 7, done, reason, period),
                 lambda: lib.ca3d_step_until_cycle(None, 4, 1, 7, C.byref(rec), done, reason, period)):
        assert call() == -1
        assert b"NULL" in lib.ca3d_last_error()
        assert list(done) == [77, 77] and list(reason) == [78, 78] and list(period) == [79, 79]


def test_python_surface():
    from cellularautomatons3d_amd import Engine, Ensemble, engine

    assert engine.STOP_PERIODIC == 4 and (engine.STOP_EXTINCT, engine.STOP_STILL) == (1, 2)
    p = inspect.signature(Engine.step_until_cycle).parameters
    assert list(p) == ["self", "max_steps", "check_every", "extinct", "still", "periodic"]
    assert (p["check_every"].default, p["extinct"].default, p["still"].default, p["periodic"].default) == (8, True, True, True)
    p = inspect.signature(Ensemble.step_until_cycle).parameters
    assert list(p) == ["self", "max_steps", "check_every", "stop_mask"]
    assert (p["check_every"].default, p["stop_mask"].default) == (8, 7)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_wrapper_exposes_cycle_detection():
    r = subprocess.run([shutil.which("node"), "-e",
                        "const c=require('./cellularautomatons3d_amd/js/ca3d.js');"
                        "const ok=typeof c.Engine.prototype.stepUntilCycle==='function'&&typeof c.Ensemble.prototype.stepUntilCycle==='function'"
                        "&&c.STOP_PERIODIC===4&&c.STOP_EXTINCT===1&&c.STOP_STILL===2;console.log(ok?'ok':'missing')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    for name in NAMES:
        assert name + "(" in napi, name
