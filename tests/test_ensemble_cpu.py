"""CPU-side checks of the ensemble surface (ca3d_ensemble_*): declared, bound, exported, refuses NULL handles without touching a
device, refuses to exist without a GPU, and is wrapped for JavaScript."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cellularautomatons3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ca3d_ensemble_create", "ca3d_ensemble_destroy", "ca3d_ensemble_configure", "ca3d_ensemble_set_rules", "ca3d_ensemble_upload_state",
         "ca3d_ensemble_read_state", "ca3d_ensemble_step", "ca3d_ensemble_step_until", "ca3d_ensemble_summarize", "ca3d_ensemble_synchronize",
         "ca3d_ensemble_get_stats"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n for n, _, _ in _capi.SYMBOLS}
    lib = _capi.load()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in bound, name
        assert hasattr(lib, name), name
    assert "#define CA3D_ENSEMBLE_ALL 0xFFFFFFFFu" in header and _capi.ENSEMBLE_ALL == 0xFFFFFFFF
    assert lib.ca3d_abi_version() == 7  # additions only


def test_null_handles_are_refused():
    lib = _capi.load()
    words = (C.c_uint32 * 8192)()
    lut = (C.c_uint32 * 81)()
    offs = (C.c_int32 * 18)()
    one = (C.c_uint32 * 1)()
    rec = _capi.SummaryStruct()
    st = _capi.Stats()
    calls = [
        lambda: lib.ca3d_ensemble_configure(None, 64, 4),
        lambda: lib.ca3d_ensemble_set_rules(None, 0, offs, 18, offs, 0, offs, 0, lut, lut),
        lambda: lib.ca3d_ensemble_upload_state(None, 0, 1, words, 8192),
        lambda: lib.ca3d_ensemble_read_state(None, 0, 1, words, 8192),
        lambda: lib.ca3d_ensemble_step(None, 1),
        lambda: lib.ca3d_ensemble_step_until(None, 4, 1, 3, one, one),
        lambda: lib.ca3d_ensemble_summarize(None, 0, 1, C.byref(rec)),
        lambda: lib.ca3d_ensemble_synchronize(None),
        lambda: lib.ca3d_ensemble_get_stats(None, C.byref(st)),
        lambda: lib.ca3d_ensemble_create(0, None),
    ]
    for call in calls:
        assert call() == -1
        assert b"NULL" in lib.ca3d_last_error()
    assert lib.ca3d_ensemble_destroy(None) == 0  # as ca3d_destroy: nothing to release


def test_no_ensemble_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.ca3d_ensemble_create(0, C.byref(h)) == -3 and not h.value
    assert b"no CPU fallback" in lib.ca3d_last_error()
    with pytest.raises(_capi.Ca3dError) as e:
        from cellularautomatons3d_amd import Ensemble

        Ensemble(0)
    assert e.value.code == -3


def test_python_class_surface():
    from cellularautomatons3d_amd import Ensemble, ensemble

    for m in ("configure", "set_rules", "set_rule_strings", "upload_state", "read_state", "step", "step_until", "summaries", "stats", "synchronize"):
        assert callable(getattr(Ensemble, m)), m
    assert ensemble.ALL == _capi.ENSEMBLE_ALL and _capi.ENSEMBLE_WORDS == 8192


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_wrapper_exposes_the_ensemble():
    r = subprocess.run([shutil.which("node"), "-e",
                        "const c=require('./cellularautomatons3d_amd/js/ca3d.js');"
                        "const ok=['configure','setRules','uploadState','readState','step','stepUntil','summaries'].every(m=>typeof c.Ensemble.prototype[m]==='function')"
                        "&&c.ENSEMBLE_ALL===0xFFFFFFFF&&c.ENSEMBLE_WORDS===8192;console.log(ok?'ok':'missing')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
