"""CPU-side checks of the clustered ensemble surface: ca3d_ensemble_configure_clustered / ca3d_ensemble_get_clustered /
ca3d_ensemble_set_rule_tables_clustered are declared, bound and exported, NULL handles are refused without touching a device, and the
Python and JavaScript classes take `clustered` beside the neighbourhood."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from cellularautomatons3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ca3d_ensemble_configure_clustered", "ca3d_ensemble_get_clustered", "ca3d_ensemble_set_rule_tables_clustered"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n for n, _, _ in _capi.SYMBOLS}
    lib = _capi.load()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in bound, name
        assert hasattr(lib, name), name
    assert lib.ca3d_abi_version() == 7  # additions only
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M)


def test_null_handles_are_refused():
    lib = _capi.load()
    out = C.c_int(7)
    masks = (C.c_uint32 * 3)(1, 1, 1)
    for call in (lambda: lib.ca3d_ensemble_configure_clustered(None, 64, 4), lambda: lib.ca3d_ensemble_get_clustered(None, C.byref(out)),
                 lambda: lib.ca3d_ensemble_set_rule_tables_clustered(None, 0, 1, masks, masks, 1)):
        assert call() == -1
        assert b"NULL" in lib.ca3d_last_error()
    assert out.value == 7 and list(masks) == [1, 1, 1]


def test_python_class_takes_clustered():
    from cellularautomatons3d_amd import Ensemble, ensemble

    p = inspect.signature(Ensemble.configure).parameters
    assert list(p) == ["self", "n", "grid_size", "neighbourhood", "clustered"]
    assert p["clustered"].default is False and p["neighbourhood"].default == "von neumann" and p["grid_size"].default == 64
    assert isinstance(inspect.getattr_static(Ensemble, "clustered"), property)
    assert inspect.getattr_static(Ensemble, "clustered").fset is None  # read-only
    assert list(inspect.signature(Ensemble.set_clustered_tables).parameters) == ["self", "first", "born_masks", "survive_masks", "count"]
    assert ensemble.NEIGHBOURHOODS == ("von neumann", "moore")  # clustered is a property beside the neighbourhood, not a third one


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_wrapper_takes_clustered():
    r = subprocess.run([shutil.which("node"), "-e",
                        "const c=require('./cellularautomatons3d_amd/js/ca3d.js');const p=c.Ensemble.prototype;"
                        "const d=Object.getOwnPropertyDescriptor(p,'clustered');"
                        "const ok=p.configure.length===3&&d&&typeof d.get==='function'&&d.set===undefined"
                        "&&typeof p.setClusteredTables==='function';console.log(ok?'ok':'missing')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
