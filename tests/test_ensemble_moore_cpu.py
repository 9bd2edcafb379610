"""CPU-side checks of the Moore ensemble surface: ca3d_ensemble_configure_neighbourhood / ca3d_ensemble_get_neighbourhood are declared,
bound and exported, the enum is in the header, NULL handles are refused without touching a device, and the Python and JavaScript
classes take the neighbourhood."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from cellularautomatons3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ca3d_ensemble_configure_neighbourhood", "ca3d_ensemble_get_neighbourhood"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n for n, _, _ in _capi.SYMBOLS}
    lib = _capi.load()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in bound, name
        assert hasattr(lib, name), name
    assert lib.ca3d_abi_version() == 7  # additions only
    assert "#define CA3D_ABI_VERSION 7" in header


def test_enum_values_are_in_the_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    m = re.search(r"enum ca3d_ensemble_neighbourhood\s*\{(.*?)\}", header, flags=re.S)
    assert m, "enum ca3d_ensemble_neighbourhood"
    assert re.search(r"\bCA3D_ENSEMBLE_VON_NEUMANN\s*=\s*0\b", m.group(1))
    assert re.search(r"\bCA3D_ENSEMBLE_MOORE\s*=\s*1\b", m.group(1))


def test_null_handles_are_refused():
    lib = _capi.load()
    out = C.c_int(7)
    for call in (lambda: lib.ca3d_ensemble_configure_neighbourhood(None, 64, 4, 1), lambda: lib.ca3d_ensemble_get_neighbourhood(None, C.byref(out))):
        assert call() == -1
        assert b"NULL" in lib.ca3d_last_error()
    assert out.value == 7


def test_python_class_takes_the_neighbourhood():
    from cellularautomatons3d_amd import Ensemble, ensemble

    p = inspect.signature(Ensemble.configure).parameters
    assert list(p)[:4] == ["self", "n", "grid_size", "neighbourhood"]
    assert p["neighbourhood"].default == "von neumann" and p["grid_size"].default == 64
    assert isinstance(inspect.getattr_static(Ensemble, "neighbourhood"), property)
    assert inspect.getattr_static(Ensemble, "neighbourhood").fset is None  # read-only
    assert ensemble.NEIGHBOURHOODS == ("von neumann", "moore")


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_wrapper_takes_the_neighbourhood():
    r = subprocess.run([shutil.which("node"), "-e",
                        "const c=require('./cellularautomatons3d_amd/js/ca3d.js');const p=c.Ensemble.prototype;"
                        "const d=Object.getOwnPropertyDescriptor(p,'neighbourhood');"
                        "const ok=p.configure.length===3&&d&&typeof d.get==='function'&&d.set===undefined;console.log(ok?'ok':'missing')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
