"""The contact sheet's host side (`ca3d_ensemble_render_sheet`, include/ca3d.h): the layout helpers, the two symbols, and the calls
that are refused without touching a device. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ca3d_ensemble_render_sheet", "ca3d_ensemble_get_sheet_stats"]


@pytest.mark.parametrize("count", [1, 3, 290])
@pytest.mark.parametrize("columns", [1, 2, 17])
def test_sheet_shape_and_tiles(count, columns):
    w, h = 48, 32
    H, W = host.sheet_shape(count, w, h, columns)
    rows = -(-count // columns)
    assert (H, W) == (rows * h, columns * w)
    assert (rows - 1) * columns < count <= rows * columns  # no row too many, none missing
    sheet = np.zeros((H, W, 4), dtype=np.uint8)
    for k in range(count):
        t = host.sheet_tile(sheet, k, w, h, columns)
        assert t.shape == (h, w, 4) and np.shares_memory(t, sheet)  # a view
        assert not t.any()  # no tile before it has written here: tiles do not overlap
        t[...] = k % 255 + 1
    for k in (0, count // 2, count - 1):  # the tile's origin: column k % columns, row k // columns
        y, x = (k // columns) * h, (k % columns) * w
        assert (sheet[y:y + h, x:x + w] == k % 255 + 1).all()
        assert host.sheet_tile(sheet, k, w, h, columns).__array_interface__["data"][0] == sheet[y:, x:].__array_interface__["data"][0]
    assert int((sheet[..., 0] != 0).sum()) == count * w * h  # the slots past `count` stay as they were
    with pytest.raises(ValueError):
        host.sheet_tile(sheet, rows * columns, w, h, columns)
    with pytest.raises(ValueError):
        host.sheet_tile(sheet, 0, w, h, columns + 1)


def test_sheet_shape_refuses_nothing_to_draw():
    for bad in ((0, 16, 16, 1), (1, 16, 16, 0), (1, 0, 16, 1), (1, 16, 0, 1)):
        with pytest.raises(ValueError):
            host.sheet_shape(*bad)
    assert host.sheet_shape(5, 16, 32, 8) == (32, 128)  # more columns than tiles: one row


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in bound and hasattr(lib, name), name
    assert len(bound[NAMES[0]]) == 11 and bound[NAMES[1]][-1] is C.POINTER(_capi.RenderStats)
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    u = (C.c_float * 128)()
    out = np.zeros(16 * 16 * 4, dtype=np.uint8)
    assert lib.ca3d_ensemble_render_sheet(None, 0, 1, u, 16, 16, 1, 1, out.ctypes.data, None, None) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert not out.any()
    st = _capi.RenderStats()
    assert lib.ca3d_ensemble_get_sheet_stats(None, C.byref(st)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
