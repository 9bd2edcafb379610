"""Windows on the CPU: `host.cut_window` / `host.stamp_windows` / `host.window_tiling`, the numpy restatement of ca3d_cut_windows and
ca3d_stamp_windows (include/ca3d.h), against the definition spelt out cell by cell; and the binding — symbols, struct size, prototypes."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (64, 96, 128)


def cells_of(G, words):
    """[z, y, x] cells of a packed G^3 state."""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)


def words_of(cells):
    return np.packbits(np.ascontiguousarray(cells, dtype=np.uint8).ravel(), bitorder="little").view("<u4").copy()


def origins(G):
    """Every x of the issue with wrapping y and z, and the plain corners."""
    xs = (0, 1, 31, 32, 33, G - 1, G - 32, G - 63)
    yz = (0, 1, G - 1, G - 63)
    return sorted({(x, yz[(i + 2) % 4], yz[(i + 3) % 4]) for i, x in enumerate(xs)} | {(x, G - 1, G - 63) for x in xs}
                  | {(0, y, z) for y in yz for z in yz})


@pytest.mark.parametrize("G", GRIDS)
def test_cut_is_a_roll_and_a_slice(G):
    words = host.random_fill(host.words_per_buffer(G), seed=G)
    cells = cells_of(G, words)
    for (x, y, z) in origins(G):
        want = np.roll(cells, (-z, -y, -x), axis=(0, 1, 2))[:64, :64, :64]
        np.testing.assert_array_equal(host.cut_window(G, words, (x, y, z)), words_of(want), err_msg=str((x, y, z)))


def stamp_by_cells(G, words, windows, mode):
    """The definition, one cell at a time."""
    cells = cells_of(G, words).copy()
    if mode == "replace":
        for _, (ox, oy, oz) in windows:
            for k, j, i in itertools.product(range(64), repeat=3):
                cells[(oz + k) % G, (oy + j) % G, (ox + i) % G] = 0
    for u, (ox, oy, oz) in windows:
        for k, j, i in zip(*np.nonzero(cells_of(64, u))):
            cells[(oz + k) % G, (oy + j) % G, (ox + i) % G] = 0 if mode == "erase" else 1
    return words_of(cells)


def overlapping(G, n=3):
    """`n` sparse universes at origins that overlap each other and wrap on every axis."""
    us = [host.random_fill(8192, seed=40 + k, and_rounds=4) for k in range(n)]
    at = [(G - 33, G - 1, 5), (G - 1, 10, G - 63), (17, G - 20, G - 30)][:n]
    return list(zip(us, at))


@pytest.mark.parametrize("mode", host.STAMP_MODES)
@pytest.mark.parametrize("G", (64, 96))
def test_stamp_is_the_cell_loop(G, mode):
    words = host.random_fill(host.words_per_buffer(G), seed=7, and_rounds=1)
    wins = overlapping(G)
    got = host.stamp_windows(G, words, wins, mode)
    np.testing.assert_array_equal(got, stamp_by_cells(G, words, wins, mode))
    assert not np.array_equal(got, words)


@pytest.mark.parametrize("mode", host.STAMP_MODES)
def test_stamp_does_not_depend_on_the_order(mode):
    G = 96
    words = host.random_fill(host.words_per_buffer(G), seed=9, and_rounds=1)
    wins = overlapping(G)
    first = host.stamp_windows(G, words, wins, mode)
    for perm in itertools.permutations(wins):
        np.testing.assert_array_equal(host.stamp_windows(G, words, list(perm), mode), first)


@pytest.mark.parametrize("G", GRIDS)
def test_cut_after_replace_returns_the_universe(G):
    words = host.random_fill(host.words_per_buffer(G), seed=3)
    u = host.random_fill(8192, seed=11, and_rounds=1)
    for at in ((G - 1, G - 63, 33), (0, 0, 0), (31, G - 1, G - 32)):
        after = host.stamp_windows(G, words, [(u, at)], "replace")
        np.testing.assert_array_equal(host.cut_window(G, after, at), u)
        # and nothing outside the box moved
        outside = np.roll(cells_of(G, after) != cells_of(G, words), tuple(-v for v in at[::-1]), axis=(0, 1, 2))
        outside[:64, :64, :64] = False
        assert not outside.any()


@pytest.mark.parametrize("G", (64, 128, 192))
def test_tiling_covers_every_cell_once(G):
    seen = np.zeros((G, G, G), dtype=np.uint8)
    at = host.window_tiling(G)
    assert at.shape == ((G // 64) ** 3, 3)
    i = np.arange(64)
    for x, y, z in at:
        seen[np.ix_((z + i) % G, (y + i) % G, (x + i) % G)] += 1
    assert (seen == 1).all()


def test_tiling_of_a_grid_64_does_not_divide():
    at = host.window_tiling(96)
    assert at.shape == (8, 3) and at.max() == 64 and [tuple(v) for v in at[:3]] == [(0, 0, 0), (64, 0, 0), (0, 64, 0)]
    with pytest.raises(ValueError):
        host.window_tiling(32)


def test_refusals_of_the_host_functions():
    words = np.zeros(host.words_per_buffer(64), dtype=np.uint32)
    with pytest.raises(ValueError):
        host.cut_window(64, words, (64, 0, 0))
    with pytest.raises(ValueError):
        host.stamp_windows(64, words, [], "xor")
    rec = host.window_records([(3, (1, 2, 3))])
    assert rec.dtype == host.WINDOW_DTYPE and rec.tobytes() == np.array([3, 1, 2, 3], dtype="<u4").tobytes()


def test_symbols_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = {
        "ca3d_cut_windows": r"int ca3d_cut_windows\(ca3d_t \*src, ca3d_ensemble_t \*dst, uint32_t n, const ca3d_window \*w, float \*gpu_ms\s*\);",
        "ca3d_stamp_windows": r"int ca3d_stamp_windows\(ca3d_t \*dst, ca3d_ensemble_t \*src, uint32_t n, const ca3d_window \*w, uint32_t mode, float \*gpu_ms\s*\);",
    }
    for name, proto in protos.items():
        assert re.search(proto, flat), name
        assert name in bound and hasattr(lib, name)
    H, u32, f32p = C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
    assert bound["ca3d_cut_windows"] == [H, H, u32, C.POINTER(_capi.WindowStruct), f32p]
    assert bound["ca3d_stamp_windows"] == [H, H, u32, C.POINTER(_capi.WindowStruct), u32, f32p]
    assert C.sizeof(_capi.WindowStruct) == 16 == host.WINDOW_DTYPE.itemsize
    assert [(n, host.WINDOW_DTYPE.fields[n][1]) for n in host.WINDOW_DTYPE.names] == [("universe", 0), ("origin", 4)]
    assert (_capi.WindowStruct.universe.offset, _capi.WindowStruct.origin.offset) == (0, 4)
    assert re.search(r"uint32_t universe;.*?uint32_t origin\[3\];.*?\} ca3d_window;", header, flags=re.S)
    for name, value in _capi.STAMP_MODES.items():
        assert re.search(r"CA3D_STAMP_%s = %d\b" % (name.upper(), value), header)
    assert tuple(_capi.STAMP_MODES) == host.STAMP_MODES
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    w = (_capi.WindowStruct * 2)()
    assert lib.ca3d_cut_windows(None, None, 2, w, None) == -1 and "NULL" in lib.ca3d_last_error().decode()
    assert lib.ca3d_stamp_windows(None, None, 2, w, 0, None) == -1 and "NULL" in lib.ca3d_last_error().decode()
    assert lib.ca3d_stamp_windows(None, None, 2, w, 3, None) == -1 and "mode" in lib.ca3d_last_error().decode()
