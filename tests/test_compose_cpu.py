"""The compose's host side (`ca3d_ensemble_compose`, include/ca3d.h): the 48 orientations (`host.orientation_matrix`,
`orientation_from_matrix`, `orient_vector`) and `host.compose`, the numpy restatement of the definition, against an independent
formulation — `np.transpose` and `np.flip` of the cropped box — and hand-built cases; the symbol, the structs, the Python and JS
surfaces and the refusal that needs no device. No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import census_cases as cc
from cellularautomatons3d_amd import _capi, host
from cellularautomatons3d_amd.ensemble import Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, W = 64, 8192


def cells_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def words_of(cells):
    return np.packbits(np.asarray(cells, dtype=np.uint8).ravel(), bitorder="little").view("<u4").astype(np.uint32)


def turned_by_numpy(words, o, at):
    """The independent formulation: the piece's box as an array indexed [x, y, z], its axes permuted by np.transpose and mirrored by
    np.flip, pasted at `at` with what leaves the cube cut off -> (cells [z, y, x], placed, clipped)."""
    c = cells_of(words).transpose(2, 1, 0)  # [x, y, z]
    idx = np.nonzero(c)
    box = c[tuple(slice(int(i.min()), int(i.max()) + 1) for i in idx)]
    t = np.transpose(box, host.ORIENTATION_PERMS[o % 6])
    t = np.flip(t, axis=[i for i in range(3) if (o // 6) >> i & 1])
    big = np.zeros((3 * G,) * 3, dtype=np.uint8)  # the cube is [G, 2 G) of it on every axis: at = -64 .. 64 and an extent of 64 fit
    big[tuple(slice(G + a, G + a + n) for a, n in zip(at, t.shape))] = t
    inside = big[G:2 * G, G:2 * G, G:2 * G]
    return inside.transpose(2, 1, 0), int(inside.sum()), int(big.sum() - inside.sum())


def test_symbol_structs_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_compose\(", header, flags=re.M)
    assert "ca3d_ensemble_compose" in bound and hasattr(lib, "ca3d_ensemble_compose")
    assert len(bound["ca3d_ensemble_compose"]) == 9
    assert C.sizeof(_capi.ComposePartStruct) == 24 == host.COMPOSE_PART_DTYPE.itemsize
    assert C.sizeof(_capi.ComposedStruct) == 16 == host.COMPOSED_DTYPE.itemsize
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    assert re.search(r"^#define CA3D_COMPOSE_OVER 0x1u\b", header, flags=re.M) and _capi.COMPOSE_OVER == 0x1
    assert re.search(r"^#define CA3D_COMPOSE_COPY_RULES 0x100u\b", header, flags=re.M) and _capi.COMPOSE_COPY_RULES == 0x100
    assert re.search(r"^#define CA3D_COMPOSE_MAX_PARTS \(1u << 20\)$", header, flags=re.M) and _capi.COMPOSE_MAX_PARTS == 1 << 20
    src = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "ca3d_ensemble.cpp")).read()
    assert re.search(r"^int ca3d_ensemble_compose\([^;{]*?\) CA3D_API_TRY\n\{\n", src, flags=re.S | re.M)


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.ComposedStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    parts = (_capi.ComposePartStruct * 2)()
    begin = (C.c_uint32 * 3)(0, 1, 2)
    ms = C.c_float(-1.0)
    assert lib.ca3d_ensemble_compose(None, 0, 2, None, parts, begin, 0, out, C.byref(ms)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and ms.value == -1.0


def test_python_and_js_surfaces():
    assert callable(Ensemble.compose) and callable(Ensemble.compose_gpu_ms)
    for name in ("ORIENTATION_PERMS", "orientation_matrix", "orientation_from_matrix", "orient_vector", "compose"):
        assert hasattr(host, name), name
    assert host.ORIENTATION_PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    assert re.search(r"^\tcompose\(layouts, opts\)$", js, flags=re.M) and "ensembleCompose(" in js
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert '{"ensembleCompose", js_ensemble_compose}' in napi and "ca3d_ensemble_compose(" in napi
    parts = host.compose_parts([(3, 47, (-64, 0, 64))])
    assert parts.tobytes() == np.array([3, 47, -64, 0, 64, 0], dtype="<i4").tobytes()


def test_the_48_orientations_are_the_symmetries_of_the_cube():
    ms = [host.orientation_matrix(o) for o in range(48)]
    for m in ms:
        assert m.shape == (3, 3) and np.issubdtype(m.dtype, np.integer)
        assert np.array_equal(m @ m.T, np.eye(3, dtype=int))  # orthogonal: a signed permutation
    keys = {m.tobytes() for m in ms}
    assert len(keys) == 48
    assert all((a @ b).tobytes() in keys for a in ms for b in ms)  # closed under product
    dets = [int(round(np.linalg.det(m))) for m in ms]
    assert dets.count(1) == 24 and dets.count(-1) == 24
    assert np.array_equal(ms[0], np.eye(3, dtype=int))
    for o, m in enumerate(ms):
        assert host.orientation_from_matrix(m) == o
        assert host.orientation_from_matrix(m.tolist()) == o
        inv = host.orientation_from_matrix(m.T)
        assert np.array_equal(host.orientation_matrix(inv) @ m, np.eye(3, dtype=int))
        v = (1, 2, 3)
        assert host.orient_vector(o, v) == tuple(int(c) for c in m @ np.array(v))
        perm, f = host.ORIENTATION_PERMS[o % 6], o // 6
        assert host.orient_vector(o, v) == tuple((-1 if f >> i & 1 else 1) * v[perm[i]] for i in range(3))
    assert host.orient_vector(0, (1, 1, 0)) == (1, 1, 0) and host.orient_vector(6, (1, 1, 0)) == (-1, 1, 0)
    for bad in (np.zeros((3, 3), dtype=int), np.ones((3, 3), dtype=int), 2 * np.eye(3, dtype=int), np.eye(2, dtype=int)):
        with pytest.raises(ValueError):
            host.orientation_from_matrix(bad)
    for bad in (-1, 48, 1.5):
        with pytest.raises(ValueError):
            host.orientation_matrix(bad)


def test_compose_is_transpose_and_flip_for_all_48():
    """SHAPE at (27, 40, 2), across the word seam, put at three places: the definition and transpose + flip agree for all 48, and the
    48 turned shapes are pairwise distinct, so a wrong orientation cannot hide."""
    state = cc.state("shape_1")
    seen = set()
    for o in range(48):
        for at in ((5, 6, 7), (30, 0, 59), (-2, 61, 33)):
            words, rec = host.compose([state], [(0, o, at)])
            want, placed, clipped = turned_by_numpy(state, o, at)
            np.testing.assert_array_equal(cells_of(words), want, err_msg=f"orientation {o} at {at}")
            assert (int(rec["population"]), int(rec["placed"]), int(rec["overlap"]), int(rec["clipped"])) == (placed, placed, 0, clipped)
            assert placed + clipped == len(cc.SHAPE)
            assert words.dtype == np.uint32 and words.shape == (W,)
        seen.add(host.compose([state], [(0, o, (5, 6, 7))])[0].tobytes())
    assert len(seen) == 48
    # a denser piece with no symmetry: a soup's corner
    soup = np.zeros((G, G, G), dtype=np.uint8)
    soup[3:12, 50:57, 29:40] = cells_of(host.random_fill(W, seed=3, and_rounds=1))[3:12, 50:57, 29:40]
    for o in range(48):
        words, rec = host.compose({7: words_of(soup)}, [(7, o, (-3, 58, 20))])
        want, placed, clipped = turned_by_numpy(words_of(soup), o, (-3, 58, 20))
        np.testing.assert_array_equal(cells_of(words), want, err_msg=f"orientation {o}")
        assert (int(rec["placed"]), int(rec["clipped"])) == (placed, clipped)


def test_orientation_0_at_box_min_is_the_identity():
    for name in ("shapes", "shell_core", "corners", "staircase", "serpentine", "full", "pairs1_+-+"):
        state = cc.state(name)
        zs, ys, xs = np.nonzero(cells_of(state))
        words, rec = host.compose([state], [(0, 0, (int(xs.min()), int(ys.min()), int(zs.min())))])
        np.testing.assert_array_equal(words, state, err_msg=name)
        assert (int(rec["population"]), int(rec["placed"]), int(rec["overlap"]), int(rec["clipped"])) == (zs.size, zs.size, 0, 0)
    words, rec = host.compose([cc.state("empty")], [(0, 17, (3, 3, 3))])
    assert not words.any() and rec.tobytes() == bytes(16)
    words, rec = host.compose([], [])
    assert not words.any() and rec.tobytes() == bytes(16) and words.shape == (W,)


def test_clipping_and_overlap_by_hand():
    bar = cc.words([(x, 0, 0) for x in range(10)])  # ten cells along x
    cell = cc.words([(40, 40, 40)])
    # pushed through the +x face: 4 of 10 stay
    words, rec = host.compose([bar], [(0, 0, (60, 5, 5))])
    assert rec.tolist() == (4, 4, 0, 6) and cells_of(words)[5, 5, 60:].all() and int(cells_of(words).sum()) == 4
    # through the -x face: the bar's high end stays; mirrored, its low end would — the same cells either way
    words, rec = host.compose([bar], [(0, 6, (-7, 5, 5))])
    assert rec.tolist() == (3, 3, 0, 7) and cells_of(words)[5, 5, :3].all()
    # turned onto z (orientation 5: perm (2, 1, 0)), through the +z face
    words, rec = host.compose([bar], [(0, 5, (9, 9, 58))])
    assert rec.tolist() == (6, 6, 0, 4) and cells_of(words)[58:, 9, 9].all()
    # wholly outside
    for at in ((64, 0, 0), (0, -64, 0), (-10, 0, 0), (0, 0, 64)):
        words, rec = host.compose([bar], [(0, 0, at)])
        assert rec.tolist() == (0, 0, 0, 10) and not words.any()
    # two bars crossing in one cell, on a base that holds that cell and one other
    base = cc.words([(14, 20, 20), (0, 0, 0)])
    words, rec = host.compose([bar, cell], [(0, 0, (10, 20, 20)), (0, 2, (14, 16, 20)), (1, 0, (63, 63, 63))], base=base)
    # perm (1, 0, 2): the bar runs along y, x = 14, y = 16 .. 25
    assert rec.tolist() == (21, 21, 2, 0)  # 2 + 10 + 10 + 1 cells, (14, 20, 20) three times
    c = cells_of(words)
    assert c[20, 20, 10:20].all() and c[20, 16:26, 14].all() and c[63, 63, 63] and c[0, 0, 0]
    # the same parts in another order, and without the base
    again, rec2 = host.compose([bar, cell], [(1, 0, (63, 63, 63)), (0, 2, (14, 16, 20)), (0, 0, (10, 20, 20))], base=base)
    np.testing.assert_array_equal(again, words)
    assert rec2.tobytes() == rec.tobytes()
    words, rec = host.compose([bar, cell], [(0, 0, (10, 20, 20)), (0, 2, (14, 16, 20))])
    assert rec.tolist() == (19, 20, 1, 0)
    for bad in ([(0, 48, (0, 0, 0))], [(0, -1, (0, 0, 0))], [(0, 0, (65, 0, 0))], [(0, 0, (0, -65, 0))], [(0, 0, (0, 0))]):
        with pytest.raises(ValueError):
            host.compose([bar], bad)
    with pytest.raises(ValueError):
        host.compose([bar[:100]], [(0, 0, (0, 0, 0))])


def test_the_glider_turns_with_its_orientation():
    """The doubled glider of tests/test_gpu_moving.py, composed in all 48 orientations near the centre: after four oracle steps it has
    moved by orient_vector(o, (1, 1, 0)). The 48 give 24 distinct states: the glider has one mirror symmetry."""
    from test_gpu_census import np_step
    from test_gpu_moving import glider

    ship = glider("xy", (28, 30, 30))
    starts = set()
    for o in range(48):
        first, rec = host.compose([ship], [(0, o, (30, 30, 30))])
        assert rec.tolist() == (10, 10, 0, 0)
        starts.add(first.tobytes())
        c = cells_of(first)
        for _ in range(4):
            c = np_step(c)
        assert host.moved_by(G, first, words_of(c)) == host.orient_vector(o, (1, 1, 0)), o
    assert len(starts) == 24
