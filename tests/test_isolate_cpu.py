"""The isolate's host side (`ca3d_ensemble_isolate`, include/ca3d.h): `host.isolate`, the numpy restatement of the definition, on the
crafted states of tests/census_cases.py — against `host.census`, `host.state_summary` and, where it imports, `scipy.ndimage.label`
with the full 3 x 3 x 3 structure; the symbol, the structs and the refusals that need no device. No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import census_cases as cc
from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, W = 64, 8192
PLACEMENTS = ("keep", "centre", "origin")
#: every crafted state but the two long fills, which one test runs once
QUICK = [n for n in cc.CRAFTED if n not in ("serpentine", "full")]


def cells_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def box_of(words):
    zs, ys, xs = np.nonzero(cells_of(words))
    return (int(xs.min()), int(ys.min()), int(zs.min())), (int(xs.max()), int(ys.max()), int(zs.max()))


def components(name):
    comps, n, rest = cc.reference(name, 64)
    assert rest == 0, name  # complete on the reference's side
    return comps[:n]


@pytest.mark.parametrize("name", QUICK)
def test_keep_isolates_partition_the_state(name):
    state = cc.state(name)
    union = np.zeros(W, dtype=np.uint32)
    total = 0
    for c in components(name):
        words, pop, shift = host.isolate(state, int(c["first_cell"]), "keep")
        assert words.dtype == np.uint32 and words.shape == (W,)
        assert shift == (0, 0, 0) and pop == int(c["population"]) == int(cells_of(words).sum())
        assert not (union & words).any(), name  # disjoint
        union |= words
        total += pop
    np.testing.assert_array_equal(union, state)
    assert total == int(cells_of(state).sum())


@pytest.mark.parametrize("name", QUICK)
def test_origin_is_the_census_record(name):
    state = cc.state(name)
    for c in components(name):
        words, pop, shift = host.isolate(state, int(c["first_cell"]), "origin")
        lo, hi = host.unpack_box(c["box_min"]), host.unpack_box(c["box_max"])
        assert shift == tuple(-v for v in lo)
        s = host.state_summary(G, words)
        assert s["digest"] == int(c["digest"]) and s["population"] == pop == int(c["population"])
        assert box_of(words) == ((0, 0, 0), tuple(h - l for l, h in zip(lo, hi)))
        # "keep" and "centre" leave another digest unless the shift is the same
        for other in ("keep", "centre"):
            w2, _, s2 = host.isolate(state, int(c["first_cell"]), other)
            assert (host.state_summary(G, w2)["digest"] == int(c["digest"])) == (s2 == shift)


@pytest.mark.parametrize("name", QUICK)
def test_centre_box(name):
    state = cc.state(name)
    for c in components(name):
        words, pop, shift = host.isolate(state, int(c["first_cell"]), "centre")
        lo, hi = host.unpack_box(c["box_min"]), host.unpack_box(c["box_max"])
        extent = tuple(h - l + 1 for l, h in zip(lo, hi))
        want_lo = tuple((G - e) // 2 for e in extent)
        assert shift == tuple(w - l for w, l in zip(want_lo, lo))
        assert box_of(words) == (want_lo, tuple(w + e - 1 for w, e in zip(want_lo, extent)))
        # the same cells, translated
        keep = cells_of(host.isolate(state, int(c["first_cell"]), "keep")[0])
        zs, ys, xs = np.nonzero(keep)
        moved = np.zeros_like(keep)
        moved[zs + shift[2], ys + shift[1], xs + shift[0]] = 1
        np.testing.assert_array_equal(cells_of(words), moved)


def test_any_cell_selects_its_component_and_a_dead_cell_nothing():
    for name in ("shapes", "shell_core", "staircase", "pairs1_+++", "corners"):
        state = cc.state(name)
        for c in components(name):
            want = host.isolate(state, int(c["first_cell"]), "centre")
            zs, ys, xs = np.nonzero(cells_of(host.isolate(state, int(c["first_cell"]), "keep")[0]))
            keys = zs * 4096 + ys * 64 + xs
            for cell in {int(keys.min()), int(keys.max()), int(keys[len(keys) // 2])}:
                got = host.isolate(state, cell, "centre")
                np.testing.assert_array_equal(got[0], want[0])
                assert got[1:] == want[1:]
    state = cc.state("shapes")
    for placement in PLACEMENTS:
        for cell in (0, 63 | 63 << 6 | 63 << 12, 3 | 2 << 6 | 2 << 12):  # the last: a dead cell inside the first shape's box
            assert not cells_of(state).ravel()[cell]
            words, pop, shift = host.isolate(state, cell, placement)
            assert not words.any() and pop == 0 and shift == (0, 0, 0) and words.shape == (W,)
    for bad in (-1, 1 << 18):
        with pytest.raises(ValueError):
            host.isolate(state, bad)
    with pytest.raises(ValueError):
        host.isolate(state, 0, "middle")
    with pytest.raises(ValueError):
        host.isolate(state[:100], 0)


def test_shell_without_core_and_core_without_shell():
    """Their boxes overlap — the core's lies inside the shell's: a cut by bounding box would take both."""
    state = cc.state("shell_core")
    shell_rec, core_rec = components("shell_core")
    shell, core = (cells_of(host.isolate(state, int(c["first_cell"]), "keep")[0]) for c in (shell_rec, core_rec))
    want_shell, want_core = np.zeros((G, G, G), dtype=np.uint8), np.zeros((G, G, G), dtype=np.uint8)
    cx, cy, cz = 27, 12, 2
    for i, j, k in itertools.product(range(9), repeat=3):
        if 0 in (i, j, k) or 8 in (i, j, k):
            want_shell[cz + k, cy + j, cx + i] = 1
    for i, j, k in itertools.product(range(3, 6), repeat=3):
        want_core[cz + k, cy + j, cx + i] = 1
    np.testing.assert_array_equal(shell, want_shell)
    np.testing.assert_array_equal(core, want_core)
    assert (int(shell.sum()), int(core.sum())) == (386, 27)
    (slo, shi), (clo, chi) = box_of(host.isolate(state, int(shell_rec["first_cell"]), "keep")[0]), box_of(host.isolate(state, int(core_rec["first_cell"]), "keep")[0])
    assert all(a < b for a, b in zip(slo, clo)) and all(a > b for a, b in zip(shi, chi))
    # centred, the shell is still hollow
    centred = cells_of(host.isolate(state, int(shell_rec["first_cell"]), "centre")[0])
    assert box_of(host.isolate(state, int(shell_rec["first_cell"]), "centre")[0]) == ((27, 27, 27), (35, 35, 35))
    assert not centred[28:35, 28:35, 28:35].any()


def test_full_and_serpentine():
    full = cc.state("full")
    for placement in PLACEMENTS:
        words, pop, shift = host.isolate(full, 12345, placement)
        assert shift == (0, 0, 0) and pop == G ** 3
        np.testing.assert_array_equal(words, full)
    state = cc.state("serpentine")
    words, pop, shift = host.isolate(state, 63 | 62 << 6 | 10 << 12, "origin")  # selected by its last cell
    assert pop == 32 * 64 + 31 and shift == (0, 0, -10)
    assert host.state_summary(G, words)["digest"] == int(cc.reference("serpentine", 4)[0]["digest"][0])


def test_the_issue_s_figures():
    """The glider of the census test beside its block: centred with shift (2, 0, 1) it moves by (1, 1, 0) in 4 steps; the block is a
    still life; a glider at corner (60, 60, 30) centres with shift (-30, -30, 1)."""
    from test_gpu_census import np_step
    from test_gpu_moving import glider

    block = [(10 + i, 10 + j, 40 + k) for i, j, k in itertools.product((0, 1), repeat=3)]
    state = glider("xy", (28, 30, 30)) | host.cells_to_words(G, block)
    comps, n, rest = host.census(state, 64)
    assert (n, rest) == (2, 0)
    ship, pop, shift = host.isolate(state, int(comps[0]["first_cell"]), "centre")
    assert (pop, shift) == (10, (2, 0, 1))
    c = cells_of(ship)
    for _ in range(4):
        c = np_step(c)
    after = np.packbits(c.ravel(), bitorder="little").view("<u4")
    assert host.moved_by(G, ship, after) == (1, 1, 0)
    blk, pop, shift = host.isolate(state, int(comps[1]["first_cell"]), "centre")
    assert pop == 8 and box_of(blk) == ((31, 31, 31), (32, 32, 32))
    np.testing.assert_array_equal(np_step(cells_of(blk)), cells_of(blk))
    corner = glider("xy", (60, 60, 30))
    assert host.isolate(corner, int(host.census(corner, 4)[0]["first_cell"][0]), "centre")[2] == (-30, -30, 1)
    for placement, same in (("origin", True), ("keep", False), ("centre", False)):
        for rec in comps[:2]:
            w = host.isolate(state, int(rec["first_cell"]), placement)[0]
            assert (host.state_summary(G, w)["digest"] == int(rec["digest"])) == same


@pytest.mark.parametrize("name", ["shapes", "shell_core", "corners", "staircase", "pairs1_+-+", "pairs2_0++", "giant"])
def test_against_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    state = cc.state(name)
    cells = cells_of(state)
    lab, n = ndimage.label(cells, structure=np.ones((3, 3, 3), dtype=int))
    assert n == (cc.CRAFTED[name][1] if name in cc.CRAFTED else cc.SYNTHETIC[name][1])
    for k in list(range(1, n + 1))[:: max(1, n // 12)]:
        part = (lab == k).astype(np.uint8)
        zs, ys, xs = np.nonzero(part)
        cell = int(zs[-1]) * 4096 + int(ys[-1]) * 64 + int(xs[-1])  # the component's last cell
        words, pop, shift = host.isolate(state, cell, "keep")
        np.testing.assert_array_equal(cells_of(words), part)
        assert pop == zs.size
        words, pop, shift = host.isolate(state, cell, "origin")
        moved = np.zeros_like(part)
        moved[zs - zs.min(), ys - ys.min(), xs - xs.min()] = 1
        np.testing.assert_array_equal(cells_of(words), moved)
        assert shift == (-int(xs.min()), -int(ys.min()), -int(zs.min()))


def test_symbol_structs_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_isolate\(", header, flags=re.M)
    assert "ca3d_ensemble_isolate" in bound and hasattr(lib, "ca3d_ensemble_isolate")
    assert len(bound["ca3d_ensemble_isolate"]) == 8
    assert C.sizeof(_capi.IsolateJobStruct) == 8 and C.sizeof(_capi.IsolatedStruct) == 16
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    for name, value in _capi.ISOLATE_PLACEMENTS.items():
        assert re.search(r"CA3D_ISOLATE_%s = %d\b" % (name.upper(), value), header)
    assert re.search(r"^#define CA3D_ISOLATE_COPY_RULES 0x100u$", header, flags=re.M) and _capi.ISOLATE_COPY_RULES == 0x100
    assert tuple(_capi.ISOLATE_PLACEMENTS) == host.ISOLATE_PLACEMENTS


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.IsolatedStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    jobs = (_capi.IsolateJobStruct * 2)()
    assert lib.ca3d_ensemble_isolate(None, 0, None, 2, jobs, 1, out, None) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out)
