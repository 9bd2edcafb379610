"""`ca3d_ensemble_census_connected` with CA3D_CONNECT_TORUS on the GPU (kernel ca_ensemble_census64_torus, csrc/ca_objects_torus.hip)
against `host.census(..., connectivity="torus")`, the numpy restatement of the definition in include/ca3d.h, of the uploaded or read
state — never against the engine. Every comparison is exact: records byte for byte, zero slots, n_components and remaining included.
The states are tests/objects_torus_cases.py's; tests/test_census_torus_cpu.py checks the host definition itself against scipy."""
import ctypes as C
import re

import numpy as np
import pytest

import census_cases as cc
import objects_torus_cases as tc
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_census import hold, same

pytestmark = pytest.mark.gpu

G, W = 64, 8192


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def check(ens, keyed, max_components, complete=True):
    """An ensemble of the states [(key, words)]: the torus census of all, each against the host definition."""
    hold(ens, [w for _, w in keyed])
    comps, n, rest = ens.census(max_components=max_components, connectivity="torus")
    assert comps.shape == (len(keyed), max_components) and comps.dtype == host.COMPONENT_DTYPE
    for u, (key, w) in enumerate(keyed):
        want = tc.reference(key, w, max_components)
        assert (want[2] == 0) == complete, key  # on the reference's side first
        same((comps[u], n[u], rest[u]), want, str(key))
    return comps, n, rest


def test_thirteen_directions_through_a_seam(ens):
    """Two cells that touch only through a face, an edge or a corner of the cube: one object on the torus, two in the closed cube,
    on the same handle."""
    keyed = [(("seam", d), host.cells_to_words(G, tc.seam_pair(d))) for d in tc.DIRECTIONS]
    comps, n, rest = check(ens, keyed, 4)
    assert [int(v) for v in n] == [1] * 13 and not rest.any() and [int(p) for p in comps["population"][:, 0]] == [2] * 13
    for u, d in enumerate(tc.DIRECTIONS):
        lo, hi = host.unpack_box(comps["box_min"][u, 0]), host.unpack_box(comps["box_max"][u, 0])
        assert [v == 63 and w == 64 for v, w in zip(lo, hi)] == [s != 0 for s in d], d  # the box runs through exactly those seams
    closed = ens.census(max_components=4, connectivity="closed")
    assert [int(v) for v in closed[1]] == [2] * 13
    for u, (_, w) in enumerate(keyed):
        same((closed[0][u], closed[1][u], closed[2][u]), host.census(w, 4), f"closed, universe {u}")
    assert len({int(v) for v in comps["digest"][:4, 0]}) == 4  # a pair along x is not a pair along y


@pytest.mark.parametrize("d", tc.ROLLS)
def test_rolled_crafted_states(ens, d):
    """census_cases' states rolled: every object crosses the word seam, a wave seam or a face. The states that were clear of the faces
    keep their shapes' names."""
    keyed = [((name, d), tc.state(name, d)) for name in tc.ROLLED]
    comps, n, rest = check(ens, keyed, 16)
    got = dict(zip(tc.ROLLED, range(len(tc.ROLLED))))
    assert [int(n[got[k]]) for k in ("faces_x", "faces_y", "faces_z", "corners", "serpentine", "staircase")] == [1] * 6
    assert int(comps["population"][got["serpentine"], 0]) == 2079 and int(comps["population"][got["corners"], 0]) == 8
    for name in tc.CLEAR:
        u = got[name]
        assert tc.shapes((comps[u], int(n[u]), int(rest[u]))) == tc.shapes(cc.reference(name, 16)), name


def test_rings_and_rings_with_a_gap(ens):
    keyed, want = [], []
    for axis in range(3):
        for missing, start in (((), 0), ((0,), 1), ((63,), 0), ((31, 32), 33)):
            keyed.append((("rod", axis, missing), host.cells_to_words(G, tc.rod(axis, missing))))
            want.append((axis, start, start + 63 - len(missing), 64 - len(missing)))
    comps, n, rest = check(ens, keyed, 4)
    assert [int(v) for v in n] == [1] * 12
    for u, (axis, lo, hi, pop) in enumerate(want):
        bmin, bmax = host.unpack_box(comps["box_min"][u, 0]), host.unpack_box(comps["box_max"][u, 0])
        assert (bmin[axis], bmax[axis], int(comps["population"][u, 0])) == (lo, hi, pop), want[u]
        others = [a for a in range(3) if a != axis]
        assert all(bmin[a] == bmax[a] == (21, 38, 10)[a] for a in others)
    assert int(comps["box_max"][3, 0]) & 0xFF == 94  # the ring around x with 31 and 32 missing: 33 .. 94


def test_whole_and_empty_universe(ens):
    comps, n, rest = check(ens, [("full", cc.state("full")), ("empty", cc.state("empty"))], 4)
    assert list(n) == [1, 0] and list(rest) == [0, 0]
    c = comps[0, 0]
    assert int(c["population"]) == 262144 and host.unpack_box(c["box_min"]) == (0, 0, 0) and host.unpack_box(c["box_max"]) == (63, 63, 63)
    assert int(c["digest"]) == host.state_summary(G, cc.state("full"))["digest"]


def test_truncated_lists(ens):
    soup = tc.state("soup", (40, 50, 60))
    comps, n, rest = check(ens, [(("soup", (40, 50, 60)), soup), (("shapes", tc.ROLLS[1]), tc.state("shapes", tc.ROLLS[1]))], 1, complete=False)
    assert list(n) == [1, 1] and int(rest[1]) == 24 and int(rest[0]) > 0
    dense = cc.state("dense")  # a whole cube at density 1 / 16: thousands of objects
    comps, n, rest = check(ens, [("dense", dense)], 1024, complete=False)
    assert int(n[0]) == 1024 and int(rest[0]) == 16472 - int(comps["population"].sum()) and int(rest[0]) > 0


SOUP_ROLLS = ((0, 0, 0), (30, 0, 0), (0, 31, 5), (40, 50, 60), (33, 1, 63))


def six_soups():
    """Five rolls of the soup — at most one clear of the faces — and the rolled giant."""
    return [(("soup", d), tc.state("soup", d)) for d in SOUP_ROLLS] + [(("giant", (33, 1, 63)), tc.state("giant", (33, 1, 63)))]


@pytest.mark.parametrize("B", [1, 3])
def test_small_ensembles(ens, B):
    comps, n, rest = check(ens, six_soups()[3:3 + B], 1024)
    assert int(n.min()) > 100


def test_a_range_of_a_large_ensemble(ens):
    """310 universes, more than compute units, universe u holding soup u % 6; the census of 300 of them from universe 7 on."""
    soups = six_soups()
    hold(ens, [soups[u % 6][1] for u in range(310)])
    comps, n, rest = ens.census(7, 300, 1024, connectivity="torus")
    assert comps.shape == (300, 1024) and n.shape == (300,) and rest.shape == (300,)
    for k in range(300):
        key, w = soups[(7 + k) % 6]
        same((comps[k], n[k], rest[k]), tc.reference(key, w, 1024), f"universe {7 + k} {key}")
    assert ens.census_gpu_ms() > 0.0
    # the rolls of one soup hold the same shapes, and that is what the closed census of the one clear of the faces lists
    want = tc.shapes(tc.reference(("soup", "closed"), tc.state("soup"), 1024, "closed"))
    for k in range(6):
        if (7 + k) % 6 < 5:
            assert tc.shapes((comps[k], int(n[k]), int(rest[k]))) == want, soups[(7 + k) % 6][0]


def test_ash_of_torus_soups(ens):
    """What it is for: Moore B6/S5-7 soups under the torus boundary, the census queued behind the steps without a wait in between."""
    ens.configure(4, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="6", survive="5-7")
    ens.seed_states(0, np.arange(101, 105), 1)
    ens.set_boundary("torus")
    joined = 0
    for steps, how in ((30, "torus"), (34, "boundary")):
        ens.step(steps)
        comps, n, rest = ens.census(max_components=1024, connectivity=how)
        closed = ens.census(max_components=1024)  # the default keeps the closed cube under every boundary
        states = ens.read_state()
        for u in range(ens.n):
            want = host.census(states[u], 1024, "torus")
            assert want[2] == 0 and want[1] > 10, (steps, u)  # complete on the reference's side, and not empty
            same((comps[u], n[u], rest[u]), want, f"after {steps} steps, universe {u} ({int(want[1])} objects)")
            same((closed[0][u], closed[1][u], closed[2][u]), host.census(states[u], 1024), f"closed, after {steps} steps, universe {u}")
            assert int(n[u]) <= int(closed[1][u])
        joined += int(closed[1].sum()) - int(n.sum())
    assert joined > 0  # objects the closed census split at a face
    ens.set_boundary("reference")
    same_as_closed = ens.census(max_components=1024, connectivity="boundary")
    assert same_as_closed[0].tobytes() == closed[0].tobytes()
    with pytest.raises(ValueError):
        ens.census(connectivity="open")


def test_closed_through_the_new_entry_point(ens):
    lib = _capi.load()
    names = ["faces_x", "corners", "shapes", "shell_core", "giant"]
    hold(ens, [cc.state(n) for n in names])
    results = []
    for new in (False, True):
        out = (_capi.ComponentStruct * (5 * 16))()
        C.memset(out, 0x5A, C.sizeof(out))
        n, rest = (C.c_uint32 * 5)(), (C.c_uint32 * 5)()
        args = (out, n, rest, None)
        rc = lib.ca3d_ensemble_census_connected(ens._h, 0, 5, 16, 0, *args) if new else lib.ca3d_ensemble_census(ens._h, 0, 5, 16, *args)
        assert rc == 0
        results.append((bytes(out), list(n), list(rest)))
    assert results[0] == results[1]
    for u, name in enumerate(names):
        want = cc.reference(name, 16)
        assert results[1][0][u * 512:(u + 1) * 512] == want[0].tobytes() and (results[1][1][u], results[1][2][u]) == (want[1], want[2])


def test_read_only(ens):
    hold(ens, [tc.state("shapes", tc.ROLLS[1]), tc.state("soup", (33, 1, 63))])
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="6", survive="5-7")
    ens.set_boundary("torus")
    ens.step(3)
    before, records = ens.read_state(), ens.summaries()
    ens.census(max_components=1024, connectivity="torus")
    ens.census(1, 1, 1, connectivity="torus")
    np.testing.assert_array_equal(ens.read_state(), before)
    assert ens.summaries() == records and ens.boundary == "torus"
    ens.step(2)
    for u in range(2):
        want = before[u]
        for _ in range(2):
            want = host.ensemble_step(want, "moore", (1 << 6, 0b111 << 5), "torus")
        np.testing.assert_array_equal(ens.read_state()[u], want)
    assert [s.step for s in ens.summaries()] == [5, 5]


def test_refusals(ens):
    lib = _capi.load()
    out = (_capi.ComponentStruct * 8)()
    C.memset(out, 0x5A, C.sizeof(out))
    n, rest = (C.c_uint32 * 2)(77, 77), (C.c_uint32 * 2)(77, 77)
    ms = C.c_float(-1.0)

    def refused(code, pattern, first, count, max_components, connectivity, *args):
        assert lib.ca3d_ensemble_census_connected(ens._h, first, count, max_components, connectivity, *args) == code, (first, count, max_components)
        msg = lib.ca3d_last_error().decode()
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(n) == [77, 77] and list(rest) == [77, 77] and ms.value == -1.0, msg

    refused(-2, "configure", 0, 1, 4, 1, out, n, rest, C.byref(ms))  # before configure
    ens.configure(3, neighbourhood="moore")
    refused(-2, "universe 0", 0, 2, 4, 1, out, n, rest, C.byref(ms))  # no state anywhere
    ens.upload_state(0, np.zeros((1, W), dtype=np.uint32))
    refused(-2, "universe 1", 0, 2, 4, 1, out, n, rest, C.byref(ms))  # universe 1 has none
    ens.upload_state(1, np.zeros((2, W), dtype=np.uint32))
    refused(-1, "universes", 0, 0, 4, 1, out, n, rest, C.byref(ms))  # count 0
    refused(-1, "universes", 2, 2, 4, 1, out, n, rest, C.byref(ms))  # past n
    refused(-1, "universes", 3, 1, 4, 1, out, n, rest, C.byref(ms))
    refused(-1, "max_components", 0, 2, 0, 1, out, n, rest, C.byref(ms))
    refused(-1, "max_components", 0, 2, 1025, 1, out, n, rest, C.byref(ms))
    refused(-1, "NULL", 0, 2, 4, 1, None, n, rest, C.byref(ms))
    refused(-1, "NULL", 0, 2, 4, 1, out, None, rest, C.byref(ms))
    refused(-1, "NULL", 0, 2, 4, 1, out, n, None, C.byref(ms))
    refused(-1, r"connectivity 2\b", 0, 2, 4, 2, out, n, rest, C.byref(ms))
    refused(-1, r"connectivity 4294967295\b", 0, 2, 4, 0xFFFFFFFF, out, n, rest, C.byref(ms))
    for kw in (dict(count=0), dict(first=2, count=2), dict(max_components=0), dict(max_components=1025)):
        with pytest.raises(Ca3dError) as e:
            ens.census(connectivity="torus", **kw)
        assert e.value.code == -1, kw
    # and the call that is not refused: gpu_ms may be NULL
    assert lib.ca3d_ensemble_census_connected(ens._h, 0, 2, 4, 1, out, n, rest, None) == 0
    assert list(n) == [0, 0] and list(rest) == [0, 0] and not bytes(out).strip(b"\0")
