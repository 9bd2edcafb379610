"""`ca3d_ensemble_census` on the GPU (kernel ca_ensemble_census64, csrc/ca_census.hip) against `host.census`, the numpy restatement of
the definition in include/ca3d.h, of the uploaded or oracle state — never against the engine. Every comparison is exact: records byte
for byte, zero slots included. The crafted states are tests/census_cases.py's; tests/test_census_cpu.py checks `host.census` itself
against scipy."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import census_cases as cc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_moving import SHIP, glider, moore_rules

pytestmark = pytest.mark.gpu

G, W = 64, 8192
MOVING = 8


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def hold(ens, states, nb="moore"):
    """An ensemble that holds `states`; a census needs no rules."""
    ens.configure(len(states), neighbourhood=nb)
    ens.upload_state(0, np.stack(states))


def same(got, want, where):
    """One universe's (components, n, remaining) against the reference's, exactly."""
    (gc, gn, gr), (wc, wn, wr) = got, want
    assert (int(gn), int(gr)) == (int(wn), int(wr)), where
    if gc.tobytes() != wc.tobytes():
        bad = [i for i in range(len(wc)) if gc[i].tobytes() != wc[i].tobytes()]
        raise AssertionError(f"{where}: {len(bad)} records differ, the first at {bad[0]}: got {gc[bad[0]]}, expected {wc[bad[0]]}")


def check_named(ens, names, max_components, complete=None):
    hold(ens, [cc.state(n) for n in names])
    comps, n, rest = ens.census(max_components=max_components)
    assert comps.shape == (len(names), max_components) and comps.dtype == host.COMPONENT_DTYPE
    for u, name in enumerate(names):
        want = cc.reference(name, max_components)
        if complete is not None:
            assert (want[2] == 0) == complete, name  # on the reference's side first: a truncated list must not hide a difference
        same((comps[u], n[u], rest[u]), want, name)
    return comps, n, rest


def test_closed_faces(ens):
    """Cells on opposite faces, per axis, and all eight corners at once: 2, 2, 2 and 8 components — a wrapping shift joins them."""
    names = ["faces_x", "faces_y", "faces_z", "corners"]
    _, n, rest = check_named(ens, names, 16, complete=True)
    assert list(n) == [2, 2, 2, 8] and not rest.any()


def test_thirteen_directions_across_every_seam(ens):
    """Every direction up to sign, each pair across x = 31 | 32, a lane seam and a wave seam: one component at distance 1, two at 2."""
    names = [n for n in cc.CRAFTED if n.startswith("pairs")]
    assert len(names) == 26
    _, n, rest = check_named(ens, names, 16, complete=True)
    assert [int(v) for v in n] == [4 if name.startswith("pairs1") else 8 for name in names] and not rest.any()


def test_long_floods(ens):
    """The serpentine (about 2 000 iterations: a convergence test one iteration early or late shows here) and the staircase up and
    down through all 16 waves."""
    comps, n, rest = check_named(ens, ["serpentine", "staircase"], 4, complete=True)
    assert list(n) == [1, 1] and [int(p) for p in comps["population"][:, 0]] == [32 * 64 + 31, 129]


def test_shell_and_core(ens):
    comps, n, _ = check_named(ens, ["shell_core"], 8, complete=True)
    assert int(n[0]) == 2 and [int(p) for p in comps["population"][0, :2]] == [386, 27]
    assert comps["first_cell"][0, 0] < comps["first_cell"][0, 1]


def test_translation(ens):
    names = ["shape_0", "shape_1", "shape_2", "shapes"]
    comps, n, _ = check_named(ens, names, 8, complete=True)
    assert list(n) == [1, 1, 1, 3]
    digests = [int(comps["digest"][u, 0]) for u in range(3)] + [int(d) for d in comps["digest"][3, :3]]
    assert len(set(digests)) == 1 and digests[0] == host.state_summary(G, host.cells_to_words(G, cc.SHAPE))["digest"]
    assert [int(comps["population"][u, 0]) for u in range(3)] == [12] * 3
    for u, place in enumerate(cc.PLACES):
        assert host.unpack_box(comps["box_min"][u, 0]) == place
        assert host.unpack_box(comps["box_max"][u, 0]) == (place[0] + 5, place[1] + 2, place[2] + 3)


def test_whole_universe(ens):
    comps, n, rest = check_named(ens, ["full", "empty"], 4, complete=True)
    assert list(n) == [1, 0] and list(rest) == [0, 0]
    c = comps[0, 0]
    assert int(c["population"]) == 262144 and host.unpack_box(c["box_min"]) == (0, 0, 0) and host.unpack_box(c["box_max"]) == (63, 63, 63)
    assert int(c["digest"]) == host.state_summary(G, cc.state("full"))["digest"]


def test_synthetic_complete(ens):
    """509 components of 518 cells at 1024; 190 components with one giant of 1 306 at 256."""
    comps, n, rest = check_named(ens, ["sparse"], 1024, complete=True)
    assert (int(n[0]), int(comps["population"].sum()), int(comps["population"].max())) == (509, 518, 2)
    comps, n, rest = check_named(ens, ["giant"], 256, complete=True)
    assert (int(n[0]), int(comps["population"].sum()), int(comps["population"].max())) == (190, 1739, 1306)


def test_synthetic_truncated(ens):
    comps, n, rest = check_named(ens, ["sparse"], 256, complete=False)
    full = cc.reference("sparse", 1024)[0]
    assert int(n[0]) == 256 and int(rest[0]) == 518 - int(comps["population"].sum()) and comps[0].tobytes() == full[:256].tobytes()
    comps, n, rest = check_named(ens, ["dense"], 1024, complete=False)
    assert int(n[0]) == 1024 and int(rest[0]) == 16472 - int(comps["population"].sum())


def np_step(c):
    """Moore B6/S5-7 on cells [z, y, x], plain numpy (np.roll wraps; what is stepped here stays clear of the faces)."""
    n = sum(np.roll(c, d, axis=(0, 1, 2)).astype(np.int32) for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0))
    return (((c == 0) & (n == 6)) | ((c == 1) & (n >= 5) & (n <= 7))).astype(np.uint8)


def test_a_glider_beside_a_block(ens):
    """What the census is for: the doubled glider of tests/test_gpu_moving.py beside one 2 x 2 x 2 block. The universe as a whole is
    not a translated pattern — step_until_moving says nothing — and the census lists the ship, census after census."""
    block = [(10 + i, 10 + j, 40 + k) for i, j, k in itertools.product((0, 1), repeat=3)]
    first = glider("xy", (28, 30, 30)) | host.cells_to_words(G, block)
    # by a plain numpy step: the block is a still life, the glider keeps 10 cells and moves by (+1, +1, 0) every 4 steps
    cells = [np.unpackbits(first.view(np.uint8), bitorder="little").reshape(G, G, G)]
    for _ in range(12):
        cells.append(np_step(cells[-1]))
    for k in (4, 8, 12):
        ship_then, ship_now = cells[k - 4].copy(), cells[k].copy()
        for c in (ship_then, ship_now):
            assert c[40:42, 10:12, 10:12].all()
            c[40:42, 10:12, 10:12] = 0
            assert int(c.sum()) == 10
        assert np.array_equal(ship_now, np.roll(ship_then, (0, 1, 1), axis=(0, 1, 2)))
    rules = moore_rules(*SHIP)
    hold(ens, [first])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    state, lists = first, []
    for k in range(0, 13, 4):
        if k:
            ens.step(4)
            for _ in range(4):
                state = ol.packed_step(G, state, rules)
            np.testing.assert_array_equal(ens.read_state()[0], state)
        got = ens.census(max_components=8)
        same((got[0][0], got[1][0], got[2][0]), cc.reference_of(("glider+block", k), state, 8), f"step {k}")
        assert int(got[1][0]) == 2 and int(got[2][0]) == 0
        lists.append(got[0][0])
    for j, comps in enumerate(lists):
        shp, blk = comps[0], comps[1]  # the glider's first cell (z = 30) lies before the block's (z = 40)
        assert (int(shp["population"]), int(blk["population"])) == (10, 8)
        assert host.unpack_box(blk["box_min"]) == (10, 10, 40) and host.unpack_box(blk["box_max"]) == (11, 11, 41)
        assert blk["digest"] == lists[0][1]["digest"] and shp["digest"] == lists[0][0]["digest"] and blk["digest"] != shp["digest"]
        assert host.unpack_box(shp["box_min"]) == (28 + j, 30 + j, 30) and host.unpack_box(shp["box_max"]) == (30 + j, 32 + j, 31)
    done, reason, period, shift = ens.step_until_moving(64)
    assert not int(reason[0]) & MOVING and int(period[0]) == 0 and int(done[0]) == 64


ASH_MOORE = [("5-7", "4-6", 2), ("6", "5-7", 1)]
ASH_CLUSTERED = ("6", "5-7", "27", "27", "", "1-8")
ASH_VN = [("3", "2,3", 2), ("2,4", "1,3,5", 5)]
KEYS = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")


def check_ash(ens, what):
    done, reason, period = ens.step_until_cycle(512)
    states = ens.read_state()
    comps, n, rest = ens.census(max_components=1024)
    for u in range(ens.n):
        want = host.census(states[u], 1024)
        assert want[2] == 0, (what, u)  # complete on the reference's side
        same((comps[u], n[u], rest[u]), want, f"{what}, universe {u} ({int(done[u])} steps, reason {int(reason[u])}, {int(want[1])} components)")
    np.testing.assert_array_equal(ens.read_state(), states)


@pytest.mark.parametrize("rule", ASH_MOORE)
def test_ash_moore(ens, rule):
    ens.configure(8, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=rule[0], survive=rule[1])
    ens.seed_states(0, np.arange(101, 109), rule[2])
    check_ash(ens, rule)


def test_ash_clustered(ens):
    ens.configure(8, neighbourhood="moore", clustered=True)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", **dict(zip(KEYS, ASH_CLUSTERED)))
    ens.seed_states(0, np.arange(101, 109), 1)
    check_ash(ens, ASH_CLUSTERED)


@pytest.mark.parametrize("rule", ASH_VN)
def test_ash_von_neumann(ens, rule):
    ens.configure(8, neighbourhood="von neumann")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, born=rule[0], survive=rule[1])
    ens.seed_states(0, np.arange(101, 109), rule[2])
    check_ash(ens, rule)


def test_range_and_scale(ens):
    """300 universes, more than compute units, universe u holding crafted state u % k; the whole range and a range inside it."""
    names = [n for n in cc.CRAFTED if n != "serpentine"] + ["giant"]
    B = 300
    hold(ens, [cc.state(names[u % len(names)]) for u in range(B)])
    for first, count in ((0, 300), (37, 5)):
        comps, n, rest = ens.census(first, count, 16)
        assert comps.shape == (count, 16) and n.shape == (count,) and rest.shape == (count,)
        for k in range(count):
            name = names[(first + k) % len(names)]
            same((comps[k], n[k], rest[k]), cc.reference(name, 16), f"universe {first + k} ({name})")
    assert ens.census_gpu_ms() > 0.0


def test_read_only(ens):
    """States and records before and after a census are identical, a step afterwards matches the oracle, and a census between two
    step_until_cycle calls — and one behind a call that was cut into two launches — changes neither steps_done nor period."""
    case = ("5", "4,5")
    rules = moore_rules(*case)
    first = [host.random_fill(W, seed=2, and_rounds=2), glider("xy", (28, 30, 30)), cc.state("shell_core")]

    def fresh():
        hold(ens, first)
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=case[0], survive=case[1])

    fresh()
    ens.step(3)
    before, records = ens.read_state(), ens.summaries()
    ens.census(max_components=1024)
    ens.census(1, 2, 1)
    np.testing.assert_array_equal(ens.read_state(), before)
    assert ens.summaries() == records
    ens.step(5)
    got = ens.read_state()
    for u, s in enumerate(first):
        np.testing.assert_array_equal(got[u], ol.packed_run(G, s, rules, 8), err_msg=f"universe {u}")
    assert [s.step for s in ens.summaries()] == [8, 8, 8]
    # the same two calls with and without a census in between; the second call is 70 000 steps at most: two launches
    runs = []
    for with_census in (False, True):
        fresh()
        a = ens.step_until_cycle(20, check_every=4)
        if with_census:
            ens.census(max_components=64)
        b = ens.step_until_cycle(70000, check_every=9001)
        if with_census:
            ens.census(max_components=64)
        runs.append([[int(v) for v in arr] for arr in a + b] + [ens.read_state().tobytes(), ens.summaries()])
    assert runs[0] == runs[1]


def test_refusals(ens):
    lib = _capi.load()
    out = (_capi.ComponentStruct * 8)()
    C.memset(out, 0x5A, C.sizeof(out))
    n, rest = (C.c_uint32 * 2)(77, 77), (C.c_uint32 * 2)(77, 77)
    ms = C.c_float(-1.0)

    def refused(code, pattern, *args):
        assert lib.ca3d_ensemble_census(ens._h, *args) == code, args
        msg = lib.ca3d_last_error().decode()
        assert re.search(pattern, msg), (args, msg)
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(n) == [77, 77] and list(rest) == [77, 77] and ms.value == -1.0, args

    refused(-2, "configure", 0, 1, 4, out, n, rest, C.byref(ms))  # before configure
    ens.configure(3, neighbourhood="moore")
    refused(-2, "universe 0", 0, 2, 4, out, n, rest, C.byref(ms))  # no state anywhere
    ens.upload_state(0, np.zeros((1, W), dtype=np.uint32))
    refused(-2, "universe 1", 0, 2, 4, out, n, rest, C.byref(ms))  # universe 1 has none
    ens.upload_state(1, np.zeros((2, W), dtype=np.uint32))
    refused(-1, "universes", 0, 0, 4, out, n, rest, C.byref(ms))  # count 0
    refused(-1, "universes", 2, 2, 4, out, n, rest, C.byref(ms))  # past n
    refused(-1, "universes", 3, 1, 4, out, n, rest, C.byref(ms))
    refused(-1, "max_components", 0, 2, 0, out, n, rest, C.byref(ms))
    refused(-1, "max_components", 0, 2, 1025, out, n, rest, C.byref(ms))
    refused(-1, "NULL", 0, 2, 4, None, n, rest, C.byref(ms))
    refused(-1, "NULL", 0, 2, 4, out, None, rest, C.byref(ms))
    refused(-1, "NULL", 0, 2, 4, out, n, None, C.byref(ms))
    for kw in (dict(count=0), dict(first=2, count=2), dict(max_components=0), dict(max_components=1025)):
        with pytest.raises(Ca3dError) as e:
            ens.census(**kw)
        assert e.value.code == -1, kw
    # and the call that is not refused: gpu_ms may be NULL
    assert lib.ca3d_ensemble_census(ens._h, 0, 2, 4, out, n, rest, None) == 0
    assert list(n) == [0, 0] and list(rest) == [0, 0] and not bytes(out).strip(b"\0")
