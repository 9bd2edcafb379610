"""`ca3d_ensemble_compose` on the GPU (kernel ca_ensemble_compose64, csrc/ca_compose.hip) against `host.compose`, the numpy restatement
of the definition in include/ca3d.h. Every comparison is exact: the destinations' states word for word, the four counters of every
record, the destinations' summaries (step 0, population, box, digest, no previous state) and the untouched source. The crafted states
are tests/census_cases.py's; tests/test_compose_cpu.py checks `host.compose` itself against np.transpose + np.flip."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import census_cases as cc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_census import KEYS
from test_gpu_moving import MOVING, SHIP, glider, moore_rules

pytestmark = pytest.mark.gpu

G, W = 64, 8192
ALL48 = list(range(48))
#: one orientation of each of the six permutations, with mixed flips: f = 5, 2, 3, 6, 1, 4
MIXED = [0 + 6 * 5, 1 + 6 * 2, 2 + 6 * 3, 3 + 6 * 6, 4 + 6 * 1, 5 + 6 * 4]


def cells_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def box_min(words):
    zs, ys, xs = np.nonzero(cells_of(words))
    return (int(xs.min()), int(ys.min()), int(zs.min())) if zs.size else (0, 0, 0)


def inverse(o):
    return host.orientation_from_matrix(host.orientation_matrix(o).T)


def make_ensemble():
    from cellularautomatons3d_amd import Ensemble

    return Ensemble(0)


@pytest.fixture()
def ens():
    e = make_ensemble()
    yield e
    e.close()


@pytest.fixture()
def stage():
    e = make_ensemble()
    yield e
    e.close()


def hold(e, states, nb="moore", clustered=False):
    e.configure(len(states), neighbourhood=nb, clustered=clustered)
    e.upload_state(0, np.stack(states))


def check_record(s, words, where):
    """A destination's summary: what an upload of `words` leaves (step 0, no previous state)."""
    want = host.state_summary(G, words)
    assert s.step == 0 and not s.has_previous and (s.births, s.deaths) == (0, 0), where
    assert s.population == want["population"] and s.digest == want["digest"], where
    if want["population"]:
        assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


def compose_and_check(dst, src, layouts, states, dst_first=0, over=False, copy_rules=False, bases=None, want=None):
    """One call; destination k against host.compose(states, layouts[k], bases[k]) — or want[k], a (words, record) computed before.
    `src` None: one handle. -> (records, the destinations' states)."""
    source = dst if src is None else src
    sources = sorted({u for layout in layouts for u, _, _ in layout})
    before = [(source.read_state(u, 1).tobytes(), source.summaries(u, 1)) for u in sources]
    recs = dst.compose(layouts, dst_first, src, over, copy_rules)
    n = len(layouts)
    assert recs.shape == (n,) and recs.dtype == host.COMPOSED_DTYPE
    got, sums = dst.read_state(dst_first, n), dst.summaries(dst_first, n)
    for k, layout in enumerate(layouts):
        where = f"destination {k}: {layout}"
        words, rec = want[k] if want is not None else host.compose(states, layout, None if bases is None else bases[k])
        assert recs[k].tolist() == rec.tolist(), (where, recs[k], rec)
        np.testing.assert_array_equal(got[k], words, err_msg=where)
        check_record(sums[k], words, where)
    assert [(source.read_state(u, 1).tobytes(), source.summaries(u, 1)) for u in sources] == before  # the source is only read
    assert dst.compose_gpu_ms() > 0.0
    return recs, got


def test_identity_on_every_crafted_state(ens, stage):
    """Orientation 0 at box_min reproduces the piece: every crafted state of the census tests, the full and the empty universe among them."""
    names = list(cc.CRAFTED)
    states = [cc.state(n) for n in names]
    hold(ens, states)
    stage.configure(len(names), neighbourhood="von neumann")  # without COPY_RULES the two may differ in kind
    layouts = [[(u, 0, box_min(s))] for u, s in enumerate(states)]
    recs, got = compose_and_check(stage, ens, layouts, states)
    np.testing.assert_array_equal(got, np.stack(states))
    for u, name in enumerate(names):
        pop = int(cells_of(states[u]).sum())
        assert recs[u].tolist() == (pop, pop, 0, 0), name


@pytest.mark.parametrize("place", range(len(cc.PLACES)))
def test_shape_in_all_48_orientations(ens, stage, place):
    """SHAPE, taken from each of PLACES — (27, 40, 2) straddles the word seam — and put back there turned, 48 destinations a launch;
    and once more at a place where x, y and z are cut by a face."""
    state = cc.state("shape_%d" % place)
    hold(ens, [cc.state("empty"), state])
    stage.configure(48, neighbourhood="moore")
    compose_and_check(stage, ens, [[(1, o, cc.PLACES[place])] for o in ALL48], [None, state])
    recs, got = compose_and_check(stage, ens, [[(1, o, (61, -1, 60))] for o in ALL48], [None, state])
    assert len({g.tobytes() for g in got}) > 24 and int(recs["clipped"].min()) > 0


def test_serpentine_and_staircase_in_all_48_orientations(ens, stage):
    """The serpentine (one plane, every row, both words) and the staircase (all 64 planes, all 16 waves): turned they run along every
    axis, through every wave and both words of the destination."""
    states = [cc.state("serpentine"), cc.state("staircase")]
    hold(ens, states)
    stage.configure(96, neighbourhood="moore")
    recs, _ = compose_and_check(stage, ens, [[(u, o, (0, 0, 0))] for u in (0, 1) for o in ALL48], states)
    assert not recs["clipped"].any()  # both fit the cube whichever way they are turned
    recs, _ = compose_and_check(stage, ens, [[(u, o, (9, -2, 5))] for u in (0, 1) for o in ALL48], states)
    assert recs["clipped"].all() and recs["placed"].any()  # (the serpentine's plane, put at -2, is outside altogether)


def test_full_universe(ens, stage):
    """The full universe is its own image under all 48: at the origin it is full, one cell off a face loses one plane of 4096 cells,
    64 cells off loses all."""
    full = cc.state("full")
    hold(ens, [full])
    stage.configure(48, neighbourhood="moore")
    ats = [(0, 0, 0)] + [tuple(s * d * (axis == i) for i in range(3)) for axis in range(3) for s in (1, -1) for d in (1, 64)]
    assert len(ats) == 13
    for at in ats:
        want = host.compose([full], [(0, 0, at)])
        other = host.compose([full], [(0, 47, at)])
        assert want[0].tobytes() == other[0].tobytes() and want[1].tobytes() == other[1].tobytes()
        lost = G ** 3 if 64 in at or -64 in at else 4096 * sum(1 for v in at if v)
        assert want[1].tolist() == (G ** 3 - lost, G ** 3 - lost, 0, lost), at
        compose_and_check(stage, ens, [[(0, o, at)] for o in ALL48], [full], want=[want] * 48)


def test_shape_through_each_of_the_six_faces(ens, stage):
    """SHAPE pushed out through every face cell by cell, under one orientation of each of the six permutations with mixed flips."""
    state = cc.state("shape_1")
    hold(ens, [state])
    layouts = []
    for o in MIXED:
        extent = [abs(int(v)) for v in host.orientation_matrix(o) @ np.array([6, 3, 4])]
        for axis in range(3):
            for k in range(extent[axis] + 1):
                low, high = [20, 30, 40], [20, 30, 40]
                low[axis], high[axis] = -k, G - extent[axis] + k
                layouts += [[(0, o, tuple(low))], [(0, o, tuple(high))]]
    stage.configure(len(layouts), neighbourhood="moore")
    recs, _ = compose_and_check(stage, ens, layouts, [state])
    clipped = sorted(set(int(c) for c in recs["clipped"]))
    assert clipped[0] == 0 and clipped[-1] == 12 and len(clipped) > 6


def test_300_soups(ens, stage):
    """The dense case, where every bit of the gather matters: 300 destinations — more than compute units — of 8 soups under orientation
    k % 48, put anywhere from -64 to 64, into universes 5 .. 304 of 310: the universes around the range keep what they held."""
    soups = [host.random_fill(W, seed=21 + u, and_rounds=1) for u in range(8)]
    hold(ens, soups)
    rng = np.random.default_rng(0xCA3D)
    layouts = [[(k % 8, k % 48, tuple(int(v) for v in rng.integers(-64, 65, size=3)))] for k in range(300)]
    for k in range(48):  # the first round near the origin, so that most of every soup lands inside
        layouts[k] = [(k % 8, k, tuple(int(v) for v in rng.integers(-3, 4, size=3)))]
    marker = host.random_fill(W, seed=5, and_rounds=3)
    stage.configure(310, neighbourhood="moore")
    stage.upload_state(0, np.stack([marker] * 5))
    stage.upload_state(305, np.stack([marker] * 5))
    recs, _ = compose_and_check(stage, ens, layouts, soups, dst_first=5)
    # (and_rounds 1: a quarter of the cells, 65 536 a soup; three cells off on every axis keep (61 / 64)^3 of them)
    assert int(recs["placed"][:48].min()) > 50000 and int(recs["clipped"].max()) > 50000
    for u in (0, 4, 305, 309):
        np.testing.assert_array_equal(stage.read_state(u, 1)[0], marker)
        check_record(stage.summaries(u, 1)[0], marker, u)
    # a smaller call afterwards reuses the staging array
    compose_and_check(stage, ens, layouts[100:105], soups, dst_first=200)


def test_several_parts(ens, stage):
    """One to five parts a destination from different sources; two copies one cell apart overlap; the order of the parts does not
    matter; a destination without parts is empty."""
    names = ["shape_0", "shell_core", "staircase", "corners", "pairs1_+-+"]
    states = [cc.state(n) for n in names]
    hold(ens, states)
    rng = np.random.default_rng(7)
    layouts = []
    for n in (1, 2, 3, 4, 5):
        for _ in range(4):
            layouts.append([(int(rng.integers(0, 5)), int(rng.integers(0, 48)), tuple(int(v) for v in rng.integers(-10, 50, size=3))) for _ in range(n)])
    twice = [(0, 13, (30, 30, 30)), (0, 13, (31, 30, 30))]
    five = layouts[-1]
    layouts += [twice, twice[::-1], [], five[::-1], [five[2], five[0], five[4], five[1], five[3]], []]
    stage.configure(len(layouts), neighbourhood="moore")
    stage.upload_state(0, np.stack([cc.state("full")] * len(layouts)))  # what is there goes away, also where nothing is put
    recs, got = compose_and_check(stage, ens, layouts, states)
    k = len(layouts) - 6
    assert int(recs[k]["overlap"]) > 0 and int(recs[k]["placed"]) == 24 and recs[k].tolist() == recs[k + 1].tolist()
    assert got[k].tobytes() == got[k + 1].tobytes()
    assert not got[k + 2].any() and not got[-1].any() and recs[k + 2].tolist() == (0, 0, 0, 0)
    assert got[k - 1].tobytes() == got[k + 3].tobytes() == got[k + 4].tobytes()
    assert recs[k - 1].tolist() == recs[k + 3].tolist() == recs[k + 4].tolist()


def test_over_a_stepped_soup(ens, stage):
    """OVER: the pieces land on the destination's current state — the steps queued in front of the call are done — and the overlap is
    counted; a destination without parts stays as it is. Without the flag the old contents are gone."""
    rules = moore_rules("5", "4,5")
    soups = [host.random_fill(W, seed=31 + u, and_rounds=2) for u in range(3)]
    stepped = [ol.packed_run(G, s, rules, 3) for s in soups]
    pieces = [cc.state("shell_core"), cc.state("full")]
    hold(ens, pieces)
    hold(stage, soups)
    stage.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="5", survive="4,5")
    stage.step(3)  # queued, not synchronised
    layouts = [[(0, 9, (20, 20, 20)), (0, 0, (-3, 5, 50))], [], [(1, 0, (32, 0, 0))]]
    recs, got = compose_and_check(stage, ens, layouts, pieces, over=True, bases=stepped)
    np.testing.assert_array_equal(got[1], stepped[1])
    assert recs[1].tolist() == (int(cells_of(stepped[1]).sum()), 0, 0, 0)
    assert int(recs[0]["overlap"]) > 0 and int(recs[2]["overlap"]) == int(cells_of(stepped[2])[:, :, 32:].sum()) > 0
    assert [s.step for s in stage.summaries()] == [0, 0, 0]
    recs, got = compose_and_check(stage, ens, layouts, pieces)
    assert not got[1].any() and not recs["overlap"].any()
    stage.step(2)  # the rules are still there
    np.testing.assert_array_equal(stage.read_state(0, 1)[0], ol.packed_run(G, host.compose(pieces, layouts[0])[0], rules, 2))


KINDS = {
    # kind -> (configure arguments, two rules as set_rule_strings arguments): 2, 6 and 1 rule words a universe
    "moore": (dict(neighbourhood="moore"), [dict(born="6", survive="5-7"), dict(born="5", survive="4,5")]),
    "clustered": (dict(neighbourhood="moore", clustered=True),
                  [dict(zip(KEYS, ("6", "5-7", "27", "27", "", "1-8"))), dict(zip(KEYS, ("5", "4,5", "3", "27", "27", "2")))]),
    "von neumann": (dict(neighbourhood="von neumann"), [dict(born="3", survive="2,3"), dict(born="2,4", survive="1,3,5")]),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_rules_follow_the_first_part(ens, stage, kind):
    """Source universes alternate between two rules; a destination takes its FIRST part's, whatever its other parts bring: after four
    steps every destination is the oracle's under that rule. Without the flag the destinations keep their own."""
    conf, two = KINDS[kind]
    nb = conf["neighbourhood"]
    soups = [host.random_fill(W, seed=41 + u, and_rounds=2) for u in range(4)]
    ens.configure(4, **conf)
    ens.upload_state(0, np.stack(soups))
    for u in range(4):
        ens.set_rule_strings(u, neighbourhood=nb, **two[u % 2])
    layouts = [[(3, 5, (0, 1, 2)), (0, 0, (7, 7, 7))], [(0, 17, (-5, 0, 3)), (1, 2, (1, 1, 1))], [(1, 40, (2, 2, -9))], [(2, 0, (0, 0, 0)), (3, 3, (4, 5, 6))]]
    stage.configure(len(layouts), **conf)
    compose_and_check(stage, ens, layouts, soups, copy_rules=True)
    stage.step(4)
    got = stage.read_state()
    differ = 0
    for k, layout in enumerate(layouts):
        start = host.compose(soups, layout)[0]
        mine, other = (ol.Rules.from_strings(neighbourhood=nb, **two[(layout[0][0] + i) % 2]) for i in (0, 1))
        want = ol.packed_run(G, start, mine, 4)
        np.testing.assert_array_equal(got[k], want, err_msg=f"destination {k} under rule {two[layout[0][0] % 2]}")
        differ += not np.array_equal(want, ol.packed_run(G, start, other, 4))
    assert differ  # the two rules tell the universes apart: a destination that took the wrong one would show
    # without the flag: rules of its own stay
    stage.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood=nb, **two[0])
    compose_and_check(stage, ens, layouts[2:3], soups, copy_rules=False)  # its source's rule is two[1]
    stage.step(4)
    start = host.compose(soups, layouts[2])[0]
    np.testing.assert_array_equal(stage.read_state(0, 1)[0], ol.packed_run(G, start, ol.Rules.from_strings(neighbourhood=nb, **two[0]), 4))
    # ... and a stage without rules has none afterwards: it has states, and still refuses to step
    stage.configure(2, **conf)
    compose_and_check(stage, ens, layouts[:2], soups, copy_rules=False)
    with pytest.raises(Ca3dError) as e:
        stage.step(1)
    assert e.value.code == -2 and "set_rules" in str(e.value)
    # with the flag a destination WITHOUT parts gets none either
    stage.compose([layouts[0], []], 0, ens, False, True)
    with pytest.raises(Ca3dError) as e:
        stage.step(1)
    assert e.value.code == -2 and "1 of 2" in str(e.value)
    stage.compose([layouts[0]], 1, ens, False, True)
    stage.step(1)
    stage.synchronize()


def test_the_glider_in_all_48_orientations(ens, stage):
    """The doubled glider (Moore B6/S5-7), composed in all 48 orientations near the centre with its rule: step_until_moving stops every
    universe with MOVING, a period that is a multiple of 4 and the shift orient_vector(o, (1, 1, 0)) a period of 4."""
    ship = glider("xy", (28, 30, 30))
    hold(ens, [ship])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    stage.configure(48, neighbourhood="moore")
    recs, got = compose_and_check(stage, ens, [[(0, o, (30, 30, 30))] for o in ALL48], [ship], copy_rules=True)
    assert all(r.tolist() == (10, 10, 0, 0) for r in recs)
    assert len({g.tobytes() for g in got}) == 24  # the glider has one mirror symmetry
    done, reason, period, shift = stage.step_until_moving(64, check_every=4)
    for o in ALL48:
        assert int(reason[o]) == MOVING and int(period[o]) > 0 and int(period[o]) % 4 == 0, o
        want = tuple(v * int(period[o]) // 4 for v in host.orient_vector(o, (1, 1, 0)))
        assert tuple(int(v) for v in shift[o]) == want, o
    assert len({tuple(int(v) * 4 // int(p) for v in s) for s, p in zip(shift, period)}) == 12  # the twelve face diagonals


def test_a_collision(ens, stage):
    """The glider thrown at a 2 x 2 x 2 block, from the other side too: 64 steps on the device are the oracle's from the host.compose
    state, and not what the two would have done apart."""
    rules = moore_rules(*SHIP)
    block = host.cells_to_words(G, list(itertools.product((0, 1), repeat=3)))
    pieces = [glider("xy", (28, 30, 30)), block]
    hold(ens, pieces)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    layouts = [[(0, 0, (20, 20, 30)), (1, 0, (31, 31, 30))], [(0, 6 + 12, (40, 40, 30)), (1, 0, (31, 31, 30))]]  # f = 3: x and y mirrored
    stage.configure(2, neighbourhood="moore")
    recs, got = compose_and_check(stage, ens, layouts, pieces, copy_rules=True)
    assert all(r.tolist() == (18, 18, 0, 0) for r in recs)
    stage.step(64)
    after = stage.read_state()
    for k, layout in enumerate(layouts):
        want = ol.packed_run(G, got[k], rules, 64)
        np.testing.assert_array_equal(after[k], want, err_msg=str(k))
        apart = ol.packed_run(G, host.compose(pieces, layout[:1])[0], rules, 64) | host.compose(pieces, layout[1:])[0]
        assert not np.array_equal(want, apart), k  # they met


def test_round_trips(ens, stage):
    """An object isolated to the origin and composed elsewhere at orientation 0 has its census digest again; composed under o, and that
    composed under the inverse of o, it has it again too."""
    names = ["shapes", "shell_core"]
    states = [cc.state(n) for n in names]
    hold(ens, states)
    records, jobs = [], []
    for u, name in enumerate(names):
        comps, n, rest = cc.reference(name, 64)
        assert rest == 0
        records += list(comps[:n])
        jobs += [(u, int(c["first_cell"])) for c in comps[:n]]
    n = len(jobs)
    nursery, back = make_ensemble(), make_ensemble()
    try:
        nursery.configure(n, neighbourhood="moore")
        nursery.isolate(np.array(jobs, dtype=np.uint32), 0, ens, "origin", False)
        objects = list(nursery.read_state())
        orientations = [5 + 6 * 3, 3 + 6 * 4, 47, 2, 10][:n]
        stage.configure(2 * n, neighbourhood="moore")
        layouts = [[(k, 0, (17 + k, 3, 40 - k))] for k in range(n)] + [[(k, orientations[k], (11, 12 + k, 13))] for k in range(n)]
        compose_and_check(stage, nursery, layouts, objects)
        comps, count, rest = stage.census(max_components=8)
        turned = list(stage.read_state(n, n))
        for k in range(n):
            assert (int(count[k]), int(rest[k])) == (1, 0)
            assert int(comps[k][0]["digest"]) == int(records[k]["digest"]) and host.unpack_box(comps[k][0]["box_min"]) == (17 + k, 3, 40 - k)
            assert k >= 3 or int(comps[n + k][0]["digest"]) != int(records[k]["digest"])  # SHAPE turned is another object
        back.configure(n, neighbourhood="moore")
        compose_and_check(back, stage, [[(n + k, inverse(orientations[k]), (30, 31, 32 - k))] for k in range(n)], dict(zip(range(n, 2 * n), turned)))
        comps, count, rest = back.census(max_components=8)
        for k in range(n):
            assert (int(count[k]), int(rest[k])) == (1, 0) and int(comps[k][0]["digest"]) == int(records[k]["digest"]), k
            assert int(comps[k][0]["population"]) == int(records[k]["population"])
    finally:
        nursery.close()
        back.close()


def test_one_handle(ens):
    """Sources and destinations in disjoint ranges of one ensemble, on one stream."""
    names = ["shapes", "shell_core", "corners"]
    states = [cc.state(n) for n in names] + [cc.state("full")] * 5
    hold(ens, states)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    layouts = [[(0, 7, (1, 2, 3))], [(1, 20, (30, 30, 30)), (2, 0, (0, 0, 0))], [], [(2, 44, (-1, 0, 0)), (0, 1, (5, 5, 5)), (7, 0, (60, 0, 0))]]
    compose_and_check(ens, None, layouts, states, dst_first=3, copy_rules=True)
    got = ens.read_state()
    for u in (0, 1, 2, 7):
        np.testing.assert_array_equal(got[u], states[u])


def test_ordering(ens, stage):
    """A step queued on the source and not waited for lies in front of the compose: the piece is the stepped state."""
    first = glider("xy", (28, 30, 30))
    rules = moore_rules(*SHIP)
    hold(ens, [first])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    stepped = ol.packed_run(G, first, rules, 6)
    assert not np.array_equal(stepped, ol.packed_run(G, first, rules, 2)) and box_min(stepped) != box_min(first)
    stage.configure(2, neighbourhood="moore")
    ens.step(6)  # queued, not synchronised
    recs = stage.compose([[(0, 0, (5, 5, 5))], [(0, 25, (40, 41, 42))]], 0, ens, False, True)
    got, sums = stage.read_state(), stage.summaries()
    for k, layout in enumerate([[(0, 0, (5, 5, 5))], [(0, 25, (40, 41, 42))]]):
        words, rec = host.compose([stepped], layout)
        assert recs[k].tolist() == rec.tolist()
        np.testing.assert_array_equal(got[k], words)
        check_record(sums[k], words, k)
    np.testing.assert_array_equal(ens.read_state()[0], stepped)
    assert ens.summaries()[0].step == 6
    ens.step(4)  # the source goes on
    np.testing.assert_array_equal(ens.read_state()[0], ol.packed_run(G, stepped, rules, 4))


def test_refusals(ens, stage):
    lib = _capi.load()
    out = (_capi.ComposedStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    ms = C.c_float(-1.0)
    OVER, COPY = 0x1, 0x100

    def parts_of(*parts):
        p = (_capi.ComposePartStruct * max(len(parts), 1))()
        for k, part in enumerate(parts):
            p[k].universe, p[k].orientation = part[0], part[1]
            p[k].at[0], p[k].at[1], p[k].at[2] = part[2]
            p[k].reserved = part[3] if len(part) > 3 else 0
        return p

    def begin_of(*values):
        return (C.c_uint32 * len(values))(*values)

    watched = []  # the ensembles that hold a state everywhere: compared before and after every refusal

    def snapshot(e):
        return (e.read_state().tobytes(), e.summaries())

    def refused(code, pattern, dst, dst_first, n_dst, src, parts, begin, flags):
        before = [snapshot(e) for e in watched]
        rc = lib.ca3d_ensemble_compose(dst._h if dst else None, dst_first, n_dst, src._h if src else None, parts, begin, flags, out, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and ms.value == -1.0, msg
        assert [snapshot(e) for e in watched] == before, msg

    two = parts_of((0, 0, (0, 0, 0)), (1, 47, (-64, 64, 0)))
    b2 = begin_of(0, 1, 2)
    refused(-1, "NULL", None, 0, 2, ens, two, b2, 0)
    refused(-1, "NULL", stage, 0, 2, None, two, b2, 0)
    refused(-1, "part_begin is NULL", stage, 0, 2, ens, two, None, 0)
    refused(-2, "configure.*destination", stage, 0, 2, ens, two, b2, 0)
    stage.configure(4, neighbourhood="moore")
    refused(-2, "configure.*source", stage, 0, 2, ens, two, b2, 0)
    ens.configure(3, neighbourhood="moore")
    refused(-2, "OVER.*universe 0", stage, 0, 2, ens, two, b2, OVER)  # a destination without a state
    stage.upload_state(0, np.stack([cc.state("shapes")] * 4))
    watched.append(stage)
    refused(-1, "parts is NULL", stage, 0, 2, ens, None, b2, 0)
    refused(-2, "part 0.*universe 0", stage, 0, 2, ens, two, b2, 0)  # no state anywhere
    ens.upload_state(0, cc.state("shell_core")[None])
    refused(-2, "part 1.*universe 1", stage, 0, 2, ens, two, b2, 0)  # universe 1 has none
    ens.upload_state(1, np.stack([cc.state("corners")] * 2))
    watched.append(ens)
    refused(-1, "destinations", stage, 0, 0, ens, two, b2, 0)          # no destination
    refused(-1, "destinations", stage, 3, 2, ens, two, b2, 0)          # more than fit behind dst_first
    refused(-1, "destinations", stage, 4, 1, ens, two, b2, 0)
    refused(-1, r"part_begin\[0\]", stage, 0, 2, ens, two, begin_of(1, 1, 2), 0)
    refused(-1, "decreases", stage, 0, 2, ens, two, begin_of(0, 2, 1), 0)
    refused(-1, "1048577 parts", stage, 0, 2, ens, two, begin_of(0, 1, (1 << 20) + 1), 0)
    refused(-1, "part 1.*universe 3", stage, 0, 2, ens, parts_of((0, 0, (0, 0, 0)), (3, 0, (0, 0, 0))), b2, 0)
    refused(-1, "part 1.*orientation 48", stage, 0, 2, ens, parts_of((0, 0, (0, 0, 0)), (1, 48, (0, 0, 0))), b2, 0)
    for axis, value in itertools.product(range(3), (65, -65, 1 << 30, -(1 << 31))):
        at = [0, 0, 0]
        at[axis] = value
        refused(-1, r"part 0: at\[%d\]" % axis, stage, 0, 2, ens, parts_of((0, 0, tuple(at)), (1, 0, (0, 0, 0))), b2, 0)
    refused(-1, "part 1: reserved", stage, 0, 2, ens, parts_of((0, 0, (0, 0, 0)), (1, 0, (0, 0, 0), 7)), b2, 0)
    for flags in (0x2, 0x200, 1 << 31, OVER | COPY | 0x80):
        refused(-1, "flags", stage, 0, 2, ens, two, b2, flags)
    # one handle: a source among the destinations
    refused(-1, "part 1.*universe 1.*destinations", ens, 1, 2, ens, two, b2, 0)
    refused(-1, "part 0.*universe 2.*destinations", ens, 2, 1, ens, parts_of((2, 0, (0, 0, 0))), begin_of(0, 1), 0)
    # COPY_RULES: no rules on a first part's source, then ensembles of different kinds
    refused(-2, "part 0.*set_rules.*universe 0", stage, 0, 2, ens, two, b2, COPY)
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    refused(-2, "part 1.*set_rules.*universe 1", stage, 0, 2, ens, two, b2, COPY)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    for conf in (dict(neighbourhood="von neumann"), dict(neighbourhood="moore", clustered=True)):
        stage.configure(4, **conf)
        stage.upload_state(0, np.stack([cc.state("shapes")] * 4))
        refused(-5, "COPY_RULES", stage, 0, 2, ens, two, b2, COPY)
    # another device, where there is one
    from cellularautomatons3d_amd import Ensemble

    try:
        other = Ensemble(1)
    except Ca3dError:
        other = None
    if other is not None:
        other.configure(2, neighbourhood="moore")
        refused(-1, "device", other, 0, 2, ens, two, b2, 0)
        other.close()
    # the Python face
    with pytest.raises(Ca3dError) as e:
        stage.compose([], 0, ens)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        stage.compose([[(0, 0, (0, 0))]], 0, ens)
    # and the calls that are not refused: out and gpu_ms may be NULL, parts may be NULL where there are none; without the flag the
    # kinds may differ (the stage is clustered)
    assert lib.ca3d_ensemble_compose(stage._h, 2, 2, ens._h, two, b2, 0, None, None) == 0
    assert bytes(out) == b"\x5a" * C.sizeof(out)
    assert lib.ca3d_ensemble_compose(stage._h, 0, 2, ens._h, None, begin_of(0, 0, 0), 0, out, C.byref(ms)) == 0
    assert ms.value > 0.0 and bytes(out)[:32] == bytes(32) and not stage.read_state(0, 2).any()
    got = stage.read_state(2, 2)
    np.testing.assert_array_equal(got[0], host.compose([cc.state("shell_core")], [(0, 0, (0, 0, 0))])[0])
    np.testing.assert_array_equal(got[1], host.compose([None, cc.state("corners")], [(1, 47, (-64, 64, 0))])[0])
