"""`ca3d_ensemble_isolate` on the GPU (kernel ca_ensemble_isolate64, csrc/ca_isolate.hip) against `host.isolate`, the numpy restatement
of the definition in include/ca3d.h, with jobs taken from `host.census` and records from `host.state_summary` — never from the engine.
Every comparison is exact: the destination's states, the populations and shifts, the destination's records (step 0, population, box,
digest, no previous state) and the untouched source, states and records. The crafted states are tests/census_cases.py's;
tests/test_isolate_cpu.py checks `host.isolate` itself."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import census_cases as cc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_census import KEYS
from test_gpu_moving import MOVING, SHIP, STILL, Trajectory, expected, glider, moore_rules

pytestmark = pytest.mark.gpu

G, W = 64, 8192
PLACEMENTS = ("keep", "centre", "origin")
CRAFTED = ["shapes", "shell_core", "corners", "staircase", "serpentine", "full", "empty"] + [n for n in cc.CRAFTED if n.startswith("pairs1_")]

_ISOLATED = {}


def isolated(key, words, cell, placement):
    """`host.isolate(words, cell, placement)`, kept under `key` (which names `words`) for the run and never changed."""
    k = (key, int(cell), placement)
    if k not in _ISOLATED:
        w, pop, shift = host.isolate(words, int(cell), placement)
        w.setflags(write=False)
        _ISOLATED[k] = (w, pop, shift)
    return _ISOLATED[k]


def cell_of(x, y, z):
    return x + 64 * y + 4096 * z


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


@pytest.fixture()
def nursery():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def hold(e, states, nb="moore", clustered=False):
    e.configure(len(states), neighbourhood=nb, clustered=clustered)
    e.upload_state(0, np.stack(states))


def check_record(s, words, where):
    """A destination's record: what an upload of `words` leaves (step 0, no previous state)."""
    want = host.state_summary(G, words)
    assert s.step == 0 and not s.has_previous and (s.births, s.deaths) == (0, 0), where
    assert s.population == want["population"] and s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


def isolate_and_check(dst, src, jobs, keys, states, placement, dst_first=0, copy_rules=False):
    """One call; job k = (universe, cell) against isolated(keys[universe], states[universe], cell, placement). `src` None: one handle."""
    source = dst if src is None else src
    sources = sorted({u for u, _ in jobs})
    before = [(source.read_state(u, 1).tobytes(), source.summaries(u, 1)) for u in sources]
    pop, shift = dst.isolate(np.array(jobs, dtype=np.uint32).reshape(-1, 2), dst_first, src, placement, copy_rules)
    n = len(jobs)
    assert pop.shape == (n,) and pop.dtype == np.uint32 and shift.shape == (n, 3) and shift.dtype == np.int32
    got, recs = dst.read_state(dst_first, n), dst.summaries(dst_first, n)
    for k, (u, cell) in enumerate(jobs):
        where = f"job {k}: universe {u} ({keys[u]}), cell {cell}, {placement}"
        words, want_pop, want_shift = isolated(keys[u], states[u], cell, placement)
        assert (int(pop[k]), tuple(int(v) for v in shift[k])) == (want_pop, want_shift), where
        np.testing.assert_array_equal(got[k], words, err_msg=where)
        check_record(recs[k], words, where)
    assert [(source.read_state(u, 1).tobytes(), source.summaries(u, 1)) for u in sources] == before  # the source is only read
    return pop, shift


def census_jobs(names):
    """Every component of every named state, as jobs on universe = index in `names`; the lists are complete on the reference's side."""
    jobs = []
    for u, name in enumerate(names):
        comps, n, rest = cc.reference(name, 64)
        assert rest == 0 and n == cc.CRAFTED[name][1], name
        jobs += [(u, int(c["first_cell"])) for c in comps[:n]]
    return jobs


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_crafted_states(ens, nursery, placement):
    """Every component of shapes, shell and core (overlapping boxes), the eight corners, the staircase through all 16 waves (dz = 0), the
    2 079-cell serpentine, the full universe (shift 0 whatever the placement), all 13 directions across word, lane and wave seams — and
    a dead cell of the empty universe."""
    states = [cc.state(n) for n in CRAFTED]
    hold(ens, states)
    jobs = census_jobs(CRAFTED) + [(CRAFTED.index("empty"), 0)]
    assert len(jobs) == 3 + 2 + 8 + 1 + 1 + 1 + 13 * 4 + 1
    nursery.configure(len(jobs), neighbourhood="von neumann")  # without COPY_RULES the two may differ in kind
    pop, shift = isolate_and_check(nursery, ens, jobs, CRAFTED, states, placement)
    full = jobs.index((CRAFTED.index("full"), 0))
    assert int(pop[full]) == G ** 3 and not shift[full].any()
    assert int(pop[-1]) == 0 and not shift[-1].any() and not nursery.read_state(len(jobs) - 1, 1).any()
    stair = [k for k, (u, _) in enumerate(jobs) if CRAFTED[u] == "staircase"][0]
    assert int(pop[stair]) == 129 and (placement == "keep" or int(shift[stair][2]) == 0)
    assert nursery.isolate_gpu_ms() > 0.0


def test_shifts_at_their_ends(ens, nursery):
    """Single cells at (0, 0, 0) and (63, 63, 63) centred (+31 and -32 on every axis: the largest shifts CENTRE knows); SHAPE at
    (50, 9, 57) to the origin (dx = -50 across the word seam, dz = -57 across 14 waves); a full 64-cell row moved in y and z; SHAPE
    placed so that dx = -1, -31, -32, -33 (ORIGIN) and +1, -1, +29 (CENTRE), and a shape of two cells along x at x = 0, 1 so that
    dx = +31 and +30. (No placement shifts by more than +31: (64 - e) / 2 - min is largest for one cell at 0.)"""
    row = [(x, 5, 50) for x in range(G)]
    thin = lambda x0: [(x0, 20, 20), (x0 + 1, 20, 20), (x0, 21, 21)]
    made = {
        "cell_0": [(0, 0, 0)], "cell_63": [(63, 63, 63)], "row": row,
        **{"shape_x%d" % x0: cc.shape_at((x0, 9, 57)) for x0 in (50, 1, 31, 32, 33, 28, 30, 0, 58)},
        "thin_0": thin(0), "thin_1": thin(1), "thin_62": thin(62),
    }
    keys = list(made)
    states = [cc.words(made[k]) for k in keys]
    hold(ens, states)
    jobs = [(u, cell_of(*made[k][0])) for u, k in enumerate(keys)]
    nursery.configure(len(jobs), neighbourhood="moore")
    _, shift = isolate_and_check(nursery, ens, jobs, keys, states, "centre")
    by = {k: tuple(int(v) for v in shift[u]) for u, k in enumerate(keys)}
    assert by["cell_0"] == (31, 31, 31) and by["cell_63"] == (-32, -32, -32)
    assert by["row"] == (0, 26, -19)
    assert [by["shape_x%d" % x][0] for x in (28, 30, 0, 58)] == [1, -1, 29, -29]
    assert (by["thin_0"][0], by["thin_1"][0], by["thin_62"][0]) == (31, 30, -31)
    _, shift = isolate_and_check(nursery, ens, jobs, keys, states, "origin")
    by = {k: tuple(int(v) for v in shift[u]) for u, k in enumerate(keys)}
    assert by["shape_x50"] == (-50, -9, -57) and by["row"] == (0, -5, -50) and by["cell_63"] == (-63, -63, -63)
    assert [by["shape_x%d" % x][0] for x in (1, 31, 32, 33)] == [-1, -31, -32, -33]
    digest = host.state_summary(G, host.cells_to_words(G, cc.SHAPE))["digest"]
    assert all(s.digest == digest for u, s in enumerate(nursery.summaries()) if keys[u].startswith("shape_x"))


def test_selection(ens, nursery):
    """A component's last cell and a cell in its middle select what its first cell selects; a dead cell — inside a box, and in an empty
    universe — selects nothing; one source universe serves many jobs."""
    names = ["shapes", "shell_core", "empty", "staircase"]
    states = [cc.state(n) for n in names]
    hold(ens, states)
    jobs = []
    for u, name in enumerate(names):
        for c in cc.reference(name, 64)[0][: cc.CRAFTED[name][1]]:
            keep = host.isolate(states[u], int(c["first_cell"]), "keep")[0]
            cells = np.flatnonzero(np.unpackbits(keep.view(np.uint8), bitorder="little"))
            picks = [int(cells[0]), int(cells[-1]), int(cells[len(cells) // 2])]
            assert picks[0] == int(c["first_cell"])
            jobs += [(u, p) for p in picks]
    dead = [(0, cell_of(3, 2, 2)), (1, cell_of(29, 14, 4)), (2, 12345), (0, 0), (0, (1 << 18) - 1)]  # inside SHAPE's box; between shell and core
    jobs += dead
    jobs += [(0, jobs[0][1])] * 5  # the same job again and again
    nursery.configure(len(jobs), neighbourhood="moore")
    for placement in ("centre", "keep"):
        pop, shift = isolate_and_check(nursery, ens, jobs, names, states, placement)
        got = nursery.read_state()
        for k in range(0, len(jobs) - len(dead) - 5, 3):
            assert got[k].tobytes() == got[k + 1].tobytes() == got[k + 2].tobytes() and int(pop[k]) > 0
        first_dead = len(jobs) - len(dead) - 5
        assert not pop[first_dead:first_dead + len(dead)].any() and not shift[first_dead:first_dead + len(dead)].any()
        assert not got[first_dead:first_dead + len(dead)].any()


def glider_and_block():
    block = [(10 + i, 10 + j, 40 + k) for i, j, k in itertools.product((0, 1), repeat=3)]
    return glider("xy", (28, 30, 30)) | host.cells_to_words(G, block)


def test_a_glider_beside_a_block_told_apart(ens, nursery):
    """The point of it: tests/test_gpu_census.py's universe, where step_until_moving is silent. One census, two jobs, CENTRE with the
    source's rule — and step_until_moving on the nursery names the ship (MOVING, shift (1, 1, 0)) and the still life."""
    first = glider_and_block()
    rules = moore_rules(*SHIP)
    hold(ens, [first])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    comps, n, rest = ens.census(max_components=8)
    want_comps = cc.reference_of(("glider+block", 0), first, 8)
    assert (int(n[0]), int(rest[0])) == (2, 0) == want_comps[1:] and comps[0].tobytes() == want_comps[0].tobytes()
    jobs = [(0, int(c["first_cell"])) for c in want_comps[0][:2]]
    nursery.configure(2, neighbourhood="moore")
    pop, shift = isolate_and_check(nursery, ens, jobs, ["glider+block"], [first], "centre", copy_rules=True)
    assert [int(p) for p in pop] == [10, 8] and tuple(int(v) for v in shift[0]) == (2, 0, 1)
    done, reason, period, moved = nursery.step_until_moving(64, check_every=4)
    for k, (u, cell) in enumerate(jobs):
        t = Trajectory(isolated("glider+block", first, cell, "centre")[0], rules)
        want = expected(t, 0, 64, 4, 15, False)
        assert (int(done[k]), int(reason[k]), int(period[k]), tuple(int(v) for v in moved[k])) == want, k
        np.testing.assert_array_equal(nursery.read_state(k, 1)[0], t[want[0]])
    assert (int(reason[0]), int(period[0]), tuple(int(v) for v in moved[0])) == (MOVING, 4, (1, 1, 0))
    assert int(reason[1]) & STILL and not int(reason[1]) & MOVING and int(done[1]) == 4
    # the source is still silent
    done, reason, period, moved = ens.step_until_moving(64)
    assert not int(reason[0]) & MOVING and int(period[0]) == 0 and int(done[0]) == 64


def test_a_glider_born_in_a_corner(ens, nursery):
    """A glider at (60, 60, 30) leaves the inside of the cube before the first check point: followed in place it is not reported, by
    the definition on the oracle trajectory. Centred it is."""
    first = glider("xy", (60, 60, 30))
    rules = moore_rules(*SHIP)
    in_place = expected(Trajectory(first, rules), 0, 64, 8, 15, False)
    assert not in_place[1] & MOVING
    hold(ens, [first])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    comps, n, rest = host.census(first, 8)
    assert (n, rest) == (1, 0)
    nursery.configure(1, neighbourhood="moore")
    pop, shift = isolate_and_check(nursery, ens, [(0, int(comps[0]["first_cell"]))], ["corner glider"], [first], "centre", copy_rules=True)
    assert tuple(int(v) for v in shift[0]) == (-30, -30, 1)
    centred = expected(Trajectory(isolated("corner glider", first, int(comps[0]["first_cell"]), "centre")[0], rules), 0, 64, 8, 15, False)
    assert centred[1] == MOVING and centred[3] == (2, 2, 0)
    done, reason, period, moved = nursery.step_until_moving(64)
    assert (int(done[0]), int(reason[0]), int(period[0]), tuple(int(v) for v in moved[0])) == centred
    done, reason, period, moved = ens.step_until_moving(64)
    assert (int(done[0]), int(reason[0]), int(period[0]), tuple(int(v) for v in moved[0])) == in_place


KINDS = {
    # kind -> (configure arguments, two rules as set_rule_strings arguments)
    "moore": (dict(neighbourhood="moore"), [dict(born="6", survive="5-7"), dict(born="5", survive="4,5")]),
    "clustered": (dict(neighbourhood="moore", clustered=True),
                  [dict(zip(KEYS, ("6", "5-7", "27", "27", "", "1-8"))), dict(zip(KEYS, ("5", "4,5", "3", "27", "27", "2")))]),
    "von neumann": (dict(neighbourhood="von neumann"), [dict(born="3", survive="2,3"), dict(born="2,4", survive="1,3,5")]),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_rules_follow_the_source(ens, nursery, kind):
    """2, 6 and 1 rule words a universe: source universes alternate between two rules, the nursery takes them in another order, and
    after four steps every nursery universe is the oracle's under ITS source's rule."""
    conf, two = KINDS[kind]
    nb = conf["neighbourhood"]
    B = 4
    states = [host.random_fill(W, seed=11 + u, and_rounds=1) for u in range(B)]
    ens.configure(B, **conf)
    ens.upload_state(0, np.stack(states))
    for u in range(B):
        ens.set_rule_strings(u, neighbourhood=nb, **two[u % 2])
    keys = [("soup", u) for u in range(B)]
    jobs = []
    for u in (3, 0, 1, 2, 1):
        i = int(np.flatnonzero(states[u])[0])
        w = int(states[u][i])
        jobs.append((u, 32 * i + (w & -w).bit_length() - 1))  # the soup's first live cell
    nursery.configure(len(jobs), **conf)
    pop, _ = isolate_and_check(nursery, ens, jobs, keys, states, "centre", copy_rules=True)
    assert int(pop.min()) > 100  # the soup's giant object
    nursery.step(4)
    got = nursery.read_state()
    differ = 0
    for k, (u, cell) in enumerate(jobs):
        start = isolated(keys[u], states[u], cell, "centre")[0]
        want = ol.packed_run(G, start, ol.Rules.from_strings(neighbourhood=nb, **two[u % 2]), 4)
        np.testing.assert_array_equal(got[k], want, err_msg=f"job {k} under rule {two[u % 2]}")
        differ += not np.array_equal(want, ol.packed_run(G, start, ol.Rules.from_strings(neighbourhood=nb, **two[1 - u % 2]), 4))
    assert differ  # the two rules tell the universes apart: a nursery that took the wrong one would show
    assert [s.step for s in nursery.summaries()] == [4] * len(jobs)


def test_without_copy_rules_the_nursery_keeps_its_own(ens, nursery):
    first = glider_and_block()
    hold(ens, [first])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    jobs = [(0, cell_of(10, 10, 40)), (0, int(host.census(first, 8)[0]["first_cell"][0]))]
    own = dict(born="5", survive="4,5")
    nursery.configure(2, neighbourhood="moore")
    nursery.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", **own)
    isolate_and_check(nursery, ens, jobs, ["glider+block"], [first], "centre", copy_rules=False)
    nursery.step(4)
    got = nursery.read_state()
    for k, (u, cell) in enumerate(jobs):
        start = isolated("glider+block", first, cell, "centre")[0]
        np.testing.assert_array_equal(got[k], ol.packed_run(G, start, moore_rules(own["born"], own["survive"]), 4))
        assert not np.array_equal(got[k], ol.packed_run(G, start, moore_rules(*SHIP), 4))
    # a nursery without rules has none afterwards either: it has states now, and still refuses to step
    nursery.configure(2, neighbourhood="moore")
    isolate_and_check(nursery, ens, jobs, ["glider+block"], [first], "centre", copy_rules=False)
    with pytest.raises(Ca3dError) as e:
        nursery.step(1)
    assert e.value.code == -2 and "set_rules" in str(e.value)
    # ... and with the flag, for one of two universes, one is still missing
    nursery.isolate(np.array(jobs[:1], dtype=np.uint32), 1, ens, "centre", True)
    with pytest.raises(Ca3dError) as e:
        nursery.step(1)
    assert e.value.code == -2 and "1 of 2" in str(e.value)
    nursery.isolate(np.array(jobs[:1], dtype=np.uint32), 0, ens, "centre", True)
    nursery.step(1)
    nursery.synchronize()


def test_ash(ens, nursery):
    """Moore B6/S5-7 ash of eight soups: every object of all eight in ONE call, at the origin — the nursery's records carry the census
    records' digests and populations."""
    ens.configure(8, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="6", survive="5-7")
    ens.seed_states(0, np.arange(101, 109), 1)
    ens.step_until_cycle(512)
    states = ens.read_state()
    comps, n, rest = ens.census(max_components=1024)
    jobs, records = [], []
    for u in range(8):
        want = cc.reference_of(("ash", 101 + u), states[u], 1024)
        assert want[2] == 0, u  # complete on the reference's side
        assert (int(n[u]), int(rest[u])) == want[1:] and comps[u].tobytes() == want[0].tobytes(), u
        jobs += [(u, int(c["first_cell"])) for c in want[0][: want[1]]]
        records += list(want[0][: want[1]])
    assert len(jobs) > 8
    nursery.configure(len(jobs), neighbourhood="moore")
    keys = [("ash", 101 + u) for u in range(8)]
    pop, shift = isolate_and_check(nursery, ens, jobs, keys, list(states), "origin", copy_rules=True)
    for k, (s, c) in enumerate(zip(nursery.summaries(), records)):
        assert (s.digest, s.population) == (int(c["digest"]), int(c["population"])) and int(pop[k]) == int(c["population"]), k
        assert tuple(-int(v) for v in shift[k]) == host.unpack_box(c["box_min"]) and s.box_min == (0, 0, 0), k


def test_one_handle(ens):
    """Sources and destinations in one ensemble, on one stream."""
    names = ["shapes", "shell_core", "corners"]
    states = [cc.state(n) for n in names] + [cc.state("full")] * 5
    hold(ens, states)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    jobs = [(0, int(c["first_cell"])) for c in cc.reference("shapes", 64)[0][:3]] + [(1, cell_of(31, 16, 7)), (2, cell_of(63, 0, 63))]
    isolate_and_check(ens, None, jobs, names, states, "centre", dst_first=3, copy_rules=True)
    got = ens.read_state()
    for u in range(3):
        np.testing.assert_array_equal(got[u], states[u])


def test_scale_and_a_range(ens, nursery):
    """300 jobs, more than compute units, into universes 7 .. 306 of 310: the ten universes around the range keep what they held."""
    names = [n for n in CRAFTED if n not in ("serpentine", "full", "empty")]
    states = [cc.state(n) for n in names]
    hold(ens, states)
    every = census_jobs(names)
    jobs = [every[k % len(every)] for k in range(300)]
    marker = host.random_fill(W, seed=5, and_rounds=3)
    nursery.configure(310, neighbourhood="moore")
    nursery.upload_state(0, np.stack([marker] * 7))
    nursery.upload_state(307, np.stack([marker] * 3))
    isolate_and_check(nursery, ens, jobs, names, states, "centre", dst_first=7)
    for u in (0, 6, 307, 309):
        np.testing.assert_array_equal(nursery.read_state(u, 1)[0], marker)
        check_record(nursery.summaries(u, 1)[0], marker, u)
    # a smaller call afterwards reuses the staging array
    isolate_and_check(nursery, ens, jobs[:5], names, states, "origin", dst_first=100)
    np.testing.assert_array_equal(nursery.read_state(105, 1)[0], isolated(names[jobs[98][0]], states[jobs[98][0]], jobs[98][1], "centre")[0])


def test_ordering(ens, nursery):
    """A step queued on the source and not waited for lies in front of the isolate; a step queued on the nursery does not survive it."""
    first = glider_and_block()
    rules = moore_rules(*SHIP)
    hold(ens, [first])
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    stepped = ol.packed_run(G, first, rules, 4)
    comps, n, rest = host.census(stepped, 8)
    assert (n, rest) == (2, 0) and host.unpack_box(comps[0]["box_min"]) == (29, 31, 30)  # the ship has moved
    jobs = [(0, int(c["first_cell"])) for c in comps[:2]]
    hold(nursery, [cc.state("shell_core")] * 2)
    nursery.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="5", survive="4,5")
    nursery.step(3)  # queued, not synchronised
    ens.step(4)      # queued, not synchronised
    pop, shift = nursery.isolate(np.array(jobs, dtype=np.uint32), 0, ens, "centre", True)
    got, recs = nursery.read_state(), nursery.summaries()
    for k, (u, cell) in enumerate(jobs):
        words, want_pop, want_shift = isolated("glider+block after 4", stepped, cell, "centre")
        np.testing.assert_array_equal(got[k], words)
        assert (int(pop[k]), tuple(int(v) for v in shift[k])) == (want_pop, want_shift)
        check_record(recs[k], words, k)
    np.testing.assert_array_equal(ens.read_state()[0], stepped)
    assert ens.summaries()[0].step == 4
    ens.step(4)  # the source goes on
    np.testing.assert_array_equal(ens.read_state()[0], ol.packed_run(G, stepped, rules, 4))


def test_refusals(ens, nursery):
    from cellularautomatons3d_amd import Ensemble

    lib = _capi.load()
    out = (_capi.IsolatedStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    ms = C.c_float(-1.0)
    KEEP, CENTRE, ORIGIN, COPY = 0, 1, 2, 0x100

    def jobs_of(*pairs):
        j = (_capi.IsolateJobStruct * max(len(pairs), 1))()
        for k, (u, c) in enumerate(pairs):
            j[k].universe, j[k].cell = u, c
        return j

    watched = []  # the ensembles that hold a state everywhere: compared before and after every refusal

    def snapshot(e):
        return (e.read_state().tobytes(), e.summaries())

    def refused(code, pattern, dst, dst_first, src, n_jobs, jobs, flags):
        before = [snapshot(e) for e in watched]
        rc = lib.ca3d_ensemble_isolate(dst._h if dst else None, dst_first, src._h if src else None, n_jobs, jobs, flags, out, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and ms.value == -1.0, msg
        assert [snapshot(e) for e in watched] == before, msg

    two = jobs_of((0, 0), (1, 5))
    refused(-1, "NULL", None, 0, ens, 2, two, CENTRE)
    refused(-1, "NULL", nursery, 0, None, 2, two, CENTRE)
    refused(-2, "configure.*destination", nursery, 0, ens, 2, two, CENTRE)
    nursery.configure(4, neighbourhood="moore")
    refused(-2, "configure.*source", nursery, 0, ens, 2, two, CENTRE)
    ens.configure(3, neighbourhood="moore")
    nursery.upload_state(0, np.stack([cc.state("shapes")] * 4))
    watched.append(nursery)
    refused(-1, "NULL", nursery, 0, ens, 2, None, CENTRE)
    refused(-2, "job 0.*universe 0", nursery, 0, ens, 2, two, CENTRE)  # no state anywhere
    ens.upload_state(0, cc.state("shell_core")[None])
    refused(-2, "job 1.*universe 1", nursery, 0, ens, 2, two, CENTRE)  # universe 1 has none
    ens.upload_state(1, np.stack([cc.state("corners")] * 2))
    watched.append(ens)
    refused(-1, "jobs", nursery, 0, ens, 0, two, CENTRE)               # no job
    refused(-1, "jobs", nursery, 3, ens, 2, two, CENTRE)               # more than fit behind dst_first
    refused(-1, "jobs", nursery, 4, ens, 1, two, CENTRE)
    refused(-1, "job 1.*universe 3", nursery, 0, ens, 2, jobs_of((0, 0), (3, 0)), CENTRE)
    refused(-1, "job 1.*cell 262144", nursery, 0, ens, 2, jobs_of((0, 0), (1, 1 << 18)), CENTRE)
    refused(-1, "placement 3", nursery, 0, ens, 2, two, 3)
    refused(-1, "flags", nursery, 0, ens, 2, two, CENTRE | 0x200)
    refused(-1, "flags", nursery, 0, ens, 2, two, ORIGIN | 1 << 31)
    # one handle: a source among the destinations
    refused(-1, "job 1.*universe 1.*destinations", ens, 1, ens, 2, two, KEEP)
    refused(-1, "job 0.*universe 2.*destinations", ens, 2, ens, 1, jobs_of((2, 0)), KEEP)
    # COPY_RULES: no rules on the source, then ensembles of different kinds
    refused(-2, "job 0.*set_rules.*universe 0", nursery, 0, ens, 2, two, CENTRE | COPY)
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    refused(-2, "job 1.*set_rules.*universe 1", nursery, 0, ens, 2, two, CENTRE | COPY)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    for conf in (dict(neighbourhood="von neumann"), dict(neighbourhood="moore", clustered=True)):
        nursery.configure(4, **conf)
        nursery.upload_state(0, np.stack([cc.state("shapes")] * 4))
        refused(-5, "COPY_RULES", nursery, 0, ens, 2, two, CENTRE | COPY)
    # another device, where there is one
    try:
        other = Ensemble(1)
    except Ca3dError:
        other = None
    if other is not None:
        other.configure(2, neighbourhood="moore")
        refused(-1, "device", other, 0, ens, 2, two, CENTRE)
        other.close()
    # the Python face
    with pytest.raises(ValueError):
        nursery.isolate([(0, 0)], placement="middle")
    with pytest.raises(ValueError):
        nursery.isolate([0, 0, 0])
    with pytest.raises(Ca3dError) as e:
        nursery.isolate(np.zeros((0, 2), dtype=np.uint32), 0, ens)
    assert e.value.code == -1
    # and the calls that are not refused: out and gpu_ms may be NULL; without the flag the kinds may differ (the nursery is clustered)
    good = jobs_of((0, cell_of(35, 20, 10)), (1, 5))  # the shell's last cell; a dead cell of `corners`
    assert lib.ca3d_ensemble_isolate(nursery._h, 2, ens._h, 2, good, CENTRE, None, None) == 0
    assert bytes(out) == b"\x5a" * C.sizeof(out)
    assert lib.ca3d_ensemble_isolate(nursery._h, 0, ens._h, 2, good, ORIGIN, out, C.byref(ms)) == 0
    assert ms.value > 0.0
    shell = host.isolate(cc.state("shell_core"), cell_of(35, 20, 10), "origin")
    assert (out[0].population, tuple(out[0].shift)) == (shell[1], shell[2]) == (386, (-27, -12, -2))
    assert (out[1].population, tuple(out[1].shift)) == (0, (0, 0, 0)) == host.isolate(cc.state("corners"), 5, "origin")[1:]
    got = nursery.read_state()
    np.testing.assert_array_equal(got[0], shell[0])
    np.testing.assert_array_equal(got[2], host.isolate(cc.state("shell_core"), cell_of(35, 20, 10), "centre")[0])
    assert not got[1].any() and not got[3].any()
