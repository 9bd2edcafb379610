"""CA3D_STOP_MOVING on the GPU: ca3d_ensemble_step_until_moving, decided inside ca_ensemble_vn64_moving / ca_ensemble_moore64_moving /
ca_ensemble_clustered64_moving for every universe on its own. Expected values always come from CPU-oracle trajectories
(oracle_lib.packed_step) fed to `expected` below — the definition in include/ca3d.h restated on [z, y, x] bit arrays, translation being
np.roll after the inside test — never from the engine. Every comparison is exact.

The ship is Moore B6/S5-7's doubled Conway glider: the five cells (0,1), (1,2), (2,0), (2,1), (2,2) of a plane, copied into the adjacent
layer; 10 cells, period 4, one cell along each of the plane's two axes per period."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host

pytestmark = pytest.mark.gpu

G, W = 64, 8192
EXTINCT, STILL, PERIODIC, MOVING = 1, 2, 4, 8
SHIP = ("6", "5-7")
GLIDER = ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2))
AXES = {"xy": (0, 1, 2), "xz": (0, 2, 1), "yz": (1, 2, 0)}  # the plane's two axes, the axis the two layers lie along
# (born, survive, seed, and_rounds) of host.random_fill: tests/test_gpu_cycle.py's lists
VN = [("2,4", "1,3,5", 3, 5), ("3", "2,3", 1, 0), ("3", "2,3", 2, 2), ("2", "1-3", 3, 5), ("0", "", 1, 0), ("2", "0", 3, 5), ("2,3", "1", 3, 5),
      ("3,4", "0-2", 2, 2), ("1", "", 1, 0), ("1,3", "0-6", 1, 0), ("5,6", "4-6", 1, 0)]
MOORE = [("5", "4,5", 2, 2), ("5", "5", 2, 2), ("6", "5-7", 1, 0), ("6-8", "5-8", 3, 4), ("3", "2,3", 1, 0), ("5", "4,5", 1, 0), ("5", "5", 1, 0)]
OSCILLATOR = ("6", "5-7", 1, 0)


def glider(plane, corner, flip=(False, False)):
    """The doubled glider as packed words: `plane` names its two axes, `corner` is the lower (x, y, z) corner of its 3 x 3 x 2 box, `flip`
    mirrors it along the plane's first / second axis (unflipped it moves towards + on both)."""
    a, b, n = AXES[plane]
    cells = []
    for (p, q) in GLIDER:
        for layer in (0, 1):
            c = list(corner)
            c[a] += 2 - p if flip[0] else p
            c[b] += 2 - q if flip[1] else q
            c[n] += layer
            cells.append(tuple(c))
    return host.cells_to_words(G, cells)


BOTH = (True, True)
# a: crosses the word boundary x = 31 | 32; b: moves -x -z, crosses a wave's plane boundary at check_every 3; c: +y -z; d: reaches the +
# faces; e: reaches the - faces
SHIPS = {"a": ("xy", (28, 30, 30), (False, False)), "b": ("xz", (33, 20, 17), BOTH), "c": ("yz", (10, 5, 40), (False, True)),
         "d": ("xy", (58, 58, 30), (False, False)), "e": ("xz", (2, 20, 2), BOTH),
         # f: -y +z, so that the module's first test sees both signs on every axis (a - e leave -y and +z out)
         "f": ("yz", (40, 30, 12), (True, False))}


class Trajectory:
    """Oracle states of one universe, computed on demand and kept for the module; with each state its unpacked cells' population and
    bounding box (what the definition below asks for at every check point)."""

    def __init__(self, first, rules):
        self.t, self.rules, self.meta = [np.ascontiguousarray(first, dtype=np.uint32)], rules, {}

    def __getitem__(self, k):
        while len(self.t) <= k:
            self.t.append(ol.packed_step(G, self.t[-1], self.rules))
        return self.t[k]

    def cells(self, k):
        return np.unpackbits(self[k].astype("<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]

    def box(self, k):
        """(population, box_min (x, y, z), box_max) of state k; the empty state: (0, None, None)."""
        if k not in self.meta:
            c = self.cells(k)
            pop = int(c.sum())
            if pop == 0:
                self.meta[k] = (0, None, None)
            else:
                idx = [np.flatnonzero(c.any(axis=ax)) for ax in ((0, 1), (0, 2), (1, 2))]  # x, y, z
                self.meta[k] = (pop, tuple(int(i[0]) for i in idx), tuple(int(i[-1]) for i in idx))
        return self.meta[k]


_TRAJ = {}


def traj(key, first=None, rules=None):
    if key not in _TRAJ:
        _TRAJ[key] = Trajectory(first() if callable(first) else first, rules)
    return _TRAJ[key]


def moore_rules(born, survive):
    return ol.Rules.from_strings(neighbourhood="moore", born=born, survive=survive)


def ship(name):
    return traj(("ship", name), lambda: glider(*SHIPS[name]), moore_rules(*SHIP))


def filled(nb, case):
    b, s, seed, rounds = case
    return traj((nb, case), lambda: host.random_fill(W, seed=seed, and_rounds=rounds), ol.Rules.from_strings(neighbourhood=nb, born=b, survive=s))


def empty():
    return traj("empty", np.zeros(W, dtype=np.uint32), moore_rules(*SHIP))


def inside(mn, mx):
    return mn is not None and min(mn) >= 1 and max(mx) <= G - 2


def moved(t, anchor, k, stats):
    """The displacement d when state k of `t` is state `anchor` translated by d != 0, both non-empty and strictly inside; else None.
    stats["filter"] counts the times populations, box extents, both inside tests and d != 0 left the comparison to decide,
    stats["failed"] the times it then said no."""
    (pa, amin, amax), (pc, cmin, cmax) = t.box(anchor), t.box(k)
    if not (pa and pc and inside(amin, amax) and inside(cmin, cmax)):
        return None
    d = tuple(c - a for a, c in zip(amin, cmin))
    if d == (0, 0, 0):
        return None
    same = np.array_equal(t.cells(k), np.roll(t.cells(anchor), shift=(d[2], d[1], d[0]), axis=(0, 1, 2)))
    if pa == pc and tuple(c - a for a, c in zip(amax, cmax)) == d:
        stats["filter"] += 1
        stats["failed"] += not same
    return d if same else None


def expected(t, start, max_steps, every, mask, has_prev, stats=None):
    """(steps_done, reason, period, shift) of a step_until_moving that begins at state t[start]: the definition of include/ca3d.h."""
    stats = {"filter": 0, "failed": 0} if stats is None else stats
    k = j = anchor = 0
    while True:
        cur = t[start + k]
        fired, d = 0, None
        if not cur.any():
            fired |= EXTINCT
        if (has_prev or k > 0) and np.array_equal(cur, t[start + k - 1]):
            fired |= STILL
        if j > 0 and np.array_equal(cur, t[start + anchor]):
            fired |= PERIODIC
        if j > 0:
            d = moved(t, start + anchor, start + k, stats)
            if d is not None:
                fired |= MOVING
        fired &= mask
        if fired or k == max_steps:
            return k, fired, (k - anchor if fired & (PERIODIC | MOVING) else 0), (d if fired & MOVING else (0, 0, 0))
        if j > 0 and j & (j - 1) == 0:  # j = 1, 2, 4, 8, ...: the anchor moves AFTER the comparison
            anchor = k
        k += min(every, max_steps - k)
        j += 1


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def make(ens, trajs, rules, clustered=False, nb="moore"):
    """An ensemble holding state 0 of every trajectory; rules: (born, survive) per universe, or six strings in a clustered one."""
    ens.configure(len(trajs), neighbourhood=nb, clustered=clustered)
    keys = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")
    for k, r in enumerate(rules):
        ens.set_rule_strings(k, neighbourhood=nb, **dict(zip(keys, r)))
    ens.upload_state(0, np.stack([t[0] for t in trajs]))


def quads(done, reason, period, shift):
    return [(int(d), int(r), int(p), tuple(int(v) for v in s)) for d, r, p, s in zip(done, reason, period, shift)]


def check_record(s, want, step, where):
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


def check_states(ens, trajs, got, offsets=None):
    """States and records after a call against the oracle's at steps_done (offsets: the steps earlier calls took)."""
    state, recs = ens.read_state(), ens.summaries()
    for k, t in enumerate(trajs):
        d = got[k][0] + (offsets[k] if offsets else 0)
        np.testing.assert_array_equal(state[k], t[d], err_msg=f"universe {k}: state after {d} steps")
        check_record(recs[k], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, f"universe {k}")


# what the issue states for the ships that stay inside (a, b, c and f), by check_every: (steps_done, reason, period, |shift| per moving axis)
STATED = {1: (8, MOVING, 4, 1), 2: (8, MOVING, 4, 1), 4: (4, MOVING, 4, 1), 3: (24, MOVING, 12, 3), 5: (40, MOVING, 20, 5)}
# ... for d (reaches the + faces) and e (the - faces): MOVING where it says so, else STILL at the step given
STATED_D = {1: MOVING, 2: MOVING, 4: MOVING, 3: (18, STILL), 5: (20, STILL)}
STATED_E = {4: MOVING, 1: (12, STILL), 2: (12, STILL), 3: (12, STILL), 5: (15, STILL)}
EVERY = [1, 2, 3, 4, 5]
_WANT = {}


def first_test(every):
    """(trajectories, rules, expectations, filter statistics per universe) of the first test at one check_every, from the oracle alone."""
    if every not in _WANT:
        trajs = [ship(n) for n in SHIPS] + [filled("moore", OSCILLATOR), empty()]
        stats = [{"filter": 0, "failed": 0} for _ in trajs]
        _WANT[every] = (trajs, [SHIP] * len(SHIPS) + [OSCILLATOR[:2], SHIP], [expected(t, 0, 48, every, 15, False, s) for t, s in zip(trajs, stats)], stats)
    return _WANT[every]


@pytest.mark.parametrize("every", EVERY)
def test_gliders_in_a_moore_ensemble(ens, every):
    """Universes a - e of the issue, f (see SHIPS), the random-fill oscillator B6/S5-7 seed 1 and an empty universe; mask 15, 48 steps at
    most."""
    names = list(SHIPS)
    trajs, rules, want, stats = first_test(every)
    make(ens, trajs, rules)
    got = quads(*ens.step_until_moving(48, check_every=every, stop_mask=15))
    print("every", every, "(steps_done, reason, period, shift):", got, "filter / failed:", [(s["filter"], s["failed"]) for s in stats])
    assert got == want
    assert ens.stats().kernel_launches == 1
    # the oracle's expectations are the ones the issue states
    for n in "abcf":
        d, r, p, sh = want[names.index(n)]
        a, b, normal = AXES[SHIPS[n][0]]
        assert (d, r, p) == STATED[every][:3] and abs(sh[a]) == abs(sh[b]) == STATED[every][3] and sh[normal] == 0, (n, want[names.index(n)])
    for n, stated in (("d", STATED_D[every]), ("e", STATED_E[every])):
        w = want[names.index(n)]
        assert w[1] == MOVING if stated == MOVING else (w[0], w[1]) == stated and w[2:] == (0, (0, 0, 0)), (n, w)
    assert want[-1] == (0, EXTINCT, 0, (0, 0, 0))  # empty: EXTINCT on entry, never MOVING
    assert want[-2][1] in (0, PERIODIC) and want[-2][3] == (0, 0, 0)
    check_states(ens, trajs, got)


def test_what_the_expectations_cover():
    """The expectations of the test above, over its five runs: shifts of both signs on all three axes; a comparison that failed after the
    filter had passed (at check_every 1 the glider's glide-reflected phases: six times a ship); a face case that is not MOVING."""
    names = list(SHIPS)
    wants = {every: first_test(every)[2] for every in EVERY}
    for want in wants.values():
        signs = {(axis, int(np.sign(w[3][axis]))) for w in want for axis in range(3) if w[3][axis]}
        assert signs == {(axis, s) for axis in range(3) for s in (-1, 1)}
    stats = first_test(1)[3]
    print("filter / failed at check_every 1:", [(s["filter"], s["failed"]) for s in stats])
    assert any(s["failed"] for s in stats) and stats[names.index("a")]["failed"] == 6
    assert any(want[names.index(n)][1] != MOVING for want in wants.values() for n in "de")


SILENT = ("27", "27", "27", "27")
CORNERS = ("6", "5-7", "27", "27", "", "1-8")  # universe a's glider under a corners table that fires (it keeps cells with a live corner neighbour)


@pytest.mark.parametrize("every", [1, 4])
def test_gliders_in_a_clustered_ensemble(ens, every):
    """A plain Moore rule is a clustered rule: the same ships, the same answers from ca_ensemble_clustered64_moving. The last universe's
    corners table fires; whatever the oracle says becomes of it is the expectation."""
    names = list(SHIPS)
    fires = traj("corners fire", lambda: glider(*SHIPS["a"]), ol.Rules.from_strings(neighbourhood="moore", **dict(zip(
        ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners"), CORNERS))))
    trajs = [ship(n) for n in names] + [filled("moore", OSCILLATOR), empty(), fires]
    make(ens, trajs, [SHIP + SILENT] * len(names) + [OSCILLATOR[:2] + SILENT, SHIP + SILENT, CORNERS], clustered=True)
    steps = 12  # (the oracle's clustered step is slow)
    want = [expected(t, 0, steps, every, 15, False) for t in trajs]
    got = quads(*ens.step_until_moving(steps, check_every=every, stop_mask=15))
    print("every", every, "(steps_done, reason, period, shift):", got)
    assert got == want
    assert [w[1] for w in want[:3]] == [MOVING] * 3 and not np.array_equal(fires[1], ship("a")[1])  # the corners table did fire
    check_states(ens, trajs, got)


@pytest.mark.parametrize("every", [1, 4])
def test_von_neumann_has_nothing_that_moves(ens, every):
    """The eleven von Neumann universes of tests/test_gpu_cycle.py: the definition, ca3d_ensemble_step_until_cycle's answer, no shift."""
    trajs = [filled("von neumann", c) for c in VN]
    make(ens, trajs, [c[:2] for c in VN], nb="von neumann")
    stats = {"filter": 0, "failed": 0}
    want = [expected(t, 0, 192, every, 15, False, stats) for t in trajs]
    got = quads(*ens.step_until_moving(192, check_every=every, stop_mask=15))
    print("every", every, "(steps_done, reason, period, shift):", got, stats)
    assert got == want
    assert all(g[3] == (0, 0, 0) and not g[1] & MOVING for g in got)
    check_states(ens, trajs, got)
    make(ens, trajs, [c[:2] for c in VN], nb="von neumann")
    done, reason, period = ens.step_until_cycle(192, check_every=every, stop_mask=7)
    assert [g[:3] for g in got] == list(zip(done.tolist(), reason.tolist(), period.tolist()))


def test_a_displacement_of_a_word_and_more(ens):
    trajs = [traj("far +", lambda: glider("xy", (2, 2, 30)), moore_rules(*SHIP)), traj("far -", lambda: glider("xz", (59, 20, 59), BOTH), moore_rules(*SHIP))]
    make(ens, trajs, [SHIP, SHIP])
    want = [expected(t, 0, 132, 132, 15, False) for t in trajs]
    got = quads(*ens.step_until_moving(132, check_every=132, stop_mask=15))
    print("(steps_done, reason, period, shift):", got)
    assert want == [(132, MOVING, 132, (33, 33, 0)), (132, MOVING, 132, (-33, 0, -33))]
    assert got == want
    check_states(ens, trajs, got)


def test_masks(ens):
    """Universe a and the oscillator. Mask 8 alone reports nothing but MOVING; without bit 8 the call is step_until_cycle, without bit 4
    as well step_until — one launch each."""
    trajs, rules = [ship("a"), filled("moore", OSCILLATOR)], [SHIP, OSCILLATOR[:2]]
    make(ens, trajs, rules)
    got = quads(*ens.step_until_moving(48, check_every=1, stop_mask=MOVING))
    assert got == [expected(t, 0, 48, 1, MOVING, False) for t in trajs] and got[1] == (48, 0, 0, (0, 0, 0)) and got[0][1] == MOVING
    assert ens.stats().kernel_launches == 1
    check_states(ens, trajs, got)
    for mask in (7, 3):
        make(ens, trajs, rules)
        got = quads(*ens.step_until_moving(48, check_every=1, stop_mask=mask))
        assert ens.stats().kernel_launches == 1
        state = ens.read_state()
        make(ens, trajs, rules)
        if mask == 7:
            done, reason, period = ens.step_until_cycle(48, check_every=1, stop_mask=7)
        else:
            done, reason = ens.step_until(48, check_every=1, stop_mask=3)
            period = np.zeros_like(done)
        assert ens.stats().kernel_launches == 1
        assert got == [(int(d), int(r), int(p), (0, 0, 0)) for d, r, p in zip(done, reason, period)], mask
        assert got == [expected(t, 0, 48, 1, mask, False) for t in trajs], mask
        np.testing.assert_array_equal(ens.read_state(), state)


def test_again(ens):
    """A second call from the stop state finds the ship again, with the same period and shift: the anchor does not survive a call."""
    names = ["a", "b", "c"]
    trajs = [ship(n) for n in names]
    make(ens, trajs, [SHIP] * 3)
    got = quads(*ens.step_until_moving(48, check_every=2, stop_mask=15))
    assert got == [expected(t, 0, 48, 2, 15, False) for t in trajs]
    got2 = quads(*ens.step_until_moving(48, check_every=2, stop_mask=15))
    assert got2 == [expected(t, g[0], 48, 2, 15, True) for t, g in zip(trajs, got)]
    assert all(g[1] == MOVING for g in got) and [g[1:] for g in got2] == [g[1:] for g in got]
    check_states(ens, trajs, got2, offsets=[g[0] for g in got])


def test_more_universes_than_compute_units(ens):
    """B = 300: ships whose plane, direction and corner come from the universe's number (36 different ones, all clear of the faces for the
    8 steps it takes to find them) alternating with the random fills; every universe against the definition."""
    B = 300
    planes = list(AXES)
    trajs, rules = [], []
    for u in range(B):
        if u % 2:
            c = MOORE[(u // 2) % len(MOORE)]
            trajs.append(filled("moore", c))
            rules.append(c[:2])
        else:
            v = (u // 2) % 36
            plane, flip = planes[v % 3], (bool(v // 3 & 1), bool(v // 6 & 1))
            corner = (12 + (v * 7) % 37, 12 + (v * 11) % 37, 12 + (v * 5) % 37)
            trajs.append(traj(("ship", v), lambda: glider(plane, corner, flip), moore_rules(*SHIP)))
            rules.append(SHIP)
    make(ens, trajs, rules)
    want = [expected(t, 0, 48, 1, 15, False) for t in trajs]
    got = quads(*ens.step_until_moving(48, check_every=1, stop_mask=15))
    assert got == want
    assert all(w[:3] == (8, MOVING, 4) for w in want[::2]) and len({w[3] for w in want[::2]}) == 12  # 3 planes x 4 directions
    state = ens.read_state()
    for u, t in enumerate(trajs):
        np.testing.assert_array_equal(state[u], t[got[u][0]], err_msg=f"universe {u}")


class Periodic:
    """An oracle trajectory continued past transient + period by periodicity — after the oracle itself has shown that state m + p is state
    m (tests/test_gpu_cycle.py's, on a Trajectory)."""

    def __init__(self, t, limit=200):
        seen, k = {}, 0
        while True:
            key = t[k].tobytes()
            if key in seen:
                break
            seen[key] = k
            k += 1
            assert k <= limit, "no cycle found"
        self.t, self.m, self.p = t, seen[key], k - seen[key]
        assert np.array_equal(t[self.m], t[self.m + self.p])

    def index(self, k):
        return k if k < self.m + self.p else self.m + (k - self.m) % self.p

    def __getitem__(self, k):
        return self.t[self.index(k)]

    def box(self, k):
        return self.t.box(self.index(k))

    def cells(self, k):
        return self.t.cells(self.index(k))


def test_the_anchor_survives_a_launch_cut(ens):
    """80 000 steps at most are two launches; the match — PERIODIC — comes in the second against the anchor, and its record, the first
    one left. A MOVING match across a cut cannot be produced in a 64^3 universe: no ship stays clear of the faces for 65 536 steps. The
    survival of the anchor's population and box is exercised through the path they share with its step and hash: they are loaded, kept
    and stored by the same code, and a box that came back wrong would let the filter pass or fail wrongly only where nothing moves."""
    case, every = ("5", "4,5", 2, 2), 9001
    t = Periodic(filled("moore", case))
    make(ens, [t], [case[:2]])
    want = expected(t, 0, 80000, every, 15, False)
    got = quads(*ens.step_until_moving(80000, check_every=every, stop_mask=15))
    print("transient", t.m, "period", t.p, "(steps_done, reason, period, shift):", got, "expected:", want)
    assert want[0] > 65536 and want[1] == PERIODIC and want[2] % t.p == 0 and want[2] % every == 0 and want[3] == (0, 0, 0)
    assert got == [want]
    assert ens.stats().kernel_launches == 2
    np.testing.assert_array_equal(ens.read_state()[0], t[want[0]])


def test_refusals(ens):
    lib = _capi.load()
    with pytest.raises(Ca3dError) as e:
        ens.step_until_moving(4)
    assert e.value.code == -2  # not configured
    ens.configure(3, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    ens.upload_state(0, np.zeros((3, W), dtype=np.uint32))
    for kw in (dict(check_every=0), dict(stop_mask=16), dict(stop_mask=31)):
        with pytest.raises(Ca3dError) as e:
            ens.step_until_moving(4, **kw)
        assert e.value.code == -1, kw
    done = (C.c_uint32 * 3)(77, 77, 77)
    shift = (C.c_int32 * 9)(*[5] * 9)
    assert lib.ca3d_ensemble_step_until_moving(ens._h, 4, 1, 16, done, None, None, shift) == -1
    assert list(done) == [77] * 3 and list(shift) == [5] * 9  # a refused call leaves the caller's arrays untouched
    assert lib.ca3d_ensemble_step_until_moving(ens._h, 4, 1, 15, None, None, None, None) == 0  # the four arrays are nullable
    for mask in (8, 15):  # the other calls keep refusing the bit
        with pytest.raises(Ca3dError) as e:
            ens.step_until_cycle(4, stop_mask=mask)
        assert e.value.code == -1
        with pytest.raises(Ca3dError) as e:
            ens.step_until(4, stop_mask=mask)
        assert e.value.code == -1
    # empty universes: EXTINCT on entry, never MOVING
    assert quads(*ens.step_until_moving(4, check_every=1)) == [(0, EXTINCT, 0, (0, 0, 0))] * 3
    assert quads(*ens.step_until_moving(4, check_every=2, stop_mask=MOVING)) == [(4, 0, 0, (0, 0, 0))] * 3
