"""CA3D_STOP_PERIODIC on the GPU: ca3d_ensemble_step_until_cycle (decided inside ca_ensemble_vn64_cycle / ca_ensemble_moore64_cycle for every
universe on its own) and ca3d_step_until_cycle (a full-grid engine). Expected values always come from CPU-oracle trajectories
(oracle_lib.packed_step / unpacked_step) fed to `expected` below — the definition in include/ca3d.h restated — never from the engine, never
hard-coded. Every comparison is exact."""
import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import LAYOUT_UNPACKED, Ca3dError, _capi, host

pytestmark = pytest.mark.gpu

G, W = 64, 8192
EXTINCT, STILL, PERIODIC = 1, 2, 4
MAX, AGAIN = 192, 64  # steps of the first call at most / of the call after it
# (born, survive, seed, and_rounds) of host.random_fill(8192, seed, and_rounds): oscillators of periods 20, 12, 2, 6, 2 (through near-empty
# and full grids), 4, 30, 24, one without a cycle in 192 steps, a fixed point, one that dies
VN = [("2,4", "1,3,5", 3, 5), ("3", "2,3", 1, 0), ("3", "2,3", 2, 2), ("2", "1-3", 3, 5), ("0", "", 1, 0), ("2", "0", 3, 5), ("2,3", "1", 3, 5),
      ("3,4", "0-2", 2, 2), ("1", "", 1, 0), ("1,3", "0-6", 1, 0), ("5,6", "4-6", 1, 0)]
# periods 4, 2, 2, 2, none in 192 steps, a fixed point, one that dies
MOORE = [("5", "4,5", 2, 2), ("5", "5", 2, 2), ("6", "5-7", 1, 0), ("6-8", "5-8", 3, 4), ("3", "2,3", 1, 0), ("5", "4,5", 1, 0), ("5", "5", 1, 0)]
CASES = {"von neumann": VN, "moore": MOORE}

_TRAJ = {}


def trajectory(nb, case, steps):
    """Oracle states 0 .. steps of one universe, computed once per module and extended on demand."""
    b, s, seed, rounds = case
    t = _TRAJ.setdefault((nb, case), [host.random_fill(W, seed=seed, and_rounds=rounds)])
    r = ol.Rules.from_strings(neighbourhood=nb, born=b, survive=s)
    while len(t) <= steps:
        t.append(ol.packed_step(G, t[-1], r))
    return t


def expected(t, start, max_steps, every, mask, has_prev):
    """(steps_done, reason, period) of a step_until_cycle that begins at state t[start]: the definition of include/ca3d.h."""
    k = j = anchor = 0
    while True:
        cur = t[start + k]
        fired = 0
        if not cur.any():
            fired |= EXTINCT
        if (has_prev or k > 0) and np.array_equal(cur, t[start + k - 1]):
            fired |= STILL
        if j > 0 and np.array_equal(cur, t[start + anchor]):
            fired |= PERIODIC
        fired &= mask
        if fired or k == max_steps:
            return k, fired, (k - anchor if fired & PERIODIC else 0)
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


def make(ens, nb, cases):
    ens.configure(len(cases), neighbourhood=nb)
    for k, (b, s, _, _) in enumerate(cases):
        ens.set_rule_strings(k, neighbourhood=nb, born=b, survive=s)
    ens.upload_state(0, np.stack([trajectory(nb, c, 0)[0] for c in cases]))


def check(s, want, step, where):
    """Every field of a record against a host.state_summary dict."""
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


def triples(done, reason, period):
    return list(zip(done.tolist(), reason.tolist(), period.tolist()))


@pytest.mark.parametrize("every,mask", [(1, 7), (4, 7), (5, 7), (1, 4)])
@pytest.mark.parametrize("nb", ["von neumann", "moore"])
def test_every_universe_finds_its_cycle(ens, nb, every, mask):
    cases = CASES[nb]
    make(ens, nb, cases)
    trajs = [trajectory(nb, c, MAX) for c in cases]
    got = triples(*ens.step_until_cycle(MAX, check_every=every, stop_mask=mask))
    want = [expected(t, 0, MAX, every, mask, False) for t in trajs]
    print(nb, "every", every, "mask", mask, "(steps_done, reason, period):", got)
    assert got == want
    reasons, periods = {w[1] for w in want}, {w[2] for w in want}
    if every == 1 and mask == 7:  # the outcome classes all occur
        if nb == "von neumann":
            assert {0, EXTINCT, STILL, PERIODIC} <= reasons and {2, 4, 6, 12, 20} <= periods
        else:
            assert {0, PERIODIC} <= reasons and {2, 4} <= periods and any(r & EXTINCT for r in reasons) and any(r & STILL for r in reasons)
    if every == 5 and nb == "von neumann":
        assert want[7][:2] == (MAX, 0)  # period 24: lcm(24, 5) = 120 does not fit between two anchor moves within 192 steps
    state, recs = ens.read_state(), ens.summaries()
    for k, t in enumerate(trajs):
        d = got[k][0]
        np.testing.assert_array_equal(state[k], t[d], err_msg=f"{cases[k]}: state after {d} steps")
        check(recs[k], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, f"{cases[k]}")
    assert ens.stats().cell_steps == float(sum(g[0] for g in got)) * G ** 3 and ens.stats().kernel_launches == 1

    # again: every call starts from its own entry state, the anchor did not survive
    got2 = triples(*ens.step_until_cycle(AGAIN, check_every=every, stop_mask=mask))
    want2 = [expected(trajectory(nb, c, g[0] + AGAIN), g[0], AGAIN, every, mask, g[0] > 0) for c, g in zip(cases, got)]
    print("again:", got2)
    assert got2 == want2
    if every == 1:
        assert any(a[1] & PERIODIC and b[1] & PERIODIC and a[2] == b[2] for a, b in zip(got, got2))  # a cycle found is found again
    state = ens.read_state()
    for k, c in enumerate(cases):
        np.testing.assert_array_equal(state[k], trajectory(nb, c, got[k][0] + got2[k][0])[got[k][0] + got2[k][0]], err_msg=f"{c}: after the second call")


@pytest.mark.parametrize("nb", ["von neumann", "moore"])
def test_without_the_periodic_bit_it_is_step_until(ens, nb):
    cases = CASES[nb]
    make(ens, nb, cases)
    done, reason, period = ens.step_until_cycle(MAX, check_every=4, stop_mask=3)
    state = ens.read_state()
    make(ens, nb, cases)
    done0, reason0 = ens.step_until(MAX, check_every=4, stop_mask=3)
    assert done.tolist() == done0.tolist() and reason.tolist() == reason0.tolist() and not period.any()
    np.testing.assert_array_equal(ens.read_state(), state)
    assert triples(done, reason, period) == [expected(trajectory(nb, c, MAX), 0, MAX, 4, 3, False) for c in cases]


class Periodic:
    """An oracle trajectory continued past transient + period by periodicity — after the oracle itself has shown that state m + p is state
    m, that the p states of the cycle are pairwise different and that m is where the cycle begins."""

    def __init__(self, nb, case, limit=200):
        seen, k = {}, 0
        while True:
            t = trajectory(nb, case, k)
            key = t[k].tobytes()
            if key in seen:
                break
            seen[key] = k
            k += 1
            assert k <= limit, "no cycle found"
        self.t, self.m, self.p = t, seen[key], k - seen[key]
        m, p = self.m, self.p
        assert np.array_equal(t[m], t[m + p]) and len({t[i].tobytes() for i in range(m, m + p)}) == p
        assert m == 0 or not np.array_equal(t[m - 1], t[m + p - 1])

    def __getitem__(self, k):
        return self.t[k] if k < self.m + self.p else self.t[self.m + (k - self.m) % self.p]


@pytest.mark.parametrize("nb,case,every", [("von neumann", ("2,3", "1", 3, 5), 1181), ("moore", ("5", "4,5", 2, 2), 9001)])
def test_the_anchor_survives_a_launch_cut(ens, nb, case, every):
    """80 000 steps at most are two launches. The first ends on the last check point before step 65 536; by then the anchor has moved
    several times, and the match comes in the second launch against the anchor the first one left."""
    dies = ("", "", case[2], case[3])
    make(ens, nb, [case, dies])
    t, t_dies = Periodic(nb, case), Periodic(nb, dies)
    print("transient", t.m, "period", t.p)
    want = [expected(t, 0, 80000, every, 7, False), expected(t_dies, 0, 80000, every, 7, False)]
    got = triples(*ens.step_until_cycle(80000, check_every=every, stop_mask=7))
    print("(steps_done, reason, period):", got, "expected:", want)
    assert want[0][0] > 65536 and want[0][1] == PERIODIC and want[0][2] % t.p == 0 and want[0][2] % every == 0  # found in the second launch
    assert want[1] == (every, EXTINCT | STILL, 0)
    assert got == want
    assert ens.stats().kernel_launches == 2
    state, recs = ens.read_state(), ens.summaries()
    d = got[0][0]
    np.testing.assert_array_equal(state[0], t[d])
    check(recs[0], host.state_summary(G, t[d], prev_words=t[d - 1]), d, "the oscillator")
    assert not state[1].any() and recs[1].step == every


def test_more_universes_than_compute_units(ens):
    B = 300
    cases = [VN[u % len(VN)] for u in range(B)]
    make(ens, "von neumann", cases)
    got = triples(*ens.step_until_cycle(MAX, check_every=1, stop_mask=7))
    want = [expected(trajectory("von neumann", c, MAX), 0, MAX, 1, 7, False) for c in VN]
    assert got == [want[u % len(VN)] for u in range(B)]
    state = ens.read_state()
    for u in range(B):
        np.testing.assert_array_equal(state[u], trajectory("von neumann", cases[u], MAX)[got[u][0]], err_msg=f"universe {u}")


@pytest.fixture()
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("every", [1, 8])
@pytest.mark.parametrize("nb,case", [("von neumann", VN[0]), ("von neumann", VN[2]), ("von neumann", VN[9]), ("moore", MOORE[1])])
def test_engine_packed(eng, ens, nb, case, every):
    """A lone 64^3 engine: the same answer as the definition and as an ensemble holding the same universe. Batches of 8 steps take the
    resident kernel and its rotation of three buffers."""
    t = trajectory(nb, case, MAX)
    eng.configure(G)
    eng.set_rule_strings(neighbourhood=nb, born=case[0], survive=case[1])
    eng.upload_state(t[0])
    done, reason, period, s = eng.step_until_cycle(MAX, check_every=every)
    want = expected(t, 0, MAX, every, 7, False)
    print(nb, case, "every", every, "(steps_done, reason, period):", (done, reason, period), "kernel", eng.info().kernel_name)
    assert (done, reason, period) == want
    np.testing.assert_array_equal(eng.read_state(), t[done])
    check(s, host.state_summary(G, t[done], prev_words=t[done - 1] if done else None), done, "the last summary")
    assert eng.info().step == done and eng.recovered_launches() == 0
    make(ens, nb, [case])
    assert triples(*ens.step_until_cycle(MAX, check_every=every)) == [want]
    # again, with one condition only: EXTINCT / STILL are not reported, the cycle is
    done2, reason2, period2, _ = eng.step_until_cycle(AGAIN, check_every=every, extinct=False, still=False)
    assert (done2, reason2, period2) == expected(trajectory(nb, case, done + AGAIN), done, AGAIN, every, PERIODIC, done > 0)
    np.testing.assert_array_equal(eng.read_state(), trajectory(nb, case, done + done2)[done + done2])


def test_engine_unpacked(eng):
    """32^3, one word per cell, born at 0 neighbours and nothing survives, from the empty grid (EXTINCT not watched)."""
    g = 32
    r = ol.Rules.from_strings(born="0", survive="")
    t = [np.zeros(g ** 3, dtype=np.uint32)]
    for _ in range(16):
        t.append(ol.unpacked_step(g, t[-1], r.main, r.survive, r.born))
    eng.configure(g, LAYOUT_UNPACKED)
    eng.set_rule_strings(born="0", survive="")
    eng.upload_state(t[0])
    got = eng.step_until_cycle(16, check_every=1, extinct=False)
    want = expected(t, 0, 16, 1, STILL | PERIODIC, False)
    print("(steps_done, reason, period):", got[:3])
    assert got[:3] == want and want[1] == PERIODIC
    np.testing.assert_array_equal(eng.read_state(), t[got[0]])
    assert eng.recovered_launches() == 0


def test_engine_refusals(eng):
    lib = _capi.load()
    rec = _capi.SummaryStruct()
    import ctypes as C

    assert lib.ca3d_step_until_cycle(eng._h, 4, 1, 7, C.byref(rec), None, None, None) == -2  # not configured
    eng.configure(G)
    eng.set_rule_strings()
    eng.upload_state(np.zeros(W, dtype=np.uint32))
    assert lib.ca3d_step_until_cycle(eng._h, 4, 0, 7, C.byref(rec), None, None, None) == -1  # check_every 0
    assert lib.ca3d_step_until_cycle(eng._h, 4, 1, 8, C.byref(rec), None, None, None) == -1  # unknown bit
    assert lib.ca3d_step_until_cycle(eng._h, 4, 1, 7, None, None, None, None) == -1  # out is NULL
    assert lib.ca3d_step_until(eng._h, 4, 1, 4, C.byref(rec), None, None) == -1  # the first call still refuses the bit
    assert lib.ca3d_step_until_cycle(eng._h, 4, 1, 7, C.byref(rec), None, None, None) == 0  # the three outputs are nullable
    eng.configure_slab(G, 16, 16, 1)
    with pytest.raises(Ca3dError) as e:
        eng.step_until_cycle(4)
    assert e.value.code == -5


def test_ensemble_refusals(ens):
    lib = _capi.load()
    with pytest.raises(Ca3dError) as e:
        ens.step_until_cycle(4)
    assert e.value.code == -2  # not configured
    ens.configure(3)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL)
    ens.upload_state(0, np.zeros((2, W), dtype=np.uint32))
    with pytest.raises(Ca3dError) as e:
        ens.step_until_cycle(4)
    assert e.value.code == -2  # universe 2 has no state
    ens.upload_state(2, np.zeros(W, dtype=np.uint32))
    for kw in (dict(check_every=0), dict(stop_mask=8), dict(stop_mask=15)):
        with pytest.raises(Ca3dError) as e:
            ens.step_until_cycle(4, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(Ca3dError) as e:
        ens.step_until(4, stop_mask=4)  # the first call still refuses the bit
    assert e.value.code == -1
    assert lib.ca3d_ensemble_step_until_cycle(ens._h, 4, 1, 7, None, None, None) == 0  # the three arrays are nullable
    # empty universes: EXTINCT on entry, PERIODIC never fires on entry
    assert triples(*ens.step_until_cycle(4, check_every=1)) == [(0, EXTINCT, 0)] * 3
    assert triples(*ens.step_until_cycle(4, check_every=2, stop_mask=PERIODIC)) == [(2, PERIODIC, 2)] * 3


def _filter_blind_pair():
    """Two single cells, not in row 0 and far apart, whose state the kernels' 32-bit filter cannot tell from the empty grid: cycle_mix of
    csrc/ca_ensemble.hip restated, searched for a pair of (word, bit) whose contributions cancel modulo 2^32. (If that hash ever changes the
    test below still holds — its expectation comes from the oracle — but no longer forces the comparison of all words.)"""
    idx = np.arange(W, dtype=np.uint64)[:, None]
    w = (np.uint64(1) << np.arange(32, dtype=np.uint64))[None, :]

    def mix(word):
        x = ((word ^ (word >> np.uint64(16)) ^ ((idx * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF))) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
        return x ^ (x >> np.uint64(15))

    d = ((mix(w) - mix(np.zeros_like(w))) & np.uint64(0xFFFFFFFF)).ravel()  # what cell (word, bit) adds to the empty grid's sum
    rows = (np.arange(W * 32) // 32 // 2) % 64
    order = np.argsort(d)
    ds = d[order]
    pos = np.searchsorted(ds, (np.uint64(1 << 32) - d) & np.uint64(0xFFFFFFFF))
    for a in range(d.size):
        p = int(pos[a])
        while p < d.size and int(ds[p]) == ((1 << 32) - int(d[a])) & 0xFFFFFFFF:
            b = int(order[p])
            if rows[a] and rows[b] and abs(a // 32 - b // 32) > 600:  # both outside lane 0; more than four planes apart
                return a, b
            p += 1
    return None


@pytest.mark.parametrize("nb", ["von neumann", "moore"])
def test_equal_hashes_are_not_equal_states(ens, nb):
    """Two lone cells die in one step. Their state and the empty grid after it have the same filter hash, and neither cell is in the lane
    that writes the workgroup's verdict: only the comparison of every word, with every lane voting, keeps PERIODIC from firing at step 1."""
    pair = _filter_blind_pair()
    assert pair is not None
    first = np.zeros(W, dtype=np.uint32)
    for c in pair:
        first[c // 32] |= np.uint32(1 << (c % 32))
    r = ol.Rules.from_strings(neighbourhood=nb, born="", survive="")
    t = [first]
    for _ in range(4):
        t.append(ol.packed_step(G, t[-1], r))
    assert t[0].any() and not t[1].any()
    ens.configure(1, neighbourhood=nb)
    ens.set_rule_strings(0, neighbourhood=nb, born="", survive="")
    ens.upload_state(0, first)
    want = expected(t, 0, 4, 1, PERIODIC, False)
    got = triples(*ens.step_until_cycle(4, check_every=1, stop_mask=PERIODIC))
    print("cells", pair, "(steps_done, reason, period):", got)
    assert want == (2, PERIODIC, 1) and got == [want]
