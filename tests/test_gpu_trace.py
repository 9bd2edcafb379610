"""ca3d_ensemble_step_until_trace on the GPU: per-universe population curves written by ca_ensemble_vn64_trace / ca_ensemble_moore64_trace.
Expected values always come from CPU-oracle trajectories (oracle_lib.packed_step, host.state_summary) fed to `expected` below — the
definition in include/ca3d.h restated — never from the engine, never hard-coded. Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host

pytestmark = pytest.mark.gpu

G, W = 64, 8192
EXTINCT, STILL, PERIODIC = 1, 2, 4
MAX, AGAIN = 192, 16  # steps of the first call at most / of the call after it
# the rule / seed cases of test_gpu_cycle.py — (born, survive, seed, and_rounds) of host.random_fill(8192, seed, and_rounds): oscillators
# of periods 20, 12, 2, 6, 2, 4, 30, 24, one without a cycle in 192 steps, a fixed point, one that dies
VN = [("2,4", "1,3,5", 3, 5), ("3", "2,3", 1, 0), ("3", "2,3", 2, 2), ("2", "1-3", 3, 5), ("0", "", 1, 0), ("2", "0", 3, 5), ("2,3", "1", 3, 5),
      ("3,4", "0-2", 2, 2), ("1", "", 1, 0), ("1,3", "0-6", 1, 0), ("5,6", "4-6", 1, 0)]
# periods 4, 2, 2, 2, none in 192 steps, a fixed point, one that dies
MOORE = [("5", "4,5", 2, 2), ("5", "5", 2, 2), ("6", "5-7", 1, 0), ("6-8", "5-8", 3, 4), ("3", "2,3", 1, 0), ("5", "4,5", 1, 0), ("5", "5", 1, 0)]
CASES = {"von neumann": VN, "moore": MOORE}

_TRAJ, _COUNTS = {}, {}


def trajectory(nb, case, steps):
    """Oracle states 0 .. steps of one universe, computed once per module and extended on demand."""
    b, s, seed, rounds = case
    t = _TRAJ.setdefault((nb, case), [host.random_fill(W, seed=seed, and_rounds=rounds)])
    r = ol.Rules.from_strings(neighbourhood=nb, born=b, survive=s)
    while len(t) <= steps:
        t.append(ol.packed_step(G, t[-1], r))
    return t


def counts(cur, prev):
    """(population, births, deaths) of a state against the state one step earlier (None: no previous state) — host.state_summary's."""
    key = (cur.tobytes(), None if prev is None else prev.tobytes())
    if key not in _COUNTS:
        s = host.state_summary(G, cur, prev_words=prev)
        _COUNTS[key] = (s["population"], s["births"], s["deaths"])
    return _COUNTS[key]


def expected(t, start, max_steps, every, mask, has_prev):
    """(samples [K][3], n_samples, steps_done, reason) of a traced call that begins at state t[start]: the definition of include/ca3d.h."""
    K = -(-max_steps // every) + 1
    samples = np.zeros((K, 3), dtype=np.uint32)
    k = j = 0
    while True:
        cur = t[start + k]
        # entry: the record as it stands (births and deaths 0 without a previous state); later: the state against the one a step earlier
        samples[j] = counts(cur, t[start + k - 1] if (has_prev or k > 0) else None)
        fired = 0
        if not cur.any():
            fired |= EXTINCT
        if (has_prev or k > 0) and np.array_equal(cur, t[start + k - 1]):
            fired |= STILL
        fired &= mask  # the sample is taken before the stop decision
        if fired or k == max_steps:
            return samples, j + 1, k, fired
        k += min(every, max_steps - k)
        j += 1


def expected_cycle(t, start, max_steps, every, mask, has_prev):
    """(steps_done, reason, period) of a step_until_cycle that begins at state t[start] (test_gpu_cycle.py's restatement)."""
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
        if j > 0 and j & (j - 1) == 0:
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


def compare(got, want, cases):
    """A step_trace result against one `expected` tuple per universe."""
    samples, count, done, reason = got
    for u, (ws, wn, wd, wr) in enumerate(want):
        where = f"universe {u} {cases[u]}"
        assert (int(count[u]), int(done[u]), int(reason[u])) == (wn, wd, wr), where
        np.testing.assert_array_equal(samples[u], ws, err_msg=where)
        assert not samples[u, wn:].any(), where  # slots past n_samples are zero


@pytest.mark.parametrize("mask", [0, 3])
@pytest.mark.parametrize("every", [1, 4, 5])
@pytest.mark.parametrize("nb", ["von neumann", "moore"])
def test_every_universe_leaves_its_curve(ens, nb, every, mask):
    cases = CASES[nb]
    make(ens, nb, cases)
    trajs = [trajectory(nb, c, MAX) for c in cases]
    K = host.trace_samples(MAX, every)
    got = ens.step_trace(MAX, check_every=every, stop_mask=mask)
    want = [expected(t, 0, MAX, every, mask, False) for t in trajs]
    print(nb, "every", every, "mask", mask, "n_samples", got[1].tolist(), "steps_done", got[2].tolist(), "reason", got[3].tolist())
    assert got[0].shape == (len(cases), K, 3)
    compare(got, want, cases)
    if mask == 0:  # nothing stops: every universe has K samples
        assert got[1].tolist() == [K] * len(cases) and got[2].tolist() == [MAX] * len(cases) and not got[3].any()
    else:  # one that dies, one that freezes, several that run on
        reasons = [w[3] for w in want]
        assert any(r & EXTINCT for r in reasons) and any(r == STILL for r in reasons) and reasons.count(0) >= 3
    state, recs = ens.read_state(), ens.summaries()
    for k, t in enumerate(trajs):
        d = want[k][2]
        np.testing.assert_array_equal(state[k], t[d], err_msg=f"{cases[k]}: state after {d} steps")
        check(recs[k], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, f"{cases[k]}")
    assert ens.stats().cell_steps == float(sum(w[2] for w in want)) * G ** 3 and ens.stats().kernel_launches == 1

    # a second call on the same handle: sample 0 is the record the first call left, births and deaths included
    got2 = ens.step_trace(AGAIN, check_every=every, stop_mask=mask)
    want2 = [expected(trajectory(nb, c, w[2] + AGAIN), w[2], AGAIN, every, mask, w[2] > 0) for c, w in zip(cases, want)]
    compare(got2, want2, cases)
    first = got2[0][:, 0, :]
    assert any(first[u, 1] or first[u, 2] for u in range(len(cases)))  # an oscillator's entry sample has births or deaths
    state = ens.read_state()
    for k, c in enumerate(cases):
        d = want[k][2] + want2[k][2]
        np.testing.assert_array_equal(state[k], trajectory(nb, c, d)[d], err_msg=f"{c}: after the second call")


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


@pytest.mark.parametrize("nb,case", [("von neumann", ("2,3", "1", 3, 5)), ("moore", ("5", "4,5", 2, 2))])
def test_the_curve_survives_a_launch_cut(ens, nb, case):
    """65 536 + 3000 steps are two launches. The first ends on the last check point before step 65 536, which is sampled there and not
    again on entry of the second; the last sample, at max_steps, lies between two regular check points."""
    total, every = 65536 + 3000, 1181
    make(ens, nb, [case])
    t = Periodic(nb, case)
    print("transient", t.m, "period", t.p)
    want = expected(t, 0, total, every, 0, False)
    # (the definition's K = ceil(68 536 / 1181) + 1: check points 0 .. 58 x 1181 and the one at 68 536)
    assert want[1] == host.trace_samples(total, every) == 60 and want[2] == total and total % every
    got = ens.step_trace(total, check_every=every, stop_mask=0)
    print("samples", got[0][0, :3].tolist(), "...", got[0][0, -2:].tolist())
    compare(got, [want], [case])
    assert ens.stats().kernel_launches == 2
    np.testing.assert_array_equal(ens.read_state()[0], t[total])
    check(ens.summaries()[0], host.state_summary(G, t[total], prev_words=t[total - 1]), total, "the oscillator")


def test_more_universes_than_compute_units(ens):
    B, steps, every = 300, 24, 3
    rule = ("2,4", "1,3,5")
    cases = [rule + (1 + u, 0) for u in range(B)]
    make(ens, "von neumann", cases)
    got = ens.step_trace(steps, check_every=every, stop_mask=0)
    want = [expected(trajectory("von neumann", c, steps), 0, steps, every, 0, False) for c in cases]
    assert got[0].shape == (B, 9, 3) and got[1].tolist() == [9] * B
    compare(got, want, cases)


def test_refusals_leave_the_arrays_alone(ens):
    lib = _capi.load()
    n, K = 3, host.trace_samples(8, 2)
    done, reason, count = ((C.c_uint32 * n)(*([v] * n)) for v in (77, 78, 79))
    samples = (C.c_uint32 * (n * K * 3))(*([80] * (n * K * 3)))

    def call(max_steps=8, every=2, mask=3, per=K):
        rc = lib.ca3d_ensemble_step_until_trace(ens._h, max_steps, every, mask, done, reason, samples, per, count)
        assert list(done) == [77] * n and list(reason) == [78] * n and list(count) == [79] * n and list(samples) == [80] * (n * K * 3)
        return rc, lib.ca3d_last_error().decode()

    assert call()[0] == -2  # not configured
    with pytest.raises(Ca3dError) as e:
        ens.step_trace(8)
    assert e.value.code == -2
    ens.configure(n)
    assert call()[0] == -2  # no rules
    ens.set_rule_strings(_capi.ENSEMBLE_ALL)
    ens.upload_state(0, np.zeros((2, W), dtype=np.uint32))
    assert call()[0] == -2  # universe 2 has no state
    ens.upload_state(2, np.zeros(W, dtype=np.uint32))
    rc, msg = call(mask=PERIODIC)
    assert rc == -1 and "unknown bits" in msg
    assert call(mask=7)[0] == -1
    assert call(every=0)[0] == -1
    rc, msg = call(per=K - 1)
    assert rc == -1 and f"K = {K}" in msg
    for kw in (dict(check_every=0), dict(stop_mask=4)):
        with pytest.raises(Ca3dError) as e:
            ens.step_trace(8, **kw)
        assert e.value.code == -1, kw
    # samples is required; the other three arrays are nullable
    assert lib.ca3d_ensemble_step_until_trace(ens._h, 8, 2, 3, None, None, None, K, None) == -1
    assert lib.ca3d_ensemble_step_until_trace(ens._h, 8, 2, 3, None, None, samples, K, None) == 0
    # empty universes: EXTINCT on entry, one sample of zeros each; a roomier array is zeroed past K as well
    assert list(samples) == [0] * (n * K * 3)
    roomy = (C.c_uint32 * (n * (K + 2) * 3))(*([80] * (n * (K + 2) * 3)))
    assert lib.ca3d_ensemble_step_until_trace(ens._h, 8, 2, 3, done, reason, roomy, K + 2, count) == 0
    assert list(roomy) == [0] * (n * (K + 2) * 3) and list(count) == [1] * n and list(done) == [0] * n and list(reason) == [EXTINCT] * n
    got = ens.step_trace(8, check_every=2, stop_mask=3)
    assert got[1].tolist() == [1] * n and got[2].tolist() == [0] * n and got[3].tolist() == [EXTINCT] * n and not got[0].any()


@pytest.mark.parametrize("nb", ["von neumann", "moore"])
def test_the_other_calls_still_work_on_a_handle_that_has_traced(ens, nb):
    cases = CASES[nb]
    make(ens, nb, cases)
    ens.step_trace(8, check_every=2)
    make(ens, nb, cases)  # (a configure frees the sample array with the others)
    first = 8
    got = ens.step_trace(first, check_every=2)
    compare(got, [expected(trajectory(nb, c, first), 0, first, 2, 0, False) for c in cases], cases)
    done, reason, period = ens.step_until_cycle(MAX, check_every=1, stop_mask=7)
    want = [expected_cycle(trajectory(nb, c, first + MAX), first, MAX, 1, 7, True) for c in cases]
    assert list(zip(done.tolist(), reason.tolist(), period.tolist())) == want
    assert {w[1] for w in want} >= {0, PERIODIC}
    state = ens.read_state()
    for k, c in enumerate(cases):
        np.testing.assert_array_equal(state[k], trajectory(nb, c, first + MAX)[first + want[k][0]], err_msg=f"{c}")
    # ... and plain stepping and step_until after that
    at = [first + w[0] for w in want]
    ens.step(3)
    done, reason = ens.step_until(4, check_every=2, stop_mask=0)
    assert done.tolist() == [4] * len(cases) and not reason.any()
    state = ens.read_state()
    for k, c in enumerate(cases):
        np.testing.assert_array_equal(state[k], trajectory(nb, c, at[k] + 7)[at[k] + 7], err_msg=f"{c}")
