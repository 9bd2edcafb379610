"""ca3d_ensemble_* on the GPU: many 64^3 universes in one launch, each with its own rule, record and end. Expected values always come
from CPU-oracle trajectories (oracle_lib.packed_step) and the numpy definition of a summary (host.state_summary) — never from the
engine, never hard-coded. Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host

pytestmark = pytest.mark.gpu

G, W = 64, 8192
STOP_EXTINCT, STOP_STILL = 1, 2
# born / survive over the von Neumann count; universe u runs rule u % 10
RULES = [("1,3", "0-6"), ("2,4", "1,3,5"), ("", ""), ("", "0-6"), ("3", "2,3"), ("1", ""), ("4-6", "3-6"), ("5,6", "4-6"), ("0", "0-6"),
         ("2", "1-3")]


def rule_of(u):
    b, s = RULES[u % 10]
    return ol.Rules.from_strings(born=b, survive=s)


def fill_of(u):
    return host.random_fill(W, seed=1 + u, and_rounds=(0, 2, 5)[u % 3])


_TRAJ = {}


def trajectory(key, first, rules, steps):
    """Oracle states 0 .. steps of one universe, computed once per module and extended on demand."""
    t = _TRAJ.setdefault(key, [first])
    while len(t) <= steps:
        t.append(ol.packed_step(G, t[-1], rules))
    return t


def universe(u, steps):
    return trajectory(("u", u), fill_of(u), rule_of(u), steps)


def make(ens, universes):
    """An ensemble of the numbered universes: rule u % 10 and fill u each, set one by one, uploaded together."""
    ens.configure(len(universes))
    for k, u in enumerate(universes):
        b, s = RULES[u % 10]
        ens.set_rule_strings(k, born=b, survive=s)
    ens.upload_state(0, np.stack([fill_of(u) for u in universes]))


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def check(s, want, step, where):
    """Every field of a record against a host.state_summary dict."""
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where
    assert s.plane_population is None


@pytest.mark.parametrize("B", [1, 3, 256, 300, 1024])
def test_parity_with_the_oracle(ens, B):
    """Every universe after step(1), step(7), step(24) equals the oracle after 1, 8, 32 steps. 300 and 1024: more workgroups than CUs.
    1024: a fixed sample of 128 universes with the first, the 256th, its successor and the last."""
    make(ens, range(B))
    sample = list(range(B)) if B <= 300 else sorted((set(range(0, B, 8)) - {8, 16}) | {255, B - 1})
    assert len(sample) == min(B, 128) or B <= 300
    done = 0
    for n in (1, 7, 24):
        ens.step(n)
        done += n
        got = ens.read_state()
        assert got.shape == (B, W)
        for u in sample:
            np.testing.assert_array_equal(got[u], universe(u, done)[done], err_msg=f"B={B} universe {u} (rule {RULES[u % 10]}) after {done} steps")
    st = ens.stats()
    assert st.steps == 24 and st.kernel_launches == 1 and st.cell_steps == 24.0 * B * G ** 3 and st.gpu_ms > 0


def test_boundary_asymmetry(ens):
    """Single cells on each face: coordinate -1 is dead, coordinate 64 wraps to 0 — on every axis."""
    faces = [(0, 20, 30), (63, 21, 31), (22, 0, 32), (23, 63, 33), (24, 34, 0), (25, 35, 63), (31, 5, 5), (32, 6, 6), (0, 0, 0), (63, 63, 63)]
    firsts = [host.cells_to_words(G, [c]) for c in faces] + [host.cells_to_words(G, faces)]
    ens.configure(len(firsts))
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, born="1", survive="")
    ens.upload_state(0, np.stack(firsts))
    r = ol.Rules.from_strings(born="1", survive="")
    done = 0
    for n in (1, 1, 3):
        ens.step(n)
        done += n
        got = ens.read_state()
        for k, w in enumerate(firsts):
            np.testing.assert_array_equal(got[k], trajectory(("face", k), w, r, done)[done], err_msg=f"universe {k} after {done} steps")


def test_records_equal_the_definition_and_a_lone_engine(ens):
    from cellularautomatons3d_amd import Engine

    B = 23
    make(ens, range(B))
    for u, s in enumerate(ens.summaries()):
        check(s, host.state_summary(G, universe(u, 0)[0]), 0, f"universe {u} after upload")
        assert not s.has_previous
    done = 0
    with Engine(0) as lone:
        lone.configure(G)
        for n in (1, 24):
            ens.step(n)
            done += n
            recs = ens.summaries()
            for u, s in enumerate(recs):
                t = universe(u, done)
                check(s, host.state_summary(G, t[done], prev_words=t[done - 1]), done, f"universe {u} after {done} steps")
                assert s.has_previous
            for u in (0, 1, 7, 22):
                r = rule_of(u)
                lone.set_rules(r.main, r.edges, r.corners, r.survive, r.born)
                lone.upload_state(fill_of(u))
                lone.step(done)
                one = lone.summary()
                one.plane_population = None
                assert recs[u] == one, f"universe {u} after {done} steps"
    part = ens.summaries(first=5, count=3)
    assert part == ens.summaries()[5:8]
    # an upload resets the uploaded universes only
    ens.upload_state(3, universe(3, 0)[0])
    recs = ens.summaries()
    check(recs[3], host.state_summary(G, universe(3, 0)[0]), 0, "universe 3 uploaded again")
    assert recs[2].step == done and recs[4].step == done


def expected_stop(t, start, max_steps, every, mask, has_prev):
    """(steps_done, reason) of a step_until that begins at state t[start]: conditions looked at on entry, after every `every` steps
    and after max_steps."""
    k = 0
    while True:
        cur = t[start + k]
        fired = 0
        if not cur.any():
            fired |= STOP_EXTINCT
        if (has_prev or k > 0) and np.array_equal(cur, t[start + k - 1]):
            fired |= STOP_STILL
        fired &= mask
        if fired or k == max_steps:
            return k, fired
        k += min(every, max_steps - k)


@pytest.mark.parametrize("every", [1, 4])
def test_every_universe_stops_on_its_own(ens, every):
    """Ten rules x seeds 1-3: some die, some freeze, some never settle — each stops (or not) where the oracle says, and stays there."""
    cases = [(r, seed) for r in range(10) for seed in (1, 2, 3)]
    firsts = [host.random_fill(W, seed=seed, and_rounds=(0, 2, 5)[seed - 1]) for _, seed in cases]
    ens.configure(len(cases))
    for k, (r, _) in enumerate(cases):
        ens.set_rule_strings(k, born=RULES[r][0], survive=RULES[r][1])
    ens.upload_state(0, np.stack(firsts))
    mask = STOP_EXTINCT | STOP_STILL
    trajs = [trajectory(("stop",) + c, w, ol.Rules.from_strings(born=RULES[c[0]][0], survive=RULES[c[0]][1]), 64 + 8) for c, w in zip(cases, firsts)]

    done, reason = ens.step_until(64, check_every=every, stop_mask=mask)
    want = [expected_stop(t, 0, 64, every, mask, False) for t in trajs]
    print("steps_done", done.tolist(), "reason", reason.tolist())
    assert done.tolist() == [w[0] for w in want] and reason.tolist() == [w[1] for w in want]
    # all three outcomes occurred: died out (seen a step late, an empty grid is still as well), froze alive, still changing after 64 steps
    assert any(r & STOP_EXTINCT for r in reason) and any(r == STOP_STILL for r in reason)
    assert any(r == 0 and d == 64 for d, r in zip(done, reason))
    got = ens.read_state()
    recs = ens.summaries()
    for k, t in enumerate(trajs):
        d = int(done[k])
        np.testing.assert_array_equal(got[k], t[d], err_msg=f"case {cases[k]}: state after {d} steps")  # a stopped universe did not move on
        check(recs[k], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, f"case {cases[k]}")
    st = ens.stats()
    assert st.cell_steps == float(int(done.sum())) * G ** 3 and st.steps == 64

    # again: whoever still satisfies a condition takes no step, the others take theirs
    done2, reason2 = ens.step_until(8, check_every=every, stop_mask=mask)
    want2 = [expected_stop(t, int(d), 8, every, mask, d > 0) for t, d in zip(trajs, done)]
    assert done2.tolist() == [w[0] for w in want2] and reason2.tolist() == [w[1] for w in want2]
    for k in range(len(cases)):
        if reason[k]:
            assert done2[k] == 0 and reason2[k] == reason[k]
    got = ens.read_state()
    for k, t in enumerate(trajs):
        np.testing.assert_array_equal(got[k], t[int(done[k]) + int(done2[k])])

    # only one bit watched; no bit watched: plain stepping
    ens.upload_state(0, np.stack(firsts))
    done3, reason3 = ens.step_until(8, check_every=every, stop_mask=STOP_EXTINCT)
    want3 = [expected_stop(t, 0, 8, every, STOP_EXTINCT, False) for t in trajs]
    assert done3.tolist() == [w[0] for w in want3] and reason3.tolist() == [w[1] for w in want3]
    ens.upload_state(0, np.stack(firsts))
    done4, reason4 = ens.step_until(3, check_every=every, stop_mask=0)
    assert done4.tolist() == [3] * len(cases) and not reason4.any()
    got = ens.read_state()
    for k, t in enumerate(trajs):
        np.testing.assert_array_equal(got[k], t[3])


def test_long_calls_are_cut_into_launches(ens):
    """max_steps above 65 536 on two universes — one that keeps changing, one that dies: the check points do not divide the launch
    length, the dead universe leaves the later launches at once, and the survivor equals a lone engine stepped as often."""
    from cellularautomatons3d_amd import Engine

    ens.configure(2)
    ens.set_rule_strings(0, born="2,4", survive="1,3,5")
    ens.set_rule_strings(1, born="", survive="")
    w = np.stack([fill_of(0), fill_of(1)])
    ens.upload_state(0, w)
    done, reason = ens.step_until(66000, check_every=1000, stop_mask=STOP_EXTINCT | STOP_STILL)
    st = ens.stats()
    print("steps_done", done.tolist(), "reason", reason.tolist(), "launches", st.kernel_launches, "gpu_ms", st.gpu_ms)
    assert st.kernel_launches == 2
    assert (done[1], reason[1]) == (1000, STOP_EXTINCT | STOP_STILL)  # empty since step 1: at the first check point it is both
    assert done[0] == 66000 or reason[0] != 0
    recs = ens.summaries()
    assert recs[1].population == 0 and recs[1].step == 1000
    with Engine(0) as lone:
        lone.configure(G)
        lone.set_rule_strings(born="2,4", survive="1,3,5")
        lone.upload_state(w[0])
        lone.step(int(done[0]))
        one = lone.summary()
        one.plane_population = None
        assert recs[0] == one
        np.testing.assert_array_equal(ens.read_state(0, 1)[0], lone.read_state())
    # plain stepping in two launches
    ens.upload_state(0, w)
    ens.step(65536 + 3)
    assert ens.stats().kernel_launches == 2
    assert [s.step for s in ens.summaries()] == [65539, 65539]


def test_refusals(ens):
    lib = _capi.load()
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_strings(0)
    assert e.value.code == -2  # not configured
    for g in (32, 128):
        with pytest.raises(Ca3dError) as e:
            ens.configure(4, grid_size=g)
        assert e.value.code == -5
    ens.configure(4)
    with pytest.raises(Ca3dError) as e:
        ens.step(1)
    assert e.value.code == -2  # no rules
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_strings(2, neighbourhood="moore", born="4", survive="4")
    assert e.value.code == -5 and "universe 2" in e.value.message
    with pytest.raises(Ca3dError) as e:  # clustered: edges / corners tables that fire
        ens.set_rule_strings(1, born="2", survive="1-3", born_edges="3-4", survive_edges="2")
    assert e.value.code == -5 and "universe 1" in e.value.message
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_strings(4)
    assert e.value.code == -1
    ens.set_rule_strings(_capi.ENSEMBLE_ALL)
    with pytest.raises(Ca3dError) as e:
        ens.step(1)
    assert e.value.code == -2  # nothing uploaded
    ens.upload_state(0, np.zeros((3, W), dtype=np.uint32))
    with pytest.raises(Ca3dError) as e:
        ens.step_until(4)
    assert e.value.code == -2  # universe 3 has no state
    with pytest.raises(Ca3dError) as e:
        ens.read_state()
    assert e.value.code == -2
    with pytest.raises(Ca3dError) as e:
        ens.upload_state(3, np.zeros((2, W), dtype=np.uint32))
    assert e.value.code == -1  # past the end
    ens.upload_state(3, np.zeros(W, dtype=np.uint32))
    ens.step(2)
    with pytest.raises(Ca3dError) as e:
        ens.step_until(4, check_every=0)
    assert e.value.code == -1
    with pytest.raises(Ca3dError) as e:
        ens.step_until(4, stop_mask=4)
    assert e.value.code == -1
    assert lib.ca3d_ensemble_step_until(ens._h, 0, 1, 3, None, None) == 0  # both arrays are nullable
    assert lib.ca3d_ensemble_summarize(ens._h, 0, 4, None) == -1
    assert [s.step for s in ens.summaries()] == [2, 2, 2, 2]
