"""Moore ensembles (ca3d_ensemble_configure_neighbourhood, ca_ensemble_moore64) on the GPU: many 64^3 universes in one launch, each with
its own 27 + 27 bit rule table pair, record and end. Expected values always come from CPU-oracle trajectories (oracle_lib.packed_step)
and the numpy definition of a summary (host.state_summary) — never from the engine, never hard-coded. Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host

pytestmark = pytest.mark.gpu

G, W = 64, 8192
STOP_EXTINCT, STOP_STILL = 1, 2
# born / survive over the Moore count (0 .. 26); universe u runs rule u % 10: the empty rule, survive-all, born "0", born "1" (explosive),
# a 4555-style and a 5766-style rule, one that uses counts 25 and 26, and three more
RULES = [("", ""), ("", "0-26"), ("0", "0-26"), ("1", ""), ("5", "4,5"), ("6", "5-7"), ("25,26", "24-26"), ("5-7", "4-6"), ("4", "3,4"),
         ("9-13,17", "8-20,26")]


def rule_of(u):
    b, s = RULES[u % 10]
    return ol.Rules.from_strings(neighbourhood="moore", born=b, survive=s)


# The oracle's Moore step counts 26 neighbours cell by cell and costs about a hundred of its von Neumann steps, so the numbered universes
# repeat with period 30 — ten rules x three densities, each with its own seed — and their trajectories are shared: neighbouring
# universes always differ, and an ensemble of up to 30 holds no two alike.
PERIOD = 30


def fill_of(u):
    return host.random_fill(W, seed=101 + u % PERIOD, and_rounds=(0, 2, 5)[u % 3])


_TRAJ = {}


def trajectory(key, first, rules, steps):
    """Oracle states 0 .. steps of one universe, computed once per module and extended on demand."""
    t = _TRAJ.setdefault(key, [first])
    while len(t) <= steps:
        t.append(ol.packed_step(G, t[-1], rules))
    return t


def universe(u, steps):
    return trajectory(("u", u % PERIOD), fill_of(u), rule_of(u), steps)


def make(ens, universes):
    """A Moore ensemble of the numbered universes: rule u % 10 and fill u each, set one by one, uploaded together."""
    ens.configure(len(universes), neighbourhood="moore")
    for k, u in enumerate(universes):
        b, s = RULES[u % 10]
        ens.set_rule_strings(k, neighbourhood="moore", born=b, survive=s)
    ens.upload_state(0, np.stack([fill_of(u) for u in universes]))


def mask_of(s):
    m = 0
    for v in host.rules_components_to_values(s):
        m |= 1 << v
    return m


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
    assert ens.neighbourhood == "moore"
    sample = list(range(B)) if B <= 300 else sorted((set(range(0, B, 8)) - {8, 16}) | {255, B - 1})
    assert len(sample) == min(B, 128) or B <= 300
    assert B <= 300 or {0, 255, 256, B - 1} <= set(sample)
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
    """Single cells on each face, each edge midpoint and all eight corners, and one universe holding them all: coordinate -1 is dead,
    coordinate 64 wraps to 0 — on every axis, and for a diagonal neighbour on each of its axes separately (dead across one, wrapped
    across another)."""
    faces = [(0, 20, 30), (63, 21, 31), (22, 0, 32), (23, 63, 33), (24, 34, 0), (25, 35, 63)]
    edges = [(x, y, 31) for x in (0, 63) for y in (0, 63)] + [(x, 32, z) for x in (0, 63) for z in (0, 63)] + [(33, y, z) for y in (0, 63) for z in (0, 63)]
    corners = [(x, y, z) for x in (0, 63) for y in (0, 63) for z in (0, 63)]
    cells = faces + edges + corners
    assert len(edges) == 12 and len(corners) == 8
    firsts = [host.cells_to_words(G, [c]) for c in cells] + [host.cells_to_words(G, cells)]
    ens.configure(len(firsts), neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="1", survive="")
    ens.upload_state(0, np.stack(firsts))
    r = ol.Rules.from_strings(neighbourhood="moore", born="1", survive="")
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
            for u in (0, 4, 7, 22):
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
    """Ten rules x seeds 1-3. By construction the empty rule dies out at the first check, survive "0-26" with born "" freezes alive, and
    born "1" (explosive) is still changing after max_steps; each universe stops (or not) where the oracle says, and stays there."""
    MAX = 24
    cases = [(r, seed) for r in range(10) for seed in (1, 2, 3)]
    firsts = [host.random_fill(W, seed=seed, and_rounds=(0, 2, 5)[seed - 1]) for _, seed in cases]
    ens.configure(len(cases), neighbourhood="moore")
    for k, (r, _) in enumerate(cases):
        ens.set_rule_strings(k, neighbourhood="moore", born=RULES[r][0], survive=RULES[r][1])
    ens.upload_state(0, np.stack(firsts))
    mask = STOP_EXTINCT | STOP_STILL
    trajs = [trajectory(("stop",) + c, w, ol.Rules.from_strings(neighbourhood="moore", born=RULES[c[0]][0], survive=RULES[c[0]][1]), MAX + 8)
             for c, w in zip(cases, firsts)]
    want = [expected_stop(t, 0, MAX, every, mask, False) for t in trajs]
    # the oracle shows all three outcomes: died out (seen a step late, an empty grid is still as well), froze alive, still changing
    assert any(w[1] & STOP_EXTINCT for w in want) and any(w[1] == STOP_STILL for w in want) and any(w == (MAX, 0) for w in want)
    assert want[0][1] & STOP_EXTINCT and want[3][1] == STOP_STILL and want[9] == (MAX, 0)  # rules 0, 1 and 3 with seed 1

    done, reason = ens.step_until(MAX, check_every=every, stop_mask=mask)
    print("steps_done", done.tolist(), "reason", reason.tolist())
    assert done.tolist() == [w[0] for w in want] and reason.tolist() == [w[1] for w in want]
    got = ens.read_state()
    recs = ens.summaries()
    for k, t in enumerate(trajs):
        d = int(done[k])
        np.testing.assert_array_equal(got[k], t[d], err_msg=f"case {cases[k]}: state after {d} steps")  # a stopped universe did not move on
        check(recs[k], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, f"case {cases[k]}")
    st = ens.stats()
    assert st.cell_steps == float(int(done.sum())) * G ** 3 and st.steps == MAX

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
    length, the dead universe leaves the later launches at once, and the survivor equals a lone engine stepped as often. Born "0" with
    no survivor cannot settle: an empty grid is followed by a full one and a full one by an empty one, and whatever else it holds
    changes every step."""
    from cellularautomatons3d_amd import Engine

    ens.configure(2, neighbourhood="moore")
    ens.set_rule_strings(0, neighbourhood="moore", born="0", survive="")
    ens.set_rule_strings(1, neighbourhood="moore", born="", survive="")
    w = np.stack([fill_of(0), fill_of(1)])
    ens.upload_state(0, w)
    done, reason = ens.step_until(66000, check_every=1000, stop_mask=STOP_EXTINCT | STOP_STILL)
    st = ens.stats()
    print("steps_done", done.tolist(), "reason", reason.tolist(), "launches", st.kernel_launches, "gpu_ms", st.gpu_ms)
    assert (done[1], reason[1]) == (1000, STOP_EXTINCT | STOP_STILL)  # empty since step 1: at the first check point it is both
    assert done[0] == 66000 or reason[0] != 0
    assert st.kernel_launches == 2
    recs = ens.summaries()
    assert recs[1].population == 0 and recs[1].step == 1000
    with Engine(0) as lone:
        lone.configure(G)
        lone.set_rule_strings(neighbourhood="moore", born="0", survive="")
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


def test_rule_tables_agree_with_rule_strings(ens):
    """set_rule_tables (27-bit masks) and set_rule_strings store the same rule: the same states after 8 steps, both the oracle's."""
    B = 20
    make(ens, range(B))
    ens.step(8)
    by_strings = ens.read_state()
    ens.configure(B, neighbourhood="moore")
    ens.set_rule_tables(0, [mask_of(RULES[u % 10][0]) for u in range(B)], [mask_of(RULES[u % 10][1]) for u in range(B)])
    ens.upload_state(0, np.stack([fill_of(u) for u in range(B)]))
    ens.step(8)
    by_tables = ens.read_state()
    for u in range(B):
        want = universe(u, 8)[8]
        np.testing.assert_array_equal(by_strings[u], want, err_msg=f"universe {u} by strings")
        np.testing.assert_array_equal(by_tables[u], want, err_msg=f"universe {u} by tables")
    # one pair for a range
    ens.set_rule_tables(4, mask_of("5-7"), mask_of("4-6"), count=2)
    ens.upload_state(0, np.stack([fill_of(u) for u in range(B)]))
    ens.step(2)
    r = ol.Rules.from_strings(neighbourhood="moore", born="5-7", survive="4-6")
    got = ens.read_state()
    for u in (4, 5):
        np.testing.assert_array_equal(got[u], trajectory(("pair", u), fill_of(u), r, 2)[2])
    np.testing.assert_array_equal(got[6], universe(6, 2)[2])


def test_refusals(ens):
    lib = _capi.load()
    nb = C.c_int(-1)
    assert lib.ca3d_ensemble_get_neighbourhood(ens._h, C.byref(nb)) == -2  # not configured
    with pytest.raises(Ca3dError) as e:
        ens.neighbourhood
    assert e.value.code == -2
    assert lib.ca3d_ensemble_configure_neighbourhood(ens._h, 64, 4, 2) == -1  # unknown neighbourhood
    assert lib.ca3d_ensemble_configure_neighbourhood(ens._h, 64, 4, -1) == -1
    with pytest.raises(ValueError):
        ens.configure(4, neighbourhood="edges")
    assert lib.ca3d_ensemble_get_neighbourhood(ens._h, C.byref(nb)) == -2  # a refused configure configures nothing
    for g in (32, 128):
        with pytest.raises(Ca3dError) as e:
            ens.configure(4, grid_size=g, neighbourhood="moore")
        assert e.value.code == -5
    ens.configure(4, neighbourhood="moore")
    assert ens.neighbourhood == "moore"
    with pytest.raises(Ca3dError) as e:  # a von Neumann payload in a Moore ensemble
        ens.set_rule_strings(2, born="1,3", survive="0-6")
    assert e.value.code == -5 and "universe 2" in e.value.message and "Moore" in e.value.message
    with pytest.raises(Ca3dError) as e:  # clustered: edges / corners tables that fire
        ens.set_rule_strings(1, neighbourhood="moore", born="5", survive="4,5", born_edges="3-4", survive_edges="2")
    assert e.value.code == -5 and "universe 1" in e.value.message
    with pytest.raises(Ca3dError) as e:  # bit 27
        ens.set_rule_tables(0, [1, 2, 1 << 27, 4], [0, 0, 0, 0])
    assert e.value.code == -1 and "universe 2" in e.value.message
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_tables(1, [1, 2], [0, 1 << 31])
    assert e.value.code == -1 and "universe 2" in e.value.message
    ens.set_rule_tables(0, (1 << 27) - 1, (1 << 27) - 1)  # all 27 bits are fine
    with pytest.raises(Ca3dError) as e:
        ens.step_until(4, stop_mask=4)
    assert e.value.code in (-1, -2)
    # the same handle: Moore -> von Neumann -> Moore, each stepping its own kind against the oracle
    w = np.stack([fill_of(u) for u in range(2)])
    for kind, b, s in (("von neumann", "2,4", "1,3,5"), ("moore", "5-7", "4-6"), ("von neumann", "1,3", "0-6"), ("moore", "6", "5-7")):
        ens.configure(2, neighbourhood=kind)
        assert ens.neighbourhood == kind
        assert lib.ca3d_ensemble_get_neighbourhood(ens._h, C.byref(nb)) == 0 and nb.value == (kind == "moore")
        with pytest.raises(Ca3dError) as e:
            ens.step(1)
        assert e.value.code == -2  # rules and states went with the old configuration
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood=kind, born=b, survive=s)
        other = "moore" if kind == "von neumann" else "von neumann"
        with pytest.raises(Ca3dError) as e:
            ens.set_rule_strings(1, neighbourhood=other, born="4", survive="4")
        assert e.value.code == -5 and "universe 1" in e.value.message
        ens.upload_state(0, w)
        ens.step(3)
        r = ol.Rules.from_strings(neighbourhood=kind, born=b, survive=s)
        got = ens.read_state()
        for u in range(2):
            np.testing.assert_array_equal(got[u], trajectory(("re", kind, b, u), w[u], r, 3)[3], err_msg=f"{kind} B{b}/S{s} universe {u}")
    ens.configure(4)  # the two-argument form stays von Neumann
    assert ens.neighbourhood == "von neumann"
    assert lib.ca3d_ensemble_configure(ens._h, 64, 4) == 0 and ens.neighbourhood == "von neumann"
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_tables(0, 1 << 7, 0)
    assert e.value.code == -1


def test_seeds(ens):
    """seed_states in a Moore ensemble: the host.seeded_state words and step-0 records, then steps from them."""
    B = 6
    ens.configure(B, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="5-7", survive="4-6")
    seeds, rounds, box = [11 + u for u in range(B)], [u % 3 for u in range(B)], ((8, 0, 5), (55, 63, 40))
    ens.seed_states(0, seeds, rounds, box=box)
    want = [host.seeded_state(G, seeds[u], rounds[u], box) for u in range(B)]
    got = ens.read_state()
    for u, s in enumerate(ens.summaries()):
        np.testing.assert_array_equal(got[u], want[u], err_msg=f"universe {u}")
        check(s, host.state_summary(G, want[u]), 0, f"universe {u} seeded")
    ens.step(2)
    r = ol.Rules.from_strings(neighbourhood="moore", born="5-7", survive="4-6")
    got = ens.read_state()
    for u, s in enumerate(ens.summaries()):
        t = trajectory(("seed", u), want[u], r, 2)
        np.testing.assert_array_equal(got[u], t[2], err_msg=f"universe {u} after 2 steps")
        check(s, host.state_summary(G, t[2], prev_words=t[1]), 2, f"universe {u} after 2 steps")
