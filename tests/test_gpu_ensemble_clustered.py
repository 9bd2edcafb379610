"""Clustered ensembles (ca3d_ensemble_configure_clustered, ca_ensemble_clustered64 / _cycle / _trace) on the GPU: many 64^3 universes in one
launch, each with three rule table pairs — main (Moore, 27 + 27 bits), edges (13 + 13), corners (9 + 9) — ORed. Expected values always
come from CPU-oracle trajectories (oracle_lib.packed_step) and the numpy definition of a summary (host.state_summary) — never from the
engine, never hard-coded. Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host

pytestmark = pytest.mark.gpu

G, W = 64, 8192
STOP_EXTINCT, STOP_STILL, STOP_PERIODIC = 1, 2, 4
KEYS = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")
# (born, survive, born_edges, survive_edges, born_corners, survive_corners); universe u runs rule u % 10 on fill u % 10:
# 0 bench.py's clustered rule; 1 only the edges pair fires; 2 only the corners pair fires; 3 plain Moore, the side strings the engine's
# silent default "27"; 4 - 7 start from the full grid and use the highest count of every class, together and one by one; 8 the empty
# rule; 9 survive "0-26" with nothing born
RULES = [("5-7", "4-7", "4", "3-5", "3", "2-4"), ("", "", "3,4", "2-4", "", ""), ("", "", "", "", "2,3", "1-3"), ("5-7", "4-6", "27", "27", "27", "27"),
         ("", "26", "", "12", "", "8"), ("", "26", "", "", "", ""), ("", "", "", "12", "", ""), ("", "", "", "", "", "8"),
         ("", "", "", "", "", ""), ("", "0-26", "", "", "", "")]
FULL = (4, 5, 6, 7)
BITS = (27, 13, 9)
# The oracle's clustered step costs about a quarter of a second, so the numbered universes repeat with period 10 and their trajectories
# are shared by every test of the module; none goes past 8 steps.
PERIOD = 10


def strings(rule):
    return dict(zip(KEYS, rule))


def rules_of(rule):
    return ol.Rules.from_strings(neighbourhood="moore", **strings(rule))


def fill_of(u):
    k = u % PERIOD
    if k in FULL:
        return np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    return host.random_fill(W, seed=101 + k, and_rounds=(0, 2, 5)[k % 3])


_TRAJ = {}


def trajectory(key, first, rules, steps):
    """Oracle states 0 .. steps of one universe, computed once per module and extended on demand."""
    assert steps <= 8
    t = _TRAJ.setdefault(key, [first])
    while len(t) <= steps:
        t.append(ol.packed_step(G, t[-1], rules))
    return t


def universe(u, steps):
    return trajectory(("u", u % PERIOD), fill_of(u), rules_of(RULES[u % PERIOD]), steps)


def make(ens, universes):
    """A clustered ensemble of the numbered universes: rule and fill u % 10 each, set one by one, uploaded together."""
    ens.configure(len(universes), neighbourhood="moore", clustered=True)
    for k, u in enumerate(universes):
        ens.set_rule_strings(k, neighbourhood="moore", **strings(RULES[u % PERIOD]))
    ens.upload_state(0, np.stack([fill_of(u) for u in universes]))


def mask_of(s, bits):
    m = 0
    for v in host.rules_components_to_values(s):
        m |= 1 << v
    return m & ((1 << bits) - 1)  # the strings' "27" is slot 26: no edges or corners count reaches it


def masks_of(rule):
    """([main, edges, corners] born, the same survive) of a rule's six strings."""
    return [mask_of(rule[2 * i], BITS[i]) for i in range(3)], [mask_of(rule[2 * i + 1], BITS[i]) for i in range(3)]


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


@pytest.mark.parametrize("B", [1, 3, 300])
def test_parity_with_the_oracle(ens, B):
    """The checked universes after step(1), step(2), step(5) equal the oracle after 1, 3, 8 steps. 300: more workgroups than CUs; the
    first 20 universes (every rule twice) and 255, 256, 299 are compared."""
    make(ens, range(B))
    assert ens.clustered and ens.neighbourhood == "moore"
    sample = list(range(min(B, 20))) + ([255, 256, 299] if B == 300 else [])
    done = 0
    for n in (1, 2, 5):
        ens.step(n)
        done += n
        got = ens.read_state()
        assert got.shape == (B, W)
        for u in sample:
            np.testing.assert_array_equal(got[u], universe(u, done)[done], err_msg=f"B={B} universe {u} (rule {RULES[u % PERIOD]}) after {done} steps")
    st = ens.stats()
    assert st.steps == 5 and st.kernel_launches == 1 and st.cell_steps == 5.0 * B * G ** 3 and st.gpu_ms > 0
    if B == 300:
        # the rules do what they are here for: bench.py's rule lives on, the one-class rules fire, and the full-grid rules erode the - faces
        assert universe(0, 8)[8].any() and universe(1, 1)[1].any() and universe(2, 1)[1].any()
        for u in FULL:
            assert int(host.state_summary(G, universe(u, 1)[1])["population"]) == 63 ** 3


def test_classes_are_counted_apart(ens):
    """A lone interior cell under born "1" of one rule-set: 26, 12 and 8 cells after one step — the Moore shell, its edge cells, its
    corner cells."""
    first = host.cells_to_words(G, [(20, 30, 40)])
    rules = [("1", "", "", "", "", ""), ("", "", "1", "", "", ""), ("", "", "", "", "1", "")]
    ens.configure(3, neighbourhood="moore", clustered=True)
    for k, r in enumerate(rules):
        ens.set_rule_strings(k, neighbourhood="moore", **strings(r))
    ens.upload_state(0, np.stack([first] * 3))
    ens.step(1)
    got = ens.read_state()
    recs = ens.summaries()
    for k, (r, n) in enumerate(zip(rules, (26, 12, 8))):
        want = trajectory(("class", k), first, rules_of(r), 1)[1]
        assert int(host.state_summary(G, want)["population"]) == n  # the oracle agrees with the definition
        np.testing.assert_array_equal(got[k], want, err_msg=f"rule {r}")
        assert recs[k].population == n


def test_boundary_asymmetry(ens):
    """One universe with a cell on each face, each edge midpoint and each corner, and six single-cell universes — a face, an edge and a
    corner cell on the - side and on the + side — under born "1" in all three rule-sets: coordinate -1 is dead, coordinate 64 wraps to 0,
    on every axis separately (a diagonal neighbour can be dead across one axis and wrapped across another)."""
    faces = [(0, 20, 30), (63, 21, 31), (22, 0, 32), (23, 63, 33), (24, 34, 0), (25, 35, 63)]
    edges = [(x, y, 31) for x in (0, 63) for y in (0, 63)] + [(x, 32, z) for x in (0, 63) for z in (0, 63)] + [(33, y, z) for y in (0, 63) for z in (0, 63)]
    corners = [(x, y, z) for x in (0, 63) for y in (0, 63) for z in (0, 63)]
    assert len(edges) == 12 and len(corners) == 8
    singles = [(0, 20, 30), (63, 21, 31), (0, 0, 31), (63, 63, 31), (0, 0, 0), (63, 63, 63)]
    firsts = [host.cells_to_words(G, faces + edges + corners)] + [host.cells_to_words(G, [c]) for c in singles]
    rule = ("1", "", "1", "", "1", "")
    ens.configure(len(firsts), neighbourhood="moore", clustered=True)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", **strings(rule))
    ens.upload_state(0, np.stack(firsts))
    r = rules_of(rule)
    for done in (1, 2, 3):
        ens.step(1)
        got = ens.read_state()
        for k, w in enumerate(firsts):
            np.testing.assert_array_equal(got[k], trajectory(("face", k), w, r, done)[done], err_msg=f"universe {k} after {done} steps")


def test_records_equal_the_definition_and_a_lone_engine(ens):
    from cellularautomatons3d_amd import Engine

    B = 10
    make(ens, range(B))
    for u, s in enumerate(ens.summaries()):
        check(s, host.state_summary(G, universe(u, 0)[0]), 0, f"universe {u} after upload")
    done = 0
    with Engine(0) as lone:
        lone.configure(G)
        for n in (1, 4):
            ens.step(n)
            done += n
            recs = ens.summaries()
            for u, s in enumerate(recs):
                t = universe(u, done)
                check(s, host.state_summary(G, t[done], prev_words=t[done - 1]), done, f"universe {u} after {done} steps")
            for u in (0, 1, 2, 4):
                r = rules_of(RULES[u])
                lone.set_rules(r.main, r.edges, r.corners, r.survive, r.born)
                lone.upload_state(fill_of(u))
                lone.step(done)
                one = lone.summary()
                one.plane_population = None
                assert recs[u] == one, f"universe {u} after {done} steps"
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
    """The empty rule dies out, survive "0-26" with nothing born stands still, bench.py's clustered rule goes on; every universe stops
    (or not) where its oracle trajectory says, and stays there."""
    MAX, AGAIN = 6, 2
    us = [8, 9, 0, 1, 2, 3, 4]
    make(ens, us)
    mask = STOP_EXTINCT | STOP_STILL
    trajs = [universe(u, MAX + AGAIN) for u in us]
    want = [expected_stop(t, 0, MAX, every, mask, False) for t in trajs]
    assert want[0][1] & STOP_EXTINCT and want[1][1] == STOP_STILL and want[2] == (MAX, 0)
    done, reason = ens.step_until(MAX, check_every=every, stop_mask=mask)
    print("steps_done", done.tolist(), "reason", reason.tolist())
    assert done.tolist() == [w[0] for w in want] and reason.tolist() == [w[1] for w in want]
    got = ens.read_state()
    recs = ens.summaries()
    for k, t in enumerate(trajs):
        d = int(done[k])
        np.testing.assert_array_equal(got[k], t[d], err_msg=f"universe {us[k]}: state after {d} steps")  # a stopped universe did not move on
        check(recs[k], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, f"universe {us[k]}")
    st = ens.stats()
    assert st.cell_steps == float(int(done.sum())) * G ** 3 and st.steps == MAX
    # again: whoever still satisfies a condition takes no step, the others take theirs
    done2, reason2 = ens.step_until(AGAIN, check_every=every, stop_mask=mask)
    want2 = [expected_stop(t, int(d), AGAIN, every, mask, d > 0) for t, d in zip(trajs, done)]
    assert done2.tolist() == [w[0] for w in want2] and reason2.tolist() == [w[1] for w in want2]
    got = ens.read_state()
    for k, t in enumerate(trajs):
        np.testing.assert_array_equal(got[k], t[int(done[k]) + int(done2[k])])


def expected_cycle(t, max_steps, every, mask):
    """(steps_done, reason, period) of a step_until_cycle from state t[0] after an upload: the definition of include/ca3d.h."""
    k = j = anchor = 0
    while True:
        cur = t[k]
        fired = 0
        if not cur.any():
            fired |= STOP_EXTINCT
        if k > 0 and np.array_equal(cur, t[k - 1]):
            fired |= STOP_STILL
        if j > 0 and np.array_equal(cur, t[anchor]):
            fired |= STOP_PERIODIC
        fired &= mask
        if fired or k == max_steps:
            return k, fired, (k - anchor if fired & STOP_PERIODIC else 0)
        if j > 0 and j & (j - 1) == 0:  # j = 1, 2, 4, 8, ...: the anchor moves AFTER the comparison
            anchor = k
        k += min(every, max_steps - k)
        j += 1


def test_cycle(ens):
    """Main tables silent, corners born "0", no survive table: an empty grid is followed by a full one and a full one by an empty one.
    From the full grid and from a sparse fill; the third universe (bench.py's clustered rule) does not cycle within the call."""
    rule = ("", "", "", "", "0", "")
    firsts = [np.full(W, 0xFFFFFFFF, dtype=np.uint32), host.random_fill(W, seed=7, and_rounds=5), fill_of(0)]
    ens.configure(3, neighbourhood="moore", clustered=True)
    for k in (0, 1):
        ens.set_rule_strings(k, neighbourhood="moore", **strings(rule))
    ens.set_rule_strings(2, neighbourhood="moore", **strings(RULES[0]))
    ens.upload_state(0, np.stack(firsts))
    MAX = 8
    trajs = [trajectory(("cycle", k), firsts[k], rules_of(rule), MAX) for k in (0, 1)] + [universe(0, MAX)]
    assert not trajs[0][1].any() and np.array_equal(trajs[0][2], firsts[0])  # empty, then full again
    want = [expected_cycle(t, MAX, 1, STOP_PERIODIC) for t in trajs]
    assert want[0][1:] == (STOP_PERIODIC, 2) and want[2] == (MAX, 0, 0)
    done, reason, period = ens.step_until_cycle(MAX, check_every=1, stop_mask=STOP_PERIODIC)
    print("steps_done", done.tolist(), "reason", reason.tolist(), "period", period.tolist())
    assert list(zip(done.tolist(), reason.tolist(), period.tolist())) == want
    got = ens.read_state()
    for k, t in enumerate(trajs):
        np.testing.assert_array_equal(got[k], t[int(done[k])], err_msg=f"universe {k}")


def test_trace(ens):
    """step_trace(8, check_every=2) on three universes: sample j is the population (births, deaths) of the oracle's state 2 j."""
    us = [0, 1, 9]
    make(ens, us)
    samples, count, done, reason = ens.step_trace(8, check_every=2)
    assert samples.shape == (3, 5, 3) and count.tolist() == [5] * 3 and done.tolist() == [8] * 3 and not reason.any()
    for k, u in enumerate(us):
        t = universe(u, 8)
        for j in range(5):
            d = host.state_summary(G, t[2 * j], prev_words=t[2 * j - 1] if j else None)
            assert samples[k, j].tolist() == [int(d["population"]), int(d["births"]), int(d["deaths"])], f"universe {u} sample {j}"
    np.testing.assert_array_equal(ens.read_state()[0], universe(0, 8)[8])


def test_tables_agree_with_strings(ens):
    """set_clustered_tables and set_rule_strings store the same rule: the same states after 2 steps, both the oracle's. The plain
    set_rule_tables sets the main pair and silences the sides."""
    B = 10
    make(ens, range(B))
    ens.step(2)
    by_strings = ens.read_state()
    ens.configure(B, neighbourhood="moore", clustered=True)
    pairs = [masks_of(RULES[u]) for u in range(B)]
    ens.set_clustered_tables(0, [p[0] for p in pairs], [p[1] for p in pairs])
    ens.upload_state(0, np.stack([fill_of(u) for u in range(B)]))
    ens.step(2)
    by_tables = ens.read_state()
    for u in range(B):
        want = universe(u, 2)[2]
        np.testing.assert_array_equal(by_strings[u], want, err_msg=f"universe {u} by strings")
        np.testing.assert_array_equal(by_tables[u], want, err_msg=f"universe {u} by tables")
    # one rule for a range; then the main pair alone over a clustered rule: universe 0 becomes universe 3's plain Moore rule
    b, s = masks_of(RULES[1])
    ens.set_clustered_tables(4, b, s, count=2)
    ens.set_rule_tables(0, mask_of("5-7", 27), mask_of("4-6", 27), count=1)
    fills = [fill_of(u) for u in range(B)]
    fills[0], fills[4], fills[5] = fill_of(3), fill_of(1), fill_of(1)
    ens.upload_state(0, np.stack(fills))
    ens.step(2)
    got = ens.read_state()
    np.testing.assert_array_equal(got[0], universe(3, 2)[2])
    np.testing.assert_array_equal(got[4], universe(1, 2)[2])
    np.testing.assert_array_equal(got[5], universe(1, 2)[2])
    np.testing.assert_array_equal(got[6], universe(6, 2)[2])


def test_refusals(ens):
    lib = _capi.load()
    out = C.c_int(-1)
    assert lib.ca3d_ensemble_get_clustered(ens._h, C.byref(out)) == -2 and out.value == -1  # not configured
    with pytest.raises(Ca3dError) as e:
        ens.clustered
    assert e.value.code == -2
    with pytest.raises(ValueError):
        ens.configure(4, neighbourhood="von neumann", clustered=True)
    with pytest.raises(ValueError):
        ens.configure(4, clustered=True)
    for g in (32, 128):
        with pytest.raises(Ca3dError) as e:
            ens.configure(4, grid_size=g, neighbourhood="moore", clustered=True)
        assert e.value.code == -5
    assert lib.ca3d_ensemble_get_clustered(ens._h, C.byref(out)) == -2  # a refused configure configures nothing
    ens.configure(4, neighbourhood="moore", clustered=True)
    one = [1, 1, 1]
    for word, bits in enumerate(BITS):
        bad = [[1, 1, 1] for _ in range(4)]
        bad[2][word] = 1 << bits
        with pytest.raises(Ca3dError) as e:
            ens.set_clustered_tables(0, bad, [one] * 4)
        assert e.value.code == -1 and "universe 2" in e.value.message
        with pytest.raises(Ca3dError) as e:
            ens.set_clustered_tables(1, [one] * 2, bad[1:3])
        assert e.value.code == -1 and "universe 2" in e.value.message
    ens.set_clustered_tables(0, [(1 << 27) - 1, (1 << 13) - 1, (1 << 9) - 1], [(1 << 27) - 1, (1 << 13) - 1, (1 << 9) - 1])  # every bit is fine
    three = (C.c_uint32 * 9)(*([1] * 9))
    assert lib.ca3d_ensemble_set_rule_tables_clustered(ens._h, 0, 4, three, three, 3) == -1  # n_rules neither 1 nor count
    assert lib.ca3d_ensemble_set_rule_tables_clustered(ens._h, 0, 4, three, three, 0) == -1
    with pytest.raises(Ca3dError) as e:  # a von Neumann payload in a clustered ensemble
        ens.set_rule_strings(2, born="1,3", survive="0-6")
    assert e.value.code == -5 and "universe 2" in e.value.message
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_strings(1, neighbourhood="moore 2D", born="3", survive="2,3")
    assert e.value.code == -5 and "universe 1" in e.value.message
    ens.configure(4, neighbourhood="moore")
    assert not ens.clustered
    with pytest.raises(Ca3dError) as e:  # three pairs in a Moore ensemble
        ens.set_clustered_tables(0, one, one)
    assert e.value.code == -5


def test_reconfiguration(ens):
    """One handle: Moore -> clustered -> von Neumann -> clustered, each kind stepping its own rules against the oracle for 2 steps."""
    vn = [("2,4", "1,3,5"), ("1,3", "0-6")]
    for nb, clustered, us in (("moore", False, (3, 9)), ("moore", True, (0, 1)), ("von neumann", False, None), ("moore", True, (2, 4))):
        ens.configure(2, neighbourhood=nb, clustered=clustered)
        assert ens.neighbourhood == nb and ens.clustered is clustered
        with pytest.raises(Ca3dError) as e:
            ens.step(1)
        assert e.value.code == -2  # rules and states went with the old configuration
        if us is None:
            w = [fill_of(0), fill_of(1)]
            for k, (b, s) in enumerate(vn):
                ens.set_rule_strings(k, born=b, survive=s)
            want = [trajectory(("vn", k), w[k], ol.Rules.from_strings(born=b, survive=s), 2)[2] for k, (b, s) in enumerate(vn)]
        else:
            w = [fill_of(u) for u in us]
            for k, u in enumerate(us):
                ens.set_rule_strings(k, neighbourhood="moore", **strings(RULES[u]))
            want = [universe(u, 2)[2] for u in us]
        ens.upload_state(0, np.stack(w))
        ens.step(2)
        got = ens.read_state()
        for k in range(2):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{nb} clustered={clustered} universe {k}")


def test_seeds(ens):
    """seed_states in a clustered ensemble, then one step from the host.seeded_state words."""
    B = 3
    ens.configure(B, neighbourhood="moore", clustered=True)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", **strings(RULES[0]))
    seeds, rounds, box = [11 + u for u in range(B)], [u % 3 for u in range(B)], ((8, 0, 5), (55, 63, 40))
    ens.seed_states(0, seeds, rounds, box=box)
    want = [host.seeded_state(G, seeds[u], rounds[u], box) for u in range(B)]
    got = ens.read_state()
    for u, s in enumerate(ens.summaries()):
        np.testing.assert_array_equal(got[u], want[u], err_msg=f"universe {u}")
        check(s, host.state_summary(G, want[u]), 0, f"universe {u} seeded")
    ens.step(1)
    r = rules_of(RULES[0])
    got = ens.read_state()
    for u, s in enumerate(ens.summaries()):
        t = trajectory(("seed", u), want[u], r, 1)
        np.testing.assert_array_equal(got[u], t[1], err_msg=f"universe {u} after 1 step")
        check(s, host.state_summary(G, t[1], prev_words=t[0]), 1, f"universe {u} after 1 step")
