"""Rule tables bit by bit, on states that reach every count: the ensemble kernels of ca_ensemble.hip (plain, _cycle, _moving, _trace), the
engine's pre-built table and generic kernels and the run-time compiled ones, under the one-hot and coded rule families of graded_lib on
graded states (density 0 .. 1 along one axis, so that every (alive, count) pair of every table occurs; test_graded_cpu.py shows it).
Expected states always come from CPU-oracle steps (oracle_lib.packed_step), computed once per module; records and trace samples from the
numpy definition of a summary (host.state_summary). graded_lib.class_counts serves the coverage asserts and the wording of a failure only.
Every comparison is exact, and a failure names kind, table, bit and orientation."""
import numpy as np
import pytest

import graded_lib as gl
from cellularautomatons3d_amd import host
from rule_tables_common import differs, engine_case, first_state, form, label, settle, trajectory

pytestmark = pytest.mark.gpu

G, W = 64, 8192
CELLS = G ** 3
EXTINCT, STILL, PERIODIC, MOVING = 1, 2, 4, 8
NB = {"vn": "von neumann", "moore": "moore"}
KINDS = ["vn", "moore", "main", "edges", "corners"]  # graded_lib.TABLES: the last three are the classes of a clustered rule, one firing


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def make(ens, kind, rules, firsts, by="tables"):
    """An ensemble of len(rules) universes of a table kind: universe i runs rules[i] from the start state named firsts[i]."""
    k = form(kind, rules[0])[0]
    if k == "clustered":
        triples = [form(kind, r)[1] for r in rules]
        ens.configure(len(rules), neighbourhood="moore", clustered=True)
        if by == "tables":
            ens.set_clustered_tables(0, [[c.born for c in t] for t in triples], [[c.survive for c in t] for t in triples])
        else:
            for i, t in enumerate(triples):
                ens.set_rule_strings(i, **gl.strings_of("clustered", t))
        assert ens.clustered
    else:
        assert by == "tables"
        ens.configure(len(rules), neighbourhood=NB[kind])
        ens.set_rule_tables(0, [r.born for r in rules], [r.survive for r in rules])
    ens.upload_state(0, np.stack([first_state(G, n) for n in firsts]))


def check_record(s, want, step, where):
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


def check_states(ens, kind, rules, firsts, trajs, done):
    """States and records after a call against the oracle's at steps_done."""
    state, recs = ens.read_state(), ens.summaries()
    wheres = [f"{label(kind, rules[i], firsts[i])}, after {int(done[i])} steps" for i in range(len(trajs))]
    settle(differs(G, state[i], t[int(done[i])], t[max(int(done[i]) - 1, 0)], wheres[i]) for i, t in enumerate(trajs))
    for i, t in enumerate(trajs):
        d = int(done[i])
        check_record(recs[i], host.state_summary(G, t[d], prev_words=t[d - 1] if d else None), d, wheres[i])


def test_the_graded_states_hold_every_count():
    """What the sweeps below rest on, from class_counts alone: every (alive, count) pair of every table at least 32 times, in every
    orientation and at both engine grids."""
    for g in (64, 128):
        for name in gl.ORIENTATIONS:
            for key, v in gl.coverage(g, first_state(g, name)).items():
                assert v.min() >= 32, (g, name, key, v.min())


# ------------------------------------------------------------------------------------------------ ensembles, plain kernels

@pytest.mark.parametrize("kind,by", [(k, "tables") for k in KINDS] + [(k, "strings") for k in gl.CLASSES])
def test_one_hot_tables_in_an_ensemble(ens, kind, by):
    """One launch, one step: every universe holds the z-graded state, universe i runs one-hot rule i (B = 14 / 54 / 54, 26, 18). A leaf of
    the multiplexer tree that reads the wrong table bit, or the wrong word of the clustered record, answers for another count."""
    rules = gl.one_hot(gl.TABLES[kind])
    firsts = ["z"] * len(rules)
    assert len(rules) == {"vn": 14, "moore": 54, "main": 54, "edges": 26, "corners": 18}[kind]
    make(ens, kind, rules, firsts, by)
    ens.step(1)
    got = ens.read_state()
    assert ens.stats().kernel_launches == 1
    lines = []
    for i, r in enumerate(rules):
        t = trajectory(G, "z", kind, r, 1)
        assert t[1].any()  # the bit decides something: the count occurs, alive and dead
        lines.append(differs(G, got[i], t[1], t[0], f"{label(kind, r, 'z')} (set by {by})"))
    settle(lines)


@pytest.mark.parametrize("kind", KINDS)
def test_coded_tables_on_the_other_orientations(ens, kind):
    """The coded rules on the y-, x- and reversed z-graded states, B = 3 x 2 ceil(log2 N): dense content meets each + face (which wraps)
    and, reversed, the dead - face."""
    fam = gl.coded(gl.TABLES[kind])
    cases = [(r, n) for n in ("y", "x", "zr") for r in fam]
    rules, firsts = [c[0] for c in cases], [c[1] for c in cases]
    make(ens, kind, rules, firsts)
    ens.step(1)
    got = ens.read_state()
    lines = []
    for i, (r, n) in enumerate(cases):
        t = trajectory(G, n, kind, r, 1)
        lines.append(differs(G, got[i], t[1], t[0], label(kind, r, n)))
    settle(lines)


def test_all_three_classes_coded_at_once(ens):
    """Clustered, class s running coded rule (j + s) mod its family size: the final three-way OR with all inputs varying."""
    cases = [(gl.coded_all(j), n) for n in gl.ORIENTATIONS for j in range(10)]
    rules, firsts = [c[0] for c in cases], [c[1] for c in cases]
    make(ens, "all", rules, firsts)
    ens.step(1)
    got = ens.read_state()
    lines = []
    for i, (r, n) in enumerate(cases):
        t = trajectory(G, n, "all", r, 1)
        lines.append(differs(G, got[i], t[1], t[0], label("all", r, n)))
    settle(lines)


# ------------------------------------------------------------------------------------------------ ensembles, the other instantiations

MAX, EVERY = 2, 1


def expected_watch(t, max_steps, every, mask):
    """(steps_done, reason, period, shift) of a step_until_cycle / step_until_moving from state t[0] after an upload: the definition of
    include/ca3d.h (test_gpu_cycle.py's and test_gpu_moving.py's restatement; the translation test is host.moved_by)."""
    k = j = anchor = 0
    while True:
        cur = t[k]
        fired, d = 0, None
        if not cur.any():
            fired |= EXTINCT
        if k > 0 and np.array_equal(cur, t[k - 1]):
            fired |= STILL
        if j > 0 and np.array_equal(cur, t[anchor]):
            fired |= PERIODIC
        if j > 0 and mask & MOVING:
            d = host.moved_by(G, t[anchor], cur)
            if d is not None:
                fired |= MOVING
        fired &= mask
        if fired or k == max_steps:
            return k, fired, (k - anchor if fired & (PERIODIC | MOVING) else 0), (tuple(d) if fired & MOVING else (0, 0, 0))
        if j > 0 and j & (j - 1) == 0:  # j = 1, 2, 4, 8, ...: the anchor moves AFTER the comparison
            anchor = k
        k += min(every, max_steps - k)
        j += 1


def expected_trace(t, max_steps, every, mask):
    """(samples [K][3], n_samples, steps_done, reason) of a traced call from state t[0] after an upload (test_gpu_trace.py's restatement)."""
    samples = np.zeros((host.trace_samples(max_steps, every), 3), dtype=np.uint32)
    k = j = 0
    while True:
        s = host.state_summary(G, t[k], prev_words=t[k - 1] if k else None)
        samples[j] = (s["population"], s["births"], s["deaths"])
        fired = 0
        if not t[k].any():
            fired |= EXTINCT
        if k > 0 and np.array_equal(t[k], t[k - 1]):
            fired |= STILL
        fired &= mask
        if fired or k == max_steps:
            return samples, j + 1, k, fired
        k += min(every, max_steps - k)
        j += 1


def coded_universes(kind):
    """(rules, firsts, trajectories) of the coded rules of a kind on the z- and x-graded states."""
    cases = [(r, n) for n in ("z", "x") for r in gl.coded(gl.TABLES[kind])]
    rules, firsts = [c[0] for c in cases], [c[1] for c in cases]
    return rules, firsts, [trajectory(G, n, kind, r, MAX) for r, n in cases]


@pytest.mark.parametrize("kind", KINDS)
def test_coded_tables_through_the_cycle_kernels(ens, kind):
    rules, firsts, trajs = coded_universes(kind)
    make(ens, kind, rules, firsts)
    want = [expected_watch(t, MAX, EVERY, PERIODIC) for t in trajs]
    done, reason, period = ens.step_until_cycle(MAX, check_every=EVERY, stop_mask=PERIODIC)
    assert list(zip(done.tolist(), reason.tolist(), period.tolist())) == [w[:3] for w in want]
    check_states(ens, kind, rules, firsts, trajs, done)


@pytest.mark.parametrize("kind", KINDS)
def test_coded_tables_through_the_moving_kernels(ens, kind):
    rules, firsts, trajs = coded_universes(kind)
    make(ens, kind, rules, firsts)
    want = [expected_watch(t, MAX, EVERY, MOVING) for t in trajs]
    done, reason, period, shift = ens.step_until_moving(MAX, check_every=EVERY, stop_mask=MOVING)
    got = [(int(d), int(r), int(p), tuple(int(v) for v in s)) for d, r, p, s in zip(done, reason, period, shift)]
    assert got == want
    check_states(ens, kind, rules, firsts, trajs, done)


@pytest.mark.parametrize("kind", KINDS)
def test_coded_tables_through_the_trace_kernels(ens, kind):
    """The coded universes and two that flip completely — the full grid under the empty rule (262 144 deaths in one sample, then extinct
    and still) and the empty grid under born "0" (262 144 births, then as many deaths): a wave's births | deaths << 16 word at its
    largest, 16 384 each. Stop mask 0: every check point is sampled."""
    rules, firsts, trajs = coded_universes(kind)
    N = gl.TABLES[kind]
    empty_rule, born0 = gl.SILENT, gl.one_hot(N)[0]
    rules, firsts = rules + [empty_rule, born0], firsts + ["full", "empty"]
    trajs = trajs + [trajectory(G, "full", kind, empty_rule, MAX), trajectory(G, "empty", kind, born0, MAX)]
    make(ens, kind, rules, firsts)
    want = [expected_trace(t, MAX, EVERY, 0) for t in trajs]
    assert want[-2][0].tolist() == [[CELLS, 0, 0], [0, 0, CELLS], [0, 0, 0]]
    assert want[-1][0].tolist() == [[0, 0, 0], [CELLS, CELLS, 0], [0, 0, CELLS]]
    samples, count, done, reason = ens.step_trace(MAX, check_every=EVERY, stop_mask=0)
    assert samples.shape == (len(rules), 3, 3)
    for i, (ws, wn, wd, wr) in enumerate(want):
        where = label(kind, rules[i], firsts[i])
        assert (int(count[i]), int(done[i]), int(reason[i])) == (wn, wd, wr) == (3, MAX, 0), where
        np.testing.assert_array_equal(samples[i], ws, err_msg=where)
    check_states(ens, kind, rules, firsts, trajs, done)


# ------------------------------------------------------------------------------------------------ engine

MODES = [(1, 0), (0, 0), (0, 1)]  # (jit, variant): compiled for the rule at run time; the pre-built table kernels; the generic kernel


@pytest.fixture(scope="module")
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def restore(eng):
    eng.set_option("jit", 1)
    eng.set_option("variant", 0)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kind", ["moore", "edges", "corners"])
def test_one_hot_tables_in_the_engine(eng, kind, variant):
    """The kernels that take the rule as data (jit 0) compile nothing: every one-hot rule of the Moore, edges and corners tables."""
    eng.configure(G)
    try:
        settle(m for r in gl.one_hot(gl.TABLES[kind]) for m in engine_case(eng, G, kind, r, "z", [(0, variant)]))
    finally:
        restore(eng)


@pytest.mark.parametrize("name", list(gl.ORIENTATIONS))
@pytest.mark.parametrize("kind", KINDS + ["all"])
def test_coded_tables_in_the_engine(eng, kind, name):
    eng.configure(G)
    rules = [gl.coded_all(j) for j in range(10)] if kind == "all" else gl.coded(gl.TABLES[kind])
    try:
        settle(m for r in rules for m in engine_case(eng, G, kind, r, name, MODES))
    finally:
        restore(eng)


@pytest.mark.parametrize("kind,j", [("moore", j) for j in range(10)] + [("all", j) for j in range(6)])
def test_coded_tables_in_the_engine_at_128(eng, kind, j):
    """The ten Moore coded rules and six clustered combinations on the z-graded 128^3 state."""
    eng.configure(128)
    rule = gl.coded(27)[j] if kind == "moore" else gl.coded_all(j)
    try:
        settle(engine_case(eng, 128, kind, rule, "z", MODES))
    finally:
        restore(eng)
