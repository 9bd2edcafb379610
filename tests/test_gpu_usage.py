"""`ca3d_ensemble_usage` on the GPU (the nine kernels of csrc/ca_usage.hip) against `host.usage`, the numpy restatement of the
definition in include/ca3d.h, fed with CPU trajectories (chains of `host.ensemble_step`, which tests/test_ensemble_boundary_cpu.py pins
to the CPU oracle): every field of every record, and the record's bytes, exactly. tests/test_usage_cpu.py checks `host.usage` itself
against histograms that do not go through it. Universes are 64^3 by construction."""
import ctypes as C
import re

import numpy as np
import pytest

import graded_lib as gl
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_ensemble_boundary_cpu import grow_rule, rule_of, tables_of
from test_gpu_envelope import hold, make_ensemble, snapshot

pytestmark = pytest.mark.gpu

G, W, CELLS = 64, 8192, 64 ** 3
KINDS = ("von neumann", "moore", "clustered")
BOUNDARIES = host.ENSEMBLE_BOUNDARIES
FULL, EMPTY = np.full(W, 0xFFFFFFFF, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
# the corners, both sides of the word seam of a row (x = 31 | 32), the first and last row (y: the ends of a wave's DPP shifts), both
# sides of the seam between two waves' planes (z = 3 | 4, 59 | 60)
LONE = ((0, 0, 0), (63, 63, 63), (31, 20, 9), (32, 20, 9), (21, 0, 42), (21, 63, 42), (21, 30, 3), (21, 30, 4), (21, 30, 59), (21, 30, 60))


@pytest.fixture()
def ens():
    e = make_ensemble()
    yield e
    e.close()


@pytest.fixture()
def nursery():
    e = make_ensemble()
    yield e
    e.close()


@pytest.fixture(scope="module")
def graded():
    return [gl.graded_state(G, axis, reverse) for axis, reverse in gl.ORIENTATIONS.values()]


def everything(kind):
    """(born nowhere, survive everywhere): FULL stays full, EMPTY stays empty."""
    return ((0, 0, 0), ((1 << 27) - 1, (1 << 13) - 1, (1 << 9) - 1)) if kind == "clustered" else (0, (1 << 27) - 1 if kind != "von neumann" else 0x7F)


_CHAINS, _WANT = {}, {}


def phases(key, state, kind, tables, boundary, p):
    """S_0 .. S_(p-1) of `state` under host.ensemble_step, kept for the run under (key, kind, boundary): `key` names state and rule."""
    t = _CHAINS.setdefault((key, kind, boundary), [np.ascontiguousarray(state, dtype=np.uint32)])
    assert np.array_equal(t[0], state)
    while len(t) < p:
        t.append(host.ensemble_step(t[-1], kind, tables, boundary))
    return t[:p]


def want(key, state, kind, tables, p, boundary="reference"):
    """`host.usage` of the CPU trajectory, computed once and left unchanged."""
    full = (key, kind, boundary, p)
    if full not in _WANT:
        _WANT[full] = host.usage_of_phases(phases(key, state, kind, tables, boundary, p), kind, boundary)
        _WANT[full].setflags(write=False)
    return _WANT[full]


def times(rec, p):
    """The record of p steps of a fixed point whose one step is `rec`."""
    out = rec.copy()
    out["steps"] = p
    out["dead"], out["alive"] = rec["dead"].astype(np.uint64) * p, rec["alive"].astype(np.uint64) * p
    return out


def same_record(got, exp, where):
    for f in host.USAGE_DTYPE.names:
        assert np.array_equal(got[f], exp[f]), (where, f, got[f], exp[f])
    assert got.tobytes() == exp.tobytes(), where


def call_and_check(e, wants, steps, first=0):
    rec = e.usage(np.asarray(steps, dtype=np.uint32), first)
    assert rec.shape == (len(wants),) and rec.dtype == host.USAGE_DTYPE
    for k, w in enumerate(wants):
        same_record(rec[k], w, first + k)
    assert e.usage_gpu_ms() > 0.0
    return rec


# ---------------------------------------------------------------------------------------------- every bin, every face

@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kind", KINDS)
def test_graded_states_reach_every_bin(ens, graded, kind, boundary):
    """The four graded states at P = 1 — no bin of any class is empty there (test_usage_cpu.py), so every bin's decode counts — and at
    P = 3 under a coded rule each, which answers adjacent counts differently: the kernel's next state counts too."""
    tables = [tables_of(kind, rule_of(kind, j)) for j in range(4)] * 2
    hold(ens, kind, tables, graded * 2, boundary)
    steps = [1] * 4 + [3] * 4
    wants = [want(("graded", k % 4), graded[k % 4], kind, tables[k], p, boundary) for k, p in enumerate(steps)]
    rec = call_and_check(ens, wants, steps)
    for base, n in host._usage_classes(kind):
        assert rec["dead"][:4, base:base + n].all() and rec["alive"][:4, base:base + n].all()
    assert not np.array_equal(rec["alive"][0] * 3, rec["alive"][4])  # the state moved


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("kind", KINDS)
def test_lone_cells_on_faces_and_seams(ens, kind, boundary):
    """One cell, born at one neighbour, P = 1 .. 4: what crosses a face, the word seam of a row or the seam between two waves shows in
    the counts of the very next step."""
    tables = tables_of(kind, grow_rule(kind))
    states = [host.cells_to_words(G, [c]) for c in LONE for _ in range(4)]
    steps = [1, 2, 3, 4] * len(LONE)
    hold(ens, kind, tables, states, boundary)
    wants = [want(("lone", LONE[k // 4]), states[k], kind, tables, p, boundary) for k, p in enumerate(steps)]
    call_and_check(ens, wants, steps)
    if kind == "moore":  # the origin is seen from all 26 sides, from 7, or from 26 on a torus; so the boundaries differ
        seen = int(wants[0]["dead"][1])
        assert seen == {"reference": 26, "torus": 26, "closed": 7}[boundary]


# ---------------------------------------------------------------------------------------------- the counters at their largest

@pytest.mark.parametrize("boundary", ("torus", "closed"))
@pytest.mark.parametrize("kind", KINDS)
def test_the_full_universe_over_many_steps(ens, kind, boundary):
    """FULL under survive-everywhere is a fixed point, so P steps are P times one step — closed form. 255 | 256 | 257 and 300 lie around
    the step count a packed 16-bit accumulator holds, 4096 is the longest run: on a Moore torus alive[26] = 2^30, the largest value a
    bin takes and every thread's largest share of one bin. EMPTY stays empty: dead[0]."""
    tables = everything(kind)
    steps = [255, 256, 257, 300, 4096]
    hold(ens, kind, tables, [FULL] * len(steps) + [EMPTY], boundary)
    one, none = want("full", FULL, kind, tables, 1, boundary), want("empty", EMPTY, kind, tables, 1, boundary)
    rec = call_and_check(ens, [times(one, p) for p in steps] + [times(none, 4096)], steps + [4096])
    if kind == "moore" and boundary == "torus":
        assert [int(v) for v in rec["alive"][:5, 26]] == [CELLS * p for p in steps] and int(rec["alive"][4, 26]) == 1 << 30
    if boundary == "closed" and kind == "von neumann":
        assert [int(v) for v in rec["alive"][0, :7]] == [0, 0, 0, 8 * 255, 12 * 62 * 255, 6 * 62 * 62 * 255, 62 ** 3 * 255]
    for base, n in host._usage_classes(kind):
        assert int(rec["dead"][5, base]) == CELLS * 4096 == int(rec["dead"][5, base:base + n].sum()) and not rec["alive"][5].any()


# ---------------------------------------------------------------------------------------------- launches

def soups(n, seed=40):
    return [host.seeded_state(G, seed + k, k % 3) for k in range(n)]


@pytest.mark.parametrize("kind", KINDS)
def test_step_counts_that_differ_inside_one_launch(ens, kind):
    steps = [1, 2, 3, 4, 8, 5]
    states = soups(len(steps))
    tables = [tables_of(kind, rule_of(kind, k)) for k in range(len(steps))]
    hold(ens, kind, tables, states, "torus")
    call_and_check(ens, [want(("mixed", k), states[k], kind, tables[k], p, "torus") for k, p in enumerate(steps)], steps)


@pytest.mark.parametrize("b", (1, 3))
def test_one_and_three_universes(ens, b):
    states = soups(b, 50)
    tables = tables_of("clustered", rule_of("clustered", 3))
    hold(ens, "clustered", tables, states)
    call_and_check(ens, [want(("small", k), states[k], "clustered", tables, 2) for k in range(b)], [2] * b)


def test_more_universes_than_compute_units_over_a_range(ens):
    """310 universes, usage over 7 .. 306 with step counts 1 .. 3 in turn."""
    pool = [(("pool", k), s) for k, s in enumerate(soups(5, 60))]
    tables = tables_of("moore", rule_of("moore", 1))
    marker = host.seeded_state(G, 6, 3)
    picks = [pool[(k * 7) % len(pool)] for k in range(300)]
    steps = [1 + (k * 2) % 3 for k in range(300)]
    hold(ens, "moore", tables, [marker] * 7 + [p[1] for p in picks] + [marker] * 3)
    before = snapshot(ens)
    rec = call_and_check(ens, [want(p[0], p[1], "moore", tables, q) for p, q in zip(picks, steps)], steps, first=7)
    assert snapshot(ens) == before
    # a smaller second call reuses the staging array; count and a scalar step count
    again = ens.usage(steps[93:98], first=100)
    assert again.tobytes() == rec[93:98].tobytes()
    assert ens.usage(3, first=8, count=2).tobytes() == ens.usage([3, 3], first=8).tobytes()


# ---------------------------------------------------------------------------------------------- what the record is for

@pytest.mark.parametrize("kind", KINDS)
def test_dont_care_bits_change_nothing(ens, nursery, kind):
    """Flip every table bit the usage names as never read, per universe; step both ensembles: the states are equal word for word, and
    the CPU chain agrees."""
    P = 5
    slow = gl._rule("born at 2", 1 << 2, 0b111)
    rules = [rule_of(kind, 2), rule_of(kind, 5), gl.clustered("main", slow) if kind == "clustered" else slow]  # (clustered: the sides silent)
    tables = [tables_of(kind, r) for r in rules]
    states = [host.seeded_state(G, 70, 2), host.seeded_state(G, 71, 4), host.seeded_state(G, 72, 6)]
    hold(ens, kind, tables, states, "reference")
    rec = ens.usage(P)
    flipped, some = [], 0
    for k, (born, survive) in enumerate(tables):
        bdc, sdc = host.usage_dont_care(rec[k], kind)
        some += sum(bdc) + sum(sdc)
        if kind == "clustered":
            flipped.append(([b ^ d for b, d in zip(born, bdc)], [s ^ d for s, d in zip(survive, sdc)]))
        else:
            flipped.append((born ^ bdc[0], survive ^ sdc[0]))
    assert some  # the sparse universe leaves the high counts unread
    hold(nursery, kind, flipped, states, "reference")
    ens.step(P)
    nursery.step(P)
    got = ens.read_state()
    np.testing.assert_array_equal(got, nursery.read_state())
    for k in range(3):
        chain = phases(("dont care", k), states[k], kind, tables[k], "reference", P + 1)
        np.testing.assert_array_equal(got[k], chain[P], err_msg=str(k))
        same_record(rec[k], want(("dont care", k), states[k], kind, tables[k], P), k)


@pytest.mark.parametrize("kind", ("von neumann", "moore"))
def test_births_and_deaths_follow_from_the_histogram(ens, nursery, kind):
    P = 6
    tables = [tables_of(kind, rule_of(kind, j)) for j in range(3)]
    states = soups(3, 80)
    hold(ens, kind, tables, states, "closed")
    hold(nursery, kind, tables, states, "closed")
    rec = ens.usage(P)
    samples, count, _, _ = nursery.step_trace(P, check_every=1)
    for k in range(3):
        assert int(count[k]) == P + 1  # the entry, then one sample a step
        births, deaths = int(samples[k, 1:, 1].sum()), int(samples[k, 1:, 2].sum())
        assert host.usage_births_deaths(rec[k], kind, tables[k]) == (births, deaths) and births and deaths, k


def test_ordering_and_read_only(ens):
    """A step queued and not waited for lies in front of the call; the ensemble is byte for byte what it was, and goes on."""
    tables = tables_of("moore", rule_of("moore", 0))
    states = soups(2, 90)
    hold(ens, "moore", tables, states)
    ens.step(3)  # queued, not synchronised
    rec = ens.usage([2, 4])
    stepped = [phases(("ordering", k), states[k], "moore", tables, "reference", 4)[3] for k in range(2)]
    for k, p in enumerate((2, 4)):
        same_record(rec[k], want(("ordering stepped", k), stepped[k], "moore", tables, p), k)
    assert ens.usage_gpu_ms() > 0.0
    before = snapshot(ens)
    np.testing.assert_array_equal(ens.read_state(), np.stack(stepped))
    assert ens.summaries()[0].step == 3
    assert ens.usage(4).tobytes() == ens.usage(4).tobytes() and snapshot(ens) == before
    ens.step(1)  # and the ensemble goes on
    np.testing.assert_array_equal(ens.read_state()[0], host.ensemble_step(stepped[0], "moore", tables))


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals(ens):
    lib = _capi.load()
    out = (_capi.UsageStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    good = (C.c_uint32 * 5)(4, 8, 1, 2, 3)
    ms = C.c_float(-1.0)
    tables = tables_of("moore", rule_of("moore", 0))

    def refused(code, pattern, e, first, count, steps, out_):
        rc = lib.ca3d_ensemble_usage(e, first, count, steps, out_, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(good) == [4, 8, 1, 2, 3] and ms.value == -1.0, msg

    refused(-1, "NULL", None, 0, 2, good, out)
    refused(-2, "configure", ens._h, 0, 2, good, out)  # an unconfigured handle
    ens.configure(8, neighbourhood="moore")
    refused(-1, "NULL", ens._h, 0, 2, good, None)
    refused(-1, "NULL", ens._h, 0, 2, None, out)
    refused(-2, "universe 0", ens._h, 0, 2, good, out)  # no state anywhere
    ens.upload_state(0, np.stack(soups(2, 95)))
    refused(-2, "upload_state.*universe 2", ens._h, 1, 2, good, out)  # universe 2 has none
    ens.upload_state(2, np.stack(soups(6, 96)))
    refused(-2, "set_rules.*universe 0", ens._h, 0, 4, good, out)  # states everywhere, rules nowhere
    ens.set_rule_tables(0, [tables[0]] * 2, [tables[1]] * 2)
    refused(-2, "set_rules.*universe 2", ens._h, 1, 2, good, out)  # universe 2 has none
    ens.set_rule_tables(0, [tables[0]] * 8, [tables[1]] * 8)
    before = snapshot(ens)
    refused(-1, "universes", ens._h, 0, 0, good, out)  # count 0
    refused(-1, "universes", ens._h, 7, 2, good, out)  # a range past n
    refused(-1, "universes", ens._h, 8, 1, good, out)
    refused(-1, "universes", ens._h, 0, 9, good, out)
    refused(-1, r"steps\[1\].*universe 3", ens._h, 2, 4, (C.c_uint32 * 4)(4, 0, 4, 4), out)  # a step count of 0
    refused(-1, r"steps\[3\]", ens._h, 0, 4, (C.c_uint32 * 4)(4, 4, 4, host.CANON_MAX_PERIOD + 1), out)
    assert snapshot(ens) == before
    with pytest.raises(Ca3dError) as e:
        ens.usage([4, 0, 4, 4])
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ens.usage([4, 4], count=3)
    # gpu_ms is nullable
    assert lib.ca3d_ensemble_usage(ens._h, 0, 4, good, out, None) == 0
    assert bytes(out) != b"\x5a" * C.sizeof(out)
    assert snapshot(ens) == before
