"""`ca3d_ensemble_envelope` on the GPU (the nine kernels of csrc/ca_envelope.hip) against `host.envelope`, the numpy restatement of the
definition in include/ca3d.h, fed with CPU trajectories (chains of `host.ensemble_step`, which tests/test_ensemble_boundary_cpu.py pins
to the CPU oracle): every field of every record and every word of every image, exactly. tests/test_envelope_cpu.py checks
`host.envelope` itself against a brute force. Universes are 64^3 by construction."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import census_cases as cc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_cycle import MOORE as CYCLE_MOORE
from test_gpu_cycle import VN as CYCLE_VN
from test_gpu_ensemble_clustered import BITS as CLUSTERED_BITS
from test_gpu_ensemble_clustered import RULES as CLUSTERED_RULES
from test_gpu_moving import SHIP, glider, ship

pytestmark = pytest.mark.gpu

G, W = 64, 8192
RETURNS = host.ENVELOPE_RETURNS
IMAGES = ("envelope", "stator", "rotor")
OSCILLATOR = ((15, 15, 15), (16, 15, 15), (15, 16, 15), (15, 15, 16))  # Moore B4/S4, period 2


def mask(s, bits=27):
    m = 0
    for v in host.rules_components_to_values(s):
        m |= 1 << v
    return m & ((1 << bits) - 1)


def clustered_tables(rule):
    return (tuple(mask(rule[2 * i], CLUSTERED_BITS[i]) for i in range(3)), tuple(mask(rule[2 * i + 1], CLUSTERED_BITS[i]) for i in range(3)))


SHIP_TABLES = (mask(SHIP[0]), mask(SHIP[1]))
B4S4 = (mask("4"), mask("4"))
LIFE_VN = (mask("3", 7), mask("2,3", 7))
#: a rule of every ensemble kind, 1, 2 and 6 rule words a universe
KIND_TABLES = {"von neumann": LIFE_VN, "moore": SHIP_TABLES, "clustered": clustered_tables(CLUSTERED_RULES[0])}


def cells(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def pack(c):
    return np.packbits(np.ascontiguousarray(c, dtype=np.uint8).ravel(), bitorder="little").view("<u4").astype(np.uint32)


def rolled(words, shift):
    """The state translated by shift = (dx, dy, dz) on the torus."""
    return pack(np.roll(cells(words), shift=(shift[2], shift[1], shift[0]), axis=(0, 1, 2)))


def make_ensemble():
    from cellularautomatons3d_amd import Ensemble

    return Ensemble(0)


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


def hold(e, kind, tables, states, boundary="reference", n=None):
    """Configure `e` as `kind` with len(states) universes (or n, the rest empty), tables[k] (or one pair for all) and the states."""
    n = len(states) if n is None else n
    e.configure(n, neighbourhood="von neumann" if kind == "von neumann" else "moore", clustered=kind == "clustered")
    e.set_boundary(boundary)
    per = tables if isinstance(tables, list) else [tables] * n
    born, survive = np.array([t[0] for t in per], dtype=np.uint32), np.array([t[1] for t in per], dtype=np.uint32)
    if kind == "clustered":
        e.set_clustered_tables(0, born.reshape(-1, 3), survive.reshape(-1, 3))
    else:
        e.set_rule_tables(0, born, survive)
    full = np.zeros((n, W), dtype=np.uint32)
    full[:len(states)] = np.stack(states)
    e.upload_state(0, full)


_CHAINS, _WANT = {}, {}


def phases(key, state, kind, tables, boundary, p):
    """S_0 .. S_p of `state` under host.ensemble_step, kept for the run under (key, kind, boundary): `key` names state and rule."""
    t = _CHAINS.setdefault((key, kind, boundary), [np.ascontiguousarray(state, dtype=np.uint32)])
    assert np.array_equal(t[0], state)
    while len(t) <= p:
        t.append(host.ensemble_step(t[-1], kind, tables, boundary))
    return np.stack(t[:p + 1])


def want(key, state, kind, tables, p, boundary="reference"):
    """`host.envelope` of the CPU trajectory: (record, envelope, stator, rotor), computed once and left unchanged."""
    full = (key, kind, boundary, p)
    if full not in _WANT:
        out = host.envelope_of_phases(phases(key, state, kind, tables, boundary, p))
        for a in out[1:]:
            a.setflags(write=False)
        _WANT[full] = out
    return _WANT[full]


def same_record(got, exp, where):
    for f in host.ENVELOPE_DTYPE.names:
        assert np.array_equal(got[f], exp[f]), (where, f, got[f], exp[f])
    assert got.tobytes() == exp.tobytes(), where


def call_and_check(e, wants, periods, first=0):
    """One call without images over universes first .. first + len(wants) - 1 against wants[k] of `want`. -> records"""
    rec = e.envelope(np.asarray(periods, dtype=np.uint32), first)
    assert rec.shape == (len(wants),) and rec.dtype == host.ENVELOPE_DTYPE
    for k, w in enumerate(wants):
        same_record(rec[k], w[0], first + k)
    assert e.envelope_gpu_ms() > 0.0
    return rec


def snapshot(e):
    return e.read_state().tobytes(), e.summaries(), bytes(e.stats())


# ---------------------------------------------------------------------------------------------- records

@pytest.mark.parametrize("kind,case", [("moore", CYCLE_MOORE[0]), ("von neumann", CYCLE_VN[2])])
def test_true_oscillators(ens, kind, case):
    """tests/test_gpu_cycle.py's Moore B5/S4,5 soup (period 4) and its von Neumann B3/S2,3 soup (period 2) once `step_until_cycle` has
    found the period p: RETURNS at p, not at p + 1, and the source is byte for byte what it was."""
    b, s, seed, rounds = case
    bits = 7 if kind == "von neumann" else 27
    tables = (mask(b, bits), mask(s, bits))
    hold(ens, kind, tables, [host.random_fill(W, seed=seed, and_rounds=rounds)])
    done, reason, period = ens.step_until_cycle(192, 1)
    p = int(period[0])
    assert p >= 2, (done, reason, period)
    state = ens.read_state()[0]
    before = snapshot(ens)
    rec = call_and_check(ens, [want(("oscillator", kind), state, kind, tables, p)], [p])
    assert int(rec["flags"][0]) == RETURNS and int(rec["heat"][0]) > 0 and int(rec["stator_population"][0]) < int(rec["envelope_population"][0])
    odd = call_and_check(ens, [want(("oscillator", kind), state, kind, tables, p + 1)], [p + 1])
    assert int(odd["flags"][0]) == 0
    assert snapshot(ens) == before
    assert ens.summaries()[0].step == int(done[0])


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
def test_a_clustered_soup(ens, boundary):
    """tests/test_gpu_ensemble_clustered.py's first four rules — all three table pairs, the edges pair alone, the corners pair alone,
    plain Moore — on soups, periods 3 and 2."""
    tables = [clustered_tables(r) for r in CLUSTERED_RULES[:4]]
    states = [host.random_fill(W, seed=101 + k, and_rounds=(0, 2, 5)[k % 3]) for k in range(4)]
    hold(ens, "clustered", tables, states, boundary)
    periods = [3, 2, 3, 2]
    rec = call_and_check(ens, [want(("clustered", k), states[k], "clustered", tables[k], periods[k], boundary) for k in range(4)], periods)
    assert rec["heat"].any()


def test_periods_that_differ_inside_one_launch(ens):
    """Periods 1, 2, 3, 4, 8 and 5 over the glider's phases and two soups: RETURNS nowhere (a ship, soups on their way)."""
    t = ship("a")
    states = [t[0], t[1], t[2], t[3], host.random_fill(W, seed=9, and_rounds=1), host.random_fill(W, seed=5, and_rounds=3)]
    periods = [1, 2, 3, 4, 8, 5]
    hold(ens, "moore", SHIP_TABLES, states)
    rec = call_and_check(ens, [want(("mixed", k), states[k], "moore", SHIP_TABLES, periods[k]) for k in range(6)], periods)
    np.testing.assert_array_equal(rec["period"], periods)
    assert not rec["flags"][:4].any()


#: the glider of tests/test_gpu_moving.py in reference mode: across the word seam x = 31 | 32, across the wave seam z = 7 | 8, and
#: onto the + x face, which it reaches in its second period
SEAMS = {"word seam": ("xy", (29, 20, 20)), "wave seam": ("yz", (20, 20, 5)), "plus face": ("xy", (60, 20, 20))}


def test_the_glider_through_seams_and_a_face(ens):
    names = list(SEAMS)
    states = [glider(*SEAMS[n]) for n in names]
    hold(ens, "moore", SHIP_TABLES, states)
    rec = call_and_check(ens, [want(("seam", n), s, "moore", SHIP_TABLES, 8) for n, s in zip(names, states)], [8] * 3)
    by = dict(zip(names, rec))
    assert tuple(by["word seam"]["envelope_min"])[0] <= 31 and tuple(by["word seam"]["envelope_max"])[0] >= 32
    assert tuple(by["wave seam"]["envelope_min"])[2] <= 7 and tuple(by["wave seam"]["envelope_max"])[2] >= 8
    assert tuple(by["plus face"]["envelope_max"])[0] == 63  # it reached the face
    assert not rec["flags"].any()  # a swept volume, no RETURNS


def test_the_oscillator_astride_a_torus_seam_and_against_a_closed_face(ens):
    """The B4/S4 oscillator's cube rolled onto x = 63 | 0, y = 63 | 0 and z = 63 | 0 of a torus ensemble, one seam a universe; and pushed
    into the corner of the - faces and against the + x face of a closed one."""
    seed = host.cells_to_words(G, OSCILLATOR)
    states = [rolled(seed, tuple(-16 if i == axis else 0 for i in range(3))) for axis in range(3)]
    hold(ens, "moore", B4S4, states, "torus")
    rec = call_and_check(ens, [want(("b4s4 seam", k), states[k], "moore", B4S4, 2, "torus") for k in range(3)], [2] * 3)
    for axis in range(3):
        assert int(rec["flags"][axis]) == RETURNS and int(rec["heat"][axis]) == 16 and int(rec["envelope_population"][axis]) == 8, axis
        assert rec["rotor_min"][axis][axis] == 0 and rec["rotor_max"][axis][axis] == 63, axis
    call_and_check(ens, [want(("b4s4 seam", k), states[k], "moore", B4S4, 3, "torus") for k in range(3)], [3] * 3)
    states = [host.cells_to_words(G, [(x - 15, y - 15, z - 15) for x, y, z in OSCILLATOR]), host.cells_to_words(G, [(x + 47, y, z) for x, y, z in OSCILLATOR])]
    hold(ens, "moore", B4S4, states, "closed")
    rec = call_and_check(ens, [want(("b4s4 face", k), states[k], "moore", B4S4, 2, "closed") for k in range(2)], [2] * 2)
    assert rec["flags"].tolist() == [RETURNS, RETURNS] and tuple(rec["envelope_max"][1]) == (63, 16, 16, 0)


def test_the_counters_at_their_largest(ens):
    """A torus von Neumann universe under B0/S(nothing) from empty flips completely every step: over P = 4096 heat = 2^30,
    population_sum = 2^29, E full, A empty, and it returns (4096 is even). The same numbers at P = 4 from host.ensemble_step first."""
    tables = (mask("0", 7), 0)
    empty = np.zeros(W, dtype=np.uint32)
    few = want("flip", empty, "von neumann", tables, 4, "torus")[0]
    assert (int(few["heat"]), int(few["population_sum"]), int(few["envelope_population"]), int(few["stator_population"]), int(few["flags"])) == \
        (4 << 18, 2 << 18, 1 << 18, 0, RETURNS)
    hold(ens, "von neumann", tables, [empty], "torus")
    call_and_check(ens, [want("flip", empty, "von neumann", tables, 4, "torus")], [4])
    rec = ens.envelope(4096)
    exp = np.zeros((), dtype=host.ENVELOPE_DTYPE)
    exp["period"], exp["flags"], exp["heat"], exp["population_sum"], exp["envelope_population"] = 4096, RETURNS, 1 << 30, 1 << 29, 1 << 18
    exp["envelope_max"][:3] = exp["rotor_max"][:3] = 63
    same_record(rec[0], exp, "P = 4096")
    odd = ens.envelope(4095)  # ends full: no RETURNS
    assert int(odd["flags"][0]) == 0 and int(odd["heat"][0]) == 4095 << 18 and int(odd["population_sum"][0]) == 2047 << 18


def test_the_full_universe_that_stays_full(ens):
    """Moore B(nothing)/S26 on a torus keeps every cell: E = A = full, heat 0, the rotor empty."""
    tables = (0, mask("26"))
    full = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    hold(ens, "moore", tables, [full], "torus")
    rec = call_and_check(ens, [want("full", full, "moore", tables, 7, "torus")], [7])
    assert (int(rec["heat"][0]), int(rec["envelope_population"][0]), int(rec["stator_population"][0]), int(rec["population_sum"][0])) == (0, 1 << 18, 1 << 18, 7 << 18)
    assert tuple(rec["rotor_min"][0]) == tuple(rec["rotor_max"][0]) == (0, 0, 0, 0) and int(rec["flags"][0]) == RETURNS


@pytest.mark.parametrize("b", [1, 3])
def test_one_and_three_universes(ens, b):
    t = ship("a")
    states = [t[1], cc.state("shapes"), host.random_fill(W, seed=77, and_rounds=2)][:b]
    periods = [4, 3, 2][:b]
    hold(ens, "moore", SHIP_TABLES, states)
    call_and_check(ens, [want(("b", k), states[k], "moore", SHIP_TABLES, periods[k]) for k in range(b)], periods)


def check_images(dst, dst_first, wants, names, where=""):
    """Universes from dst_first of `dst` hold, source by source, the images `names` (in the documented order) of wants[k]."""
    n = len(names)
    got = dst.read_state(dst_first, len(wants) * n)
    for k, w in enumerate(wants):
        for i, name in enumerate(names):
            np.testing.assert_array_equal(got[k * n + i], w[1 + IMAGES.index(name)], err_msg=f"{where} source {k}: {name}")


def test_more_universes_than_compute_units_over_a_range(ens, nursery):
    """310 universes, envelope over 7 .. 306 with periods 1 .. 4 in turn and all three images each into a second ensemble of 900."""
    t = ship("a")
    pool = [(("glider phase", k), t[k]) for k in range(4)]
    pool += [(("crafted", n), cc.state(n)) for n in ("shapes", "corners", "empty")]
    pool += [(("soup", 5), host.random_fill(W, seed=5, and_rounds=3)), (("b4s4", 0), host.cells_to_words(G, OSCILLATOR))]
    marker = host.random_fill(W, seed=6, and_rounds=3)
    picks = [pool[(k * 7) % len(pool)] for k in range(300)]
    periods = [1 + (k * 3) % 4 for k in range(300)]
    hold(ens, "moore", SHIP_TABLES, [marker] * 7 + [p[1] for p in picks] + [marker] * 3)
    nursery.configure(900, neighbourhood="moore")
    wants = [want(p[0], p[1], "moore", SHIP_TABLES, q) for p, q in zip(picks, periods)]
    before = snapshot(ens)
    rec = ens.envelope(periods, first=7, dst=nursery, images=IMAGES)
    for k in range(300):
        same_record(rec[k], wants[k][0], 7 + k)
    check_images(nursery, 0, wants, IMAGES)
    assert snapshot(ens) == before
    assert [s.step for s in nursery.summaries(0, 3)] == [0, 0, 0]
    # a smaller second call reuses the staging array
    again = ens.envelope(periods[93:98], first=100)
    assert again.tobytes() == rec[93:98].tobytes()


# ---------------------------------------------------------------------------------------------- images

@pytest.mark.parametrize("kind", ["von neumann", "moore", "clustered"])
def test_images_in_every_combination(ens, nursery, kind):
    """first = 5 in an ensemble of 16: every subset of the three image bits lands at dst_first + k n + i in bit order, in both buffers
    (a step from either parity is the CPU's), with records at step 0; COPY_RULES brings the source's rule of 1, 2 or 6 words, and
    without it the destination keeps its own."""
    tables = KIND_TABLES[kind]
    if kind == "moore":
        t = ship("a")
        states = [t[0], host.cells_to_words(G, OSCILLATOR), host.random_fill(W, seed=21, and_rounds=2)]
    else:
        states = [host.random_fill(W, seed=30 + k, and_rounds=(1, 3, 2)[k]) for k in range(3)]
    marker = host.random_fill(W, seed=6, and_rounds=3)
    per = [KIND_TABLES[kind]] * 16
    hold(ens, kind, per, [marker] * 5 + states + [marker] * 8)
    periods = [4, 2, 3]
    wants = [want((kind, "image", k), states[k], kind, tables, periods[k]) for k in range(3)]
    silent = ((0, 0, 0), (0, 0, 0)) if kind == "clustered" else (0, 0)  # nothing is born, nothing survives
    before = snapshot(ens)
    for r in range(1, 4):
        for names in itertools.combinations(IMAGES, r):
            for copy_rules in (True, False):
                n = len(names)
                hold(nursery, kind, silent, [marker] * (3 * n + 4))
                rec = ens.envelope(periods, first=5, dst=nursery, dst_first=2, images=names, copy_rules=copy_rules)
                for k in range(3):
                    same_record(rec[k], wants[k][0], (names, k))
                check_images(nursery, 2, wants, names, str(names))
                np.testing.assert_array_equal(nursery.read_state(0, 2), np.stack([marker] * 2))
                np.testing.assert_array_equal(nursery.read_state(2 + 3 * n, 2), np.stack([marker] * 2))
                for s, (k, name) in zip(nursery.summaries(2, 3 * n), itertools.product(range(3), names)):
                    assert s.step == 0 and not s.has_previous and (s.births, s.deaths) == (0, 0), (names, k, name)
                    assert s.population == int(ol.popcount(wants[k][1 + IMAGES.index(name)])), (names, k, name)
                # one step from the buffer the images were written to, one more from the other one
                image = wants[1][1 + IMAGES.index(names[0])]
                rule = tables if copy_rules else silent
                one = host.ensemble_step(image, kind, rule)
                nursery.step(1)
                np.testing.assert_array_equal(nursery.read_state(2 + n, 1)[0], one, err_msg=f"{names} {copy_rules}: step 1")
                nursery.step(1)
                np.testing.assert_array_equal(nursery.read_state(2 + n, 1)[0], host.ensemble_step(one, kind, rule), err_msg=f"{names} {copy_rules}: step 2")
                s = nursery.summaries(2 + n, 1)[0]
                assert s.step == 2 and s.has_previous
    # no image: nothing but the records
    rec = ens.envelope(periods, first=5)
    for k in range(3):
        same_record(rec[k], wants[k][0], k)
    assert snapshot(ens) == before


def test_images_into_the_same_ensemble_and_a_census_of_the_rotor(ens):
    """Sources 0 .. 1 write their rotor and envelope behind themselves into the ensemble they live in; the census of a rotor there is
    `host.census` of the host's rotor: the glider's swept volume is one object, the oscillator's cube another."""
    t = ship("a")
    states = [t[0], host.cells_to_words(G, OSCILLATOR)]
    hold(ens, "moore", [SHIP_TABLES, B4S4], states, n=6)
    wants = [want(("census", 0), states[0], "moore", SHIP_TABLES, 4), want(("census", 1), states[1], "moore", B4S4, 2)]
    rec = ens.envelope([4, 2], first=0, dst=ens, dst_first=2, images=("rotor", "envelope"), copy_rules=True)
    assert rec.shape == (2,)  # periods decide the count
    for k in range(2):
        same_record(rec[k], wants[k][0], k)
    check_images(ens, 2, wants, ("envelope", "rotor"))  # bit order, whatever order they were named in
    np.testing.assert_array_equal(ens.read_state(0, 2), np.stack(states))
    comps, n, rest = ens.census(2, 4, max_components=8)
    for u, (k, name) in enumerate(itertools.product(range(2), ("envelope", "rotor"))):
        exp, exp_n, exp_rest = host.census(wants[k][1 + IMAGES.index(name)], 8)
        assert (int(n[u]), int(rest[u])) == (exp_n, exp_rest), (k, name)
        assert comps[u].tobytes() == exp.tobytes(), (k, name)
    assert int(n[3]) == 1 and int(comps[3][0]["population"]) == 8
    # COPY_RULES: destination 4 steps as source 1 does
    ens.step(1)
    np.testing.assert_array_equal(ens.read_state(4, 1)[0], host.ensemble_step(wants[1][1], "moore", B4S4))


def test_ordering(ens, nursery):
    """A step queued and not waited for lies in front of the call; a step of the destination queued behind it sees the images."""
    first = host.random_fill(W, seed=9, and_rounds=1)
    states = [first, cc.state("shapes")]
    hold(ens, "moore", SHIP_TABLES, states)
    hold(nursery, "moore", SHIP_TABLES, [first] * 4)
    ens.step(3)  # queued, not synchronised
    nursery.step(2)  # on the other stream, likewise
    rec = ens.envelope([2, 3], dst=nursery, images=("envelope", "stator"))
    nursery.step(1)
    stepped = [phases(("ordering", k), states[k], "moore", SHIP_TABLES, "reference", 3)[3] for k in range(2)]
    wants = [want(("ordering stepped", k), stepped[k], "moore", SHIP_TABLES, p) for k, p in enumerate((2, 3))]
    for k in range(2):
        same_record(rec[k], wants[k][0], k)
    got = nursery.read_state()
    for k in range(2):
        for i in range(2):
            np.testing.assert_array_equal(got[2 * k + i], host.ensemble_step(wants[k][1 + i], "moore", SHIP_TABLES), err_msg=f"{k} {i}")
    np.testing.assert_array_equal(ens.read_state(), np.stack(stepped))
    assert ens.summaries()[0].step == 3 and nursery.summaries()[0].step == 1
    ens.step(1)  # and the source goes on
    np.testing.assert_array_equal(ens.read_state()[0], host.ensemble_step(stepped[0], "moore", SHIP_TABLES))


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals(ens, nursery):
    lib = _capi.load()
    out = (_capi.EnvelopeStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    good = (C.c_uint32 * 5)(4, 8, 1, 2, 3)
    ms = C.c_float(-1.0)
    E, S, R, COPY = 1, 2, 4, _capi.ENVELOPE_COPY_RULES

    def refused(code, pattern, src, first, count, periods, dst, dst_first, flags, out_):
        rc = lib.ca3d_ensemble_envelope(src, first, count, periods, dst, dst_first, flags, out_, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(good) == [4, 8, 1, 2, 3] and ms.value == -1.0, msg

    refused(-1, "NULL", None, 0, 2, good, None, 0, 0, out)
    refused(-2, "configure", ens._h, 0, 2, good, None, 0, 0, out)  # an unconfigured handle
    ens.configure(8, neighbourhood="moore")
    refused(-1, "NULL", ens._h, 0, 2, good, None, 0, 0, None)
    refused(-1, "NULL", ens._h, 0, 2, None, None, 0, 0, out)
    refused(-2, "universe 0", ens._h, 0, 2, good, None, 0, 0, out)  # no state anywhere
    ens.upload_state(0, np.stack([cc.state("shapes")] * 2))
    refused(-2, "upload_state.*universe 2", ens._h, 1, 2, good, None, 0, 0, out)  # universe 2 has none
    ens.upload_state(2, np.stack([cc.state("corners")] * 6))
    refused(-2, "set_rules.*universe 0", ens._h, 0, 4, good, None, 0, 0, out)  # states everywhere, rules nowhere
    ens.set_rule_tables(0, [SHIP_TABLES[0]] * 2, [SHIP_TABLES[1]] * 2)
    refused(-2, "set_rules.*universe 2", ens._h, 1, 2, good, None, 0, 0, out)  # universe 2 has none
    ens.set_rule_tables(0, [SHIP_TABLES[0]] * 8, [SHIP_TABLES[1]] * 8)
    refused(-2, "configure.*destination", ens._h, 0, 2, good, nursery._h, 0, E, out)  # an unconfigured destination
    nursery.configure(6, neighbourhood="von neumann")
    nursery.upload_state(0, np.stack([cc.state("shapes")] * 6))
    before = (snapshot(ens), nursery.read_state().tobytes())
    refused(-1, "universes", ens._h, 0, 0, good, None, 0, 0, out)  # count 0
    refused(-1, "universes", ens._h, 7, 2, good, None, 0, 0, out)  # a range past n
    refused(-1, "universes", ens._h, 8, 1, good, None, 0, 0, out)
    refused(-1, "universes", ens._h, 0, 9, good, None, 0, 0, out)
    refused(-1, r"periods\[1\]", ens._h, 0, 4, (C.c_uint32 * 4)(4, 0, 4, 4), None, 0, 0, out)  # a period of 0
    refused(-1, r"periods\[3\]", ens._h, 0, 4, (C.c_uint32 * 4)(4, 4, 4, host.CANON_MAX_PERIOD + 1), None, 0, 0, out)
    refused(-1, "unknown bits", ens._h, 0, 2, good, None, 0, 8, out)
    refused(-1, "unknown bits", ens._h, 0, 2, good, nursery._h, 0, E | 0x200, out)
    refused(-1, "dst is NULL", ens._h, 0, 2, good, None, 0, E | R, out)  # image bits without a destination
    refused(-1, "no image", ens._h, 0, 2, good, nursery._h, 0, 0, out)  # a destination without image bits
    refused(-1, "no image", ens._h, 0, 2, good, None, 0, COPY, out)  # rules to copy and nowhere to
    refused(-1, "images into universes", ens._h, 0, 4, good, nursery._h, 0, E | S, out)  # 8 destinations of 6
    refused(-1, "images into universes", ens._h, 0, 2, good, nursery._h, 3, E | S, out)  # 3 + 4 of 6
    refused(-1, "images into universes", ens._h, 0, 2, good, nursery._h, 6, E, out)
    refused(-1, "source universe 3 lies among the destinations", ens._h, 0, 4, good, ens._h, 3, E, out)  # the same ensemble
    refused(-1, "source universe 2 lies among the destinations", ens._h, 2, 2, good, ens._h, 0, E | S, out)
    refused(-5, "CA3D_ENVELOPE_COPY_RULES.*neighbourhood", ens._h, 0, 2, good, nursery._h, 0, E | COPY, out)  # Moore into von Neumann
    assert (snapshot(ens), nursery.read_state().tobytes()) == before
    with pytest.raises(Ca3dError) as e:
        ens.envelope([4, 0, 4, 4])
    assert e.value.code == -1
    with pytest.raises(Ca3dError) as e:
        ens.envelope(4, images=("rotor",))  # no dst
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ens.envelope(4, dst=nursery, images=("halo",))
    # gpu_ms is nullable; without COPY_RULES the kinds may differ; the destinations right behind the sources are fine
    assert lib.ca3d_ensemble_envelope(ens._h, 0, 4, good, None, 0, 0, out, None) == 0
    assert bytes(out) != b"\x5a" * C.sizeof(out)
    assert lib.ca3d_ensemble_envelope(ens._h, 0, 2, good, nursery._h, 2, E | S, out, None) == 0
    assert lib.ca3d_ensemble_envelope(ens._h, 0, 4, good, ens._h, 4, E, out, None) == 0
    # a scalar period is that of every universe from `first` on
    np.testing.assert_array_equal(ens.envelope(2, first=6), ens.envelope([2, 2], first=6))
