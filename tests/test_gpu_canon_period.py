"""`ca3d_ensemble_canon_period` on the GPU (kernels ca_ensemble_canon_period_vn64 / _moore64 / _clustered64, csrc/ca_canon_period.hip)
against `host.canon_period`, the numpy restatement of the definition in include/ca3d.h, fed with CPU-oracle trajectories
(oracle_lib.packed_step): every field of every record and the key of every phase, exactly. tests/test_canon_period_cpu.py checks
`host.canon_period` itself against a brute force. The crafted states are tests/census_cases.py's, the small shapes
tests/canon_cases.py's, the glider tests/test_gpu_moving.py's."""
import ctypes as C
import re

import numpy as np
import pytest

import canon_cases as kc
import census_cases as cc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_cycle import MOORE as CYCLE_MOORE
from test_gpu_cycle import VN as CYCLE_VN
from test_gpu_ensemble_clustered import KEYS as CLUSTERED_KEYS
from test_gpu_ensemble_clustered import RULES as CLUSTERED_RULES
from test_gpu_moving import SHIP, moore_rules, ship

pytestmark = pytest.mark.gpu

G, W = 64, 8192
FULL = (1 << 48) - 1
FIELDS = ("key", "symmetry", "orientation", "phase", "population", "flags_shift")
CLOSED = host.CANON_CLOSED


def make_ensemble():
    from cellularautomatons3d_amd import Ensemble

    return Ensemble(0)


@pytest.fixture()
def ens():
    e = make_ensemble()
    yield e
    e.close()


@pytest.fixture()
def stage():
    e = make_ensemble()
    yield e
    e.close()


def hold(e, states, rule=SHIP, nb="moore"):
    e.configure(len(states), neighbourhood=nb)
    e.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood=nb, born=rule[0], survive=rule[1])
    e.upload_state(0, np.stack(states))


def phases(state, rules, p):
    """The oracle's S_0 .. S_p."""
    t = [np.ascontiguousarray(state, dtype=np.uint32)]
    for _ in range(p):
        t.append(ol.packed_step(G, t[-1], rules))
    return np.stack(t)


_REF = {}


def reference(key, state, rules, p):
    """`host.canon_period` of the oracle's phases of `state`, kept under (key, p) for the run."""
    if (key, p) not in _REF:
        rec, keys = host.canon_period(phases(state, rules, p))
        keys.setflags(write=False)
        _REF[key, p] = (rec, keys)
    return _REF[key, p]


def call_and_check(e, wants, periods, first=0):
    """One call with keys over universes first .. first + len(wants) - 1 against wants[k] = (record, keys) of `reference`; and once more
    without keys: the same records. -> (records, keys)"""
    n = len(wants)
    periods = np.asarray(periods, dtype=np.uint32)
    rec, keys = e.canon_period(periods, first, n, keys=True)
    assert rec.shape == (n,) and rec.dtype == host.CANON_PERIOD_DTYPE and keys.shape == (n, int(periods.max())) and keys.dtype == np.uint64
    for k in range(n):
        want, want_keys = wants[k]
        p = int(periods[k])
        assert want_keys.shape == (p,)
        np.testing.assert_array_equal(keys[k, :p], want_keys, err_msg=f"universe {first + k}: keys")
        assert not keys[k, p:].any(), f"universe {first + k}: slots past the period"
        for f in FIELDS:
            assert int(rec[k][f]) == int(want[f]), (first + k, f, int(rec[k][f]), int(want[f]))
    assert e.canon_period_gpu_ms() > 0.0
    alone = e.canon_period(periods, first, n)
    assert alone.tobytes() == rec.tobytes()
    return rec, keys


def test_period_one_is_canon(ens):
    """Every crafted state of the census tests and every small shape with period 1: key, orientation, symmetry and population are
    `canon`'s, keys[:, 0] is the key, and CLOSED says whether one step of B6/S5-7 leaves the state as it is up to a translation."""
    names = [("crafted", n) for n in cc.CRAFTED] + [("small", n) for n in sorted(kc.SHAPES)]
    states = [cc.state(n) if kind == "crafted" else kc.shape_words(n) for kind, n in names]
    hold(ens, states)
    rules = moore_rules(*SHIP)
    wants = [reference(k, s, rules, 1) for k, s in zip(names, states)]
    rec, keys = call_and_check(ens, wants, np.ones(len(states), dtype=np.uint32))
    canon = ens.canon()
    for f in ("key", "orientation", "symmetry", "population"):
        np.testing.assert_array_equal(rec[f], canon[f], err_msg=f)
    for k, name in enumerate(names):
        assert int(rec["key"][k]) == int(kc.reference(name, states[k])[0]["key"]), name
    np.testing.assert_array_equal(keys[:, 0], rec["key"])
    assert not rec["phase"].any()
    by = dict(zip(names, rec))
    assert [int(by["crafted", "empty"][f]) for f in FIELDS] == [0, FULL, 0, 0, 0, CLOSED]
    # at least one state of the list is a still life under the rule and at least one is not: CLOSED is looked at both ways
    closed = (rec["flags_shift"] & CLOSED).astype(bool)
    assert closed.any() and not closed.all()
    assert not (rec["flags_shift"][closed] >> 8).any()


def glider_universes(ens, stage):
    """tests/test_gpu_canon.py's 192 universes in `stage`: the doubled glider's four phases, each turned by every orientation on the
    device and put at (30, 30, 30), with the rule. -> their states"""
    t = ship("a")
    hold(ens, [t[k] for k in range(4)])
    stage.configure(192, neighbourhood="moore")
    stage.compose([[(k, o, (30, 30, 30))] for k in range(4) for o in range(48)], 0, ens, False, True)
    return list(stage.read_state())


def test_the_glider_in_48_orientations_and_4_phases(ens, stage):
    """One key for all 192, the smallest of the four `host.canon` keys; `phase` the first round that reaches it; CLOSED everywhere; the
    shift is the untransformed glider's, turned. Afterwards states, records and stats are byte for byte what they were."""
    t = ship("a")
    states = glider_universes(ens, stage)
    rules = moore_rules(*SHIP)
    before = (stage.read_state().tobytes(), stage.summaries(), bytes(stage.stats()))
    wants = [reference(("glider", u), states[u], rules, 4) for u in range(192)]
    rec, keys = call_and_check(stage, wants, np.full(192, 4, dtype=np.uint32))
    want = [int(host.canon(t[k])[0]["key"]) for k in range(4)]
    smallest = min(want)
    assert set(rec["key"].tolist()) == {smallest}
    for k in range(4):  # group k is in phase (k + t) % 4 in round t
        first = next(r for r in range(4) if want[(k + r) % 4] == smallest)
        assert set(rec["phase"][48 * k:48 * k + 48].tolist()) == {first}, k
        for r in range(4):
            assert set(keys[48 * k:48 * k + 48, r].tolist()) == {want[(k + r) % 4]}, (k, r)
    assert (rec["flags_shift"] & CLOSED).all()
    moved = host.moved_by(G, t[0], t[4])
    assert moved == (1, 1, 0)
    for u in range(192):
        assert host.unpack_shift(rec["flags_shift"][u]) == host.orient_vector(u % 48, moved), u
    assert (stage.read_state().tobytes(), stage.summaries(), bytes(stage.stats())) == before
    assert stage.summaries(0, 1)[0].step == 0


def test_periods_that_differ_inside_one_launch(ens, stage):
    """Periods 1, 2, 3, 4, 8 and 5 in rotation over the 192 glider universes: CLOSED exactly where the period is a multiple of 4, and
    the slots of `keys` past a universe's period are zero (call_and_check)."""
    states = glider_universes(ens, stage)
    rules = moore_rules(*SHIP)
    periods = np.array([(1, 2, 3, 4, 8, 5)[u % 6] for u in range(192)], dtype=np.uint32)
    wants = [reference(("glider", u), states[u], rules, int(periods[u])) for u in range(192)]
    rec, keys = call_and_check(stage, wants, periods)
    assert keys.shape == (192, 8)
    np.testing.assert_array_equal((rec["flags_shift"] & CLOSED).astype(bool), periods % 4 == 0)
    for u in np.flatnonzero(periods == 8):
        assert host.unpack_shift(rec["flags_shift"][u]) == host.orient_vector(u % 48, (2, 2, 0)), u


def heading(v):
    """An orientation that turns the glider's (1, 1, 0) into v."""
    return next(o for o in range(48) if host.orient_vector(o, (1, 1, 0)) == v)


#: name -> (orientation's heading, where compose puts the turned box's minimum, period): the glider crosses the word seam x = 31 | 32;
#: wave seams z = 7 | 8 upwards and z = 3 | 4 downwards; reaches lane y = 0 and lane y = 63 without leaving; leaves through the + x face
#: and wraps; runs into the - x face, and into the - z face, and dies against it
SEAMS = {
    "word seam": ((1, 1, 0), (29, 20, 20), 8),
    "word seam back": ((-1, 1, 0), (32, 20, 20), 8),
    "wave seam up": ((0, 1, 1), (20, 20, 5), 8),
    "wave seam down": ((1, 0, -1), (20, 20, 4), 8),
    "lane 0": ((1, -1, 0), (20, 2, 20), 8),
    "lane 63": ((0, 1, 1), (20, 59, 40), 8),
    "plus x face": ((1, 1, 0), (60, 20, 20), 8),
    "plus z face": ((0, 1, 1), (20, 20, 61), 8),
    "minus x face": ((-1, 1, 0), (1, 20, 20), 12),
    "minus z face": ((1, 0, -1), (20, 20, 1), 12),
}


def test_seams_and_faces(ens, stage):
    t = ship("a")
    hold(ens, [t[0]])
    names = list(SEAMS)
    stage.configure(len(names), neighbourhood="moore")
    made = stage.compose([[(0, heading(SEAMS[n][0]), SEAMS[n][1])] for n in names], 0, ens, False, True)
    assert not made["clipped"].any()
    states = list(stage.read_state())
    rules = moore_rules(*SHIP)
    periods = [SEAMS[n][2] for n in names]
    wants = [reference(("seam", n), states[k], rules, periods[k]) for k, n in enumerate(names)]
    rec, _ = call_and_check(stage, wants, periods)
    by = dict(zip(names, rec))
    for n in names:
        inside = "face" not in n
        assert bool(int(by[n]["flags_shift"]) & CLOSED) == inside, n  # (the oracle's, by call_and_check; what the case is there for)
        if inside:
            assert host.unpack_shift(by[n]["flags_shift"]) == tuple(2 * c for c in SEAMS[n][0]), n


def soup_cases(kind):
    """[(key, state, oracle rules, strings for set_rule_strings, period)] of one ensemble kind: dense and sparse soups (and_rounds 0, 1,
    3) under the kind's rules, periods 5 and 2 in turn — untrue ones."""
    if kind == "clustered":
        rule_list = [dict(zip(CLUSTERED_KEYS, CLUSTERED_RULES[0]))]
    else:
        src = CYCLE_VN if kind == "von neumann" else CYCLE_MOORE
        rule_list = [dict(born=src[0][0], survive=src[0][1]), dict(born=src[3][0], survive=src[3][1])]
    nb = "von neumann" if kind == "von neumann" else "moore"
    out = []
    for r, strings in enumerate(rule_list):
        for f, rounds in enumerate((0, 1, 3)):
            state = host.random_fill(W, seed=40 + 3 * r + f, and_rounds=rounds)
            out.append(((kind, r, rounds), state, ol.Rules.from_strings(neighbourhood=nb, **strings), strings, (5, 2)[(r + f) % 2]))
    return nb, out


@pytest.mark.parametrize("kind", ["von neumann", "moore", "clustered"])
def test_soups_of_every_kind_with_an_untrue_period(ens, kind):
    """What catches a wrong step, a stale exchange buffer or an image that the exchange overwrote: every key of every phase of soups
    that fill the cube, under rules of all three ensemble kinds, against the oracle."""
    nb, cases = soup_cases(kind)
    ens.configure(len(cases), neighbourhood=nb, clustered=kind == "clustered")
    for k, (_, _, _, strings, _) in enumerate(cases):
        ens.set_rule_strings(k, neighbourhood=nb, **strings)
    ens.upload_state(0, np.stack([c[1] for c in cases]))
    periods = [c[4] for c in cases]
    wants = [reference(c[0], c[1], c[2], c[4]) for c in cases]
    rec, keys = call_and_check(ens, wants, periods)
    assert set(periods) == {5, 2}
    assert any(len(set(k[:p].tolist())) == p for k, p in zip(keys, periods))  # the phases differ: the kernel stepped


def copy_of(e, stage, nb, rule):
    stage.configure(e.n, neighbourhood=nb)
    stage.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood=nb, born=rule[0], survive=rule[1])
    stage.upload_state(0, e.read_state())


@pytest.mark.parametrize("nb,case", [("moore", CYCLE_MOORE[0]), ("von neumann", CYCLE_VN[2])])
def test_true_oscillators(ens, stage, nb, case):
    """tests/test_gpu_cycle.py's Moore B5/S4,5 soup (period 4) and its von Neumann B3/S2,3 soup (period 2) once `step_until_cycle` has
    found the cycle: CLOSED with shift 0; key, phase, orientation and symmetry are what `canon_phases` computes on a copy of the
    ensemble, which is p steps further afterwards — the original is not."""
    b, s, seed, rounds = case
    ens.configure(1, neighbourhood=nb)
    ens.set_rule_strings(0, neighbourhood=nb, born=b, survive=s)
    ens.upload_state(0, host.random_fill(W, seed=seed, and_rounds=rounds)[None])
    done, reason, period = ens.step_until_cycle(192, 1)
    p = int(period[0])
    assert p >= 2, (done, reason, period)
    state = ens.read_state()[0]
    before = (state.tobytes(), ens.summaries(), bytes(ens.stats()))
    rules = ol.Rules.from_strings(neighbourhood=nb, born=b, survive=s)
    rec, _ = call_and_check(ens, [reference(("oscillator", nb), state, rules, p)], [p])
    assert int(rec["flags_shift"][0]) == CLOSED
    assert (ens.read_state()[0].tobytes(), ens.summaries(), bytes(ens.stats())) == before
    copy_of(ens, stage, nb, (b, s))
    key, phase, orientation, symmetry = stage.canon_phases([p])
    assert (int(rec["key"][0]), int(rec["phase"][0]), int(rec["orientation"][0]), int(rec["symmetry"][0])) == \
        (int(key[0]), int(phase[0]), int(orientation[0]), int(symmetry[0]))
    assert stage.summaries()[0].step == p and ens.summaries()[0].step == int(done[0])
    # a period that is not a multiple of the true one does not close
    odd, _ = call_and_check(ens, [reference(("oscillator", nb), state, rules, p + 1)], [p + 1])
    assert int(odd["flags_shift"][0]) == 0


@pytest.mark.parametrize("b", [1, 3])
def test_one_and_three_universes(ens, b):
    t = ship("a")
    states = [t[1], cc.state("shapes"), host.random_fill(W, seed=77, and_rounds=2)][:b]
    hold(ens, states)
    rules = moore_rules(*SHIP)
    periods = [4, 3, 2][:b]
    call_and_check(ens, [reference(("b", k), states[k], rules, periods[k]) for k in range(b)], periods)


def test_more_universes_than_compute_units_over_a_range(ens):
    """310 universes, canon_period over 7 .. 306: glider phases, small shapes, crafted states and a sparse soup in turn, periods 1 .. 4
    in turn; the result is indexed by universe - first. A smaller second call reuses the staging array."""
    t = ship("a")
    pool = [(("glider phase", k), t[k]) for k in range(4)]
    pool += [(("small", n), kc.shape_words(n)) for n in sorted(kc.SHAPES)]
    pool += [(("crafted", n), cc.state(n)) for n in ("shapes", "corners", "shell_core", "empty", "pairs2_+-+")]
    pool.append((("soup", 5), host.random_fill(W, seed=5, and_rounds=3)))
    marker = host.random_fill(W, seed=6, and_rounds=3)
    picks = [pool[(k * 7) % len(pool)] for k in range(300)]
    periods = [1 + (k * 3) % 4 for k in range(300)]
    ens.configure(310, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    ens.upload_state(0, np.stack([marker] * 7))
    ens.upload_state(7, np.stack([p[1] for p in picks]))
    ens.upload_state(307, np.stack([marker] * 3))
    rules = moore_rules(*SHIP)
    wants = [reference(p[0], p[1], rules, q) for p, q in zip(picks, periods)]
    call_and_check(ens, wants, periods, first=7)
    call_and_check(ens, wants[93:98], periods[93:98], first=100)


def test_canon_and_canon_period_share_the_staging_array(ens):
    """`canon` and `canon_period` stage in one array of the handle. On one handle of 8 universes — the glider's four phases, two small
    shapes and two crafted states — a `canon` of one universe (the smallest array), a `canon_period` of all with keys (grows it), a
    `canon` of all with digests (grows it again) and a `canon_period` of one (reuses it): every result is `host.canon`'s /
    `host.canon_period`'s."""
    t = ship("a")
    pool = [(("glider phase", k), t[k]) for k in range(4)]
    pool += [(("small", n), kc.shape_words(n)) for n in ("block", "rod")] + [(("crafted", n), cc.state(n)) for n in ("shapes", "corners")]
    hold(ens, [s for _, s in pool])
    rules = moore_rules(*SHIP)
    periods = np.array([4, 4, 4, 4, 1, 2, 3, 2], dtype=np.uint32)
    want_canon = [kc.reference(k, s) for k, s in pool]
    want_period = [reference(k, s, rules, int(p)) for (k, s), p in zip(pool, periods)]

    def same_period_record(got, k):
        for f in FIELDS:
            assert int(got[f]) == int(want_period[k][0][f]), (k, f, int(got[f]), int(want_period[k][0][f]))

    one = ens.canon(0, 1)
    assert one.shape == (1,)
    for f in ("key", "symmetry", "orientation", "population", "box_min", "box_max"):
        assert int(one[0][f]) == int(want_canon[0][0][f]), f
    rec, keys = ens.canon_period(periods, 0, 8, keys=True)
    assert rec.shape == (8,) and keys.shape == (8, 4)
    for k in range(8):
        same_period_record(rec[k], k)
        p = int(periods[k])
        np.testing.assert_array_equal(keys[k, :p], want_period[k][1], err_msg=f"universe {k}: keys")
        assert not keys[k, p:].any(), k
    rec, dig = ens.canon(0, 8, digests=True)
    for k in range(8):
        kc.assert_record(rec[k], dig[k], want_canon[k], pool[k][0])
    alone = ens.canon_period(periods[:1], 0, 1)
    assert alone.shape == (1,)
    same_period_record(alone[0], 0)


def test_ordering(ens):
    """A step queued and not waited for lies in front of the call: the result is that of the stepped states."""
    first = host.random_fill(W, seed=9, and_rounds=1)
    rules = moore_rules(*SHIP)
    hold(ens, [first, cc.state("shapes")])
    ens.step(3)  # queued, not synchronised
    rec, keys = ens.canon_period([2, 3], keys=True)
    stepped = [ol.packed_run(G, first, rules, 3), ol.packed_run(G, cc.state("shapes"), rules, 3)]
    for u, p in enumerate((2, 3)):
        want, want_keys = host.canon_period(phases(stepped[u], rules, p))
        np.testing.assert_array_equal(keys[u, :p], want_keys)
        assert [int(rec[u][f]) for f in FIELDS] == [int(want[f]) for f in FIELDS], u
    np.testing.assert_array_equal(ens.read_state(), np.stack(stepped))
    assert ens.summaries()[0].step == 3
    ens.step(1)  # and the ensemble goes on
    np.testing.assert_array_equal(ens.read_state()[0], ol.packed_step(G, stepped[0], rules))


def test_refusals(ens):
    lib = _capi.load()
    out = (_capi.CanonPeriodStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    keys = (C.c_uint64 * (4 * 8))(*([7] * (4 * 8)))
    good = (C.c_uint32 * 5)(4, 8, 1, 2, 3)
    ms = C.c_float(-1.0)

    def refused(code, pattern, handle, first, count, periods, out_, keys_=keys, stride=8):
        rc = lib.ca3d_ensemble_canon_period(handle, first, count, periods, out_, keys_, stride, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(keys) == [7] * (4 * 8) and ms.value == -1.0, msg

    refused(-1, "NULL", None, 0, 2, good, out)
    refused(-2, "configure", ens._h, 0, 2, good, out)  # an unconfigured handle
    ens.configure(4, neighbourhood="moore")
    refused(-1, "NULL", ens._h, 0, 2, good, None)
    refused(-1, "NULL", ens._h, 0, 2, None, out)
    refused(-2, "universe 0", ens._h, 0, 2, good, out)  # no state anywhere
    ens.upload_state(0, np.stack([cc.state("shapes")] * 2))
    refused(-2, "upload_state.*universe 2", ens._h, 1, 2, good, out)  # universe 2 has none
    ens.upload_state(2, np.stack([cc.state("corners")] * 2))
    refused(-2, "set_rules.*universe 0", ens._h, 0, 4, good, out)  # states everywhere, rules nowhere
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    ens.set_rule_strings(1, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    refused(-2, "set_rules.*universe 2", ens._h, 1, 2, good, out)  # universe 2 has none
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    before = (ens.read_state().tobytes(), ens.summaries(), bytes(ens.stats()))
    refused(-1, "universes", ens._h, 0, 0, good, out)  # count 0
    refused(-1, "universes", ens._h, 3, 2, good, out)  # a range past n
    refused(-1, "universes", ens._h, 4, 1, good, out)
    refused(-1, "universes", ens._h, 0, 5, good, out)
    refused(-1, r"periods\[1\]", ens._h, 0, 4, (C.c_uint32 * 4)(4, 0, 4, 4), out)  # a period of 0
    refused(-1, r"periods\[3\]", ens._h, 0, 4, (C.c_uint32 * 4)(4, 4, 4, host.CANON_MAX_PERIOD + 1), out)
    refused(-1, "keys_stride", ens._h, 0, 4, good, out, keys, 7)  # max(periods) is 8
    refused(-1, "keys_stride", ens._h, 0, 4, good, out, keys, 0)
    assert (ens.read_state().tobytes(), ens.summaries(), bytes(ens.stats())) == before
    with pytest.raises(Ca3dError) as e:
        ens.canon_period([4, 0, 4, 4])
    assert e.value.code == -1
    with pytest.raises(Ca3dError) as e:
        ens.canon_period(host.CANON_MAX_PERIOD + 1, keys=True)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ens.canon_period([4, 4])
    # keys and gpu_ms are nullable, and a stride without keys is not looked at
    assert lib.ca3d_ensemble_canon_period(ens._h, 0, 4, good, out, None, 0, None) == 0
    assert bytes(out) != b"\x5a" * C.sizeof(out) and list(keys) == [7] * (4 * 8)
    # a scalar period is every universe's
    np.testing.assert_array_equal(ens.canon_period(2), ens.canon_period([2, 2, 2, 2]))
    assert (ens.read_state().tobytes(), ens.summaries(), bytes(ens.stats())) == before
