"""`ca3d_ensemble_canon` on the GPU (kernel ca_ensemble_canon64, csrc/ca_canon.hip) against `host.canon`, the numpy restatement of the
definition in include/ca3d.h: every field of every record and all 48 digests, exactly. tests/test_canon_cpu.py checks `host.canon`
itself against a brute force. The crafted states are tests/census_cases.py's, the small shapes tests/canon_cases.py's."""
import ctypes as C
import re

import numpy as np
import pytest

import canon_cases as kc
import census_cases as cc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_cycle import MOORE as CYCLE_MOORE
from test_gpu_moving import SHIP, moore_rules, ship

pytestmark = pytest.mark.gpu

G, W = 64, 8192
FULL = (1 << 48) - 1
FIELDS = ("key", "symmetry", "orientation", "population", "box_min", "box_max")


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


def hold(e, states, nb="moore"):
    e.configure(len(states), neighbourhood=nb)
    e.upload_state(0, np.stack(states))


def canon_and_check(e, keys, states, first=0):
    """One call with digests over universes first .. first + len(states) - 1, against kc.reference(keys[k], states[k]); and once more
    without digests: the same records. -> (records, digests)"""
    n = len(states)
    rec, dig = e.canon(first, n, digests=True)
    assert rec.shape == (n,) and rec.dtype == host.CANON_DTYPE and dig.shape == (n, 48) and dig.dtype == np.uint64
    for k in range(n):
        kc.assert_record(rec[k], dig[k], kc.reference(keys[k], states[k]), keys[k])
    assert e.canon_gpu_ms() > 0.0
    alone = e.canon(first, n, digests=None)
    assert alone.tobytes() == rec.tobytes()
    return rec, dig


def test_every_crafted_state(ens):
    """The word seam at x = 31 | 32, the lane seams, the wave seams at z = 4 k, faces and corners, the serpentine and the staircase
    through all 16 waves, the full and the empty universe: every state of the census tests in one launch."""
    names = list(cc.CRAFTED)
    states = [cc.state(n) for n in names]
    hold(ens, states)
    rec, dig = canon_and_check(ens, [("crafted", n) for n in names], states)
    by = dict(zip(names, rec))
    assert [int(by["empty"][f]) for f in FIELDS] == [0, FULL, 0, 0, 0, 0] and not dig[names.index("empty")].any()
    assert int(by["full"]["symmetry"]) == FULL and int(by["full"]["orientation"]) == 0 and int(by["full"]["population"]) == 1 << 18
    assert int(by["full"]["key"]) == host.state_summary(G, cc.state("full"))["digest"]
    assert int(by["corners"]["symmetry"]) == FULL  # the eight corners of the cube
    assert len({int(by["shape_%d" % k]["key"]) for k in range(3)}) == 1  # one shape at three places


def test_small_shapes_and_their_groups(ens):
    """A cell and a block (48), a rod (16), a flat L (4), SHAPE (the identity alone, chiral) and the slab of extent 64 x 3 x 2, which
    turned lies along every lane and through every wave (8)."""
    names = sorted(kc.SHAPES)
    states = [kc.shape_words(n) for n in names]
    hold(ens, states)
    rec, _ = canon_and_check(ens, [("small", n) for n in names], states)
    for n, r in zip(names, rec):
        group = host.symmetry_orientations(r["symmetry"])
        assert len(group) == kc.SHAPES[n][1] and group[0] == 0, n
        assert host.is_chiral(r["symmetry"]) == (n == "shape"), n


def test_shape_in_all_48_orientations_at_three_places(ens, stage):
    """SHAPE turned by every orientation on the device and put at PLACES: 144 universes, one key. Composing universe u by
    orientation[u] to the origin gives a universe whose summary digest is the key."""
    sources = [cc.state("shape_%d" % k) for k in range(3)]
    hold(ens, sources)
    stage.configure(144, neighbourhood="moore")
    layouts = [[(k, o, cc.PLACES[k])] for k in range(3) for o in range(48)]
    made = stage.compose(layouts, 0, ens, False, False)
    assert not made["clipped"].any() and (made["population"] == len(cc.SHAPE)).all()
    states = list(stage.read_state())
    rec, dig = canon_and_check(stage, [("shape copy", k) for k in range(144)], states)
    assert len(set(rec["key"].tolist())) == 1 and int(rec["key"][0]) == int(kc.reference(("crafted", "shape_1"), cc.state("shape_1"))[0]["key"])
    assert (rec["symmetry"] == 1).all() and len(set(dig[:48, 0].tolist())) == 48
    ens.configure(144, neighbourhood="moore")
    ens.compose([[(u, int(rec["orientation"][u]), (0, 0, 0))] for u in range(144)], 0, stage, False, False)
    assert [s.digest for s in ens.summaries()] == rec["key"].tolist()


@pytest.mark.parametrize("b", [1, 3])
def test_one_and_three_universes(ens, b):
    names = ["shapes", "staircase", "shell_core"][:b]
    states = [cc.state(n) for n in names]
    hold(ens, states)
    canon_and_check(ens, [("crafted", n) for n in names], states)


def test_more_universes_than_compute_units_over_a_range(ens):
    """310 universes, canon over 7 .. 306: small shapes and crafted states in turn; the result is indexed by universe - first."""
    pool = [("small", n, kc.shape_words(n)) for n in sorted(kc.SHAPES)]
    pool += [("crafted", n, cc.state(n)) for n in ("shapes", "corners", "shell_core", "empty", "faces_z", "pairs2_+-+", "pairs1_0+-")]
    marker = host.random_fill(W, seed=5, and_rounds=3)
    picks = [pool[(k * 7) % len(pool)] for k in range(300)]
    ens.configure(310, neighbourhood="moore")
    ens.upload_state(0, np.stack([marker] * 7))
    ens.upload_state(7, np.stack([p[2] for p in picks]))
    ens.upload_state(307, np.stack([marker] * 3))
    canon_and_check(ens, [p[:2] for p in picks], [p[2] for p in picks], first=7)
    # a smaller call afterwards reuses the staging array
    canon_and_check(ens, [p[:2] for p in picks[93:98]], [p[2] for p in picks[93:98]], first=100)


def test_dense_soups(ens):
    """Eight dense soups, half and a quarter full: the forty orientations that do not keep x on x gather every row over all 64 x."""
    states = [host.random_fill(W, seed=21 + k, and_rounds=k % 2) for k in range(8)]
    hold(ens, states)
    rec, dig = canon_and_check(ens, [("soup", k) for k in range(8)], states)
    assert (rec["symmetry"] == 1).all() and all(len(set(d.tolist())) == 48 for d in dig)


def test_the_glider_in_48_orientations_and_4_phases(ens, stage):
    """The doubled glider of tests/test_gpu_moving.py (Moore B6/S5-7, period 4), its four phases from the oracle, each turned by every
    orientation on the device: 192 universes. `canon` is `host.canon` of each; `canon_phases` with periods 4 gives ONE key, the
    smallest over the phases, and leaves the ensemble four steps further. The glider has a mirror plane: it is not chiral."""
    t = ship("a")
    phases = [t[k] for k in range(4)]
    hold(ens, phases)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    stage.configure(192, neighbourhood="moore")
    stage.compose([[(k, o, (30, 30, 30))] for k in range(4) for o in range(48)], 0, ens, False, True)
    states = list(stage.read_state())
    rec, _ = canon_and_check(stage, [("glider", k) for k in range(192)], states)
    want = [kc.reference(("glider phase", k), phases[k])[0] for k in range(4)]
    for k in range(4):
        assert set(rec["key"][48 * k:48 * k + 48].tolist()) == {int(want[k]["key"])}, k
    _, _, sym, _ = kc.brute(phases[0])
    assert bin(sym).count("1") == 2 and int(want[0]["symmetry"]) == sym
    assert host.is_chiral(sym) == (not any(kc.mirrors(o) for o in host.symmetry_orientations(sym))) and not host.is_chiral(sym)
    for r in rec:
        assert len(host.symmetry_orientations(r["symmetry"])) == 2 and not host.is_chiral(r["symmetry"])
    key, phase, orientation, symmetry = stage.canon_phases(np.full(192, 4, dtype=np.uint32))
    smallest = min(int(w["key"]) for w in want)
    assert key.dtype == np.uint64 and phase.dtype == np.uint32 and orientation.dtype == np.uint32 and symmetry.dtype == np.uint64
    assert set(key.tolist()) == {smallest}
    for k in range(4):  # group k is in phase (k + t) % 4 in round t: the first round that reaches the key
        first = next(t for t in range(4) if int(want[(k + t) % 4]["key"]) == smallest)
        assert set(phase[48 * k:48 * k + 48].tolist()) == {first}, k
    assert stage.summaries(0, 1)[0].step == 4
    # a shorter period takes fewer rounds into account: period 1 is the key of the state as it lies
    now = stage.canon(0, 96)
    key1, phase1, _, _ = stage.canon_phases(np.array([1] * 48 + [4] * 48, dtype=np.uint32), 0, 96)
    assert key1[:48].tolist() == now["key"][:48].tolist() and not phase1[:48].any() and set(key1[48:].tolist()) == {smallest}


def test_an_oscillator_over_its_period(ens):
    """tests/test_gpu_cycle.py's Moore B5/S4,5 soup settles into a cycle of period 4: `canon_phases` over its period is the smallest
    `host.canon` key of the oracle's states, at the first phase that reaches it."""
    b, s, seed, rounds = CYCLE_MOORE[0]
    ens.configure(1, neighbourhood="moore")
    ens.set_rule_strings(0, neighbourhood="moore", born=b, survive=s)
    ens.upload_state(0, host.random_fill(W, seed=seed, and_rounds=rounds)[None])
    done, reason, period = ens.step_until_cycle(192, 1)
    p = int(period[0])
    assert p >= 2, (done, reason, period)
    state = ens.read_state()[0]
    rules = moore_rules(b, s)
    keys = []
    for k in range(p):
        keys.append(host.canon(state)[0])
        state = ol.packed_step(G, state, rules)
    key, phase, orientation, symmetry = ens.canon_phases([p])
    first = min(range(p), key=lambda k: (int(keys[k]["key"]), k))
    assert (int(key[0]), int(phase[0]), int(orientation[0]), int(symmetry[0])) == \
        (int(keys[first]["key"]), first, int(keys[first]["orientation"]), int(keys[first]["symmetry"]))
    np.testing.assert_array_equal(ens.read_state()[0], state)  # p steps further: the same phase again


def test_ash_becomes_a_catalogue(ens, stage):
    """Moore B6/S5-7 ash of eight soups through census and isolate ("origin") into a nursery, then canon: digests[:, 0] are the census
    digests, equal census digests have equal keys, and there are no more keys than census digests."""
    ens.configure(8, neighbourhood="moore")
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born="6", survive="5-7")
    ens.seed_states(0, np.arange(101, 109), 1)
    ens.step_until_cycle(512)
    comps, n, rest = ens.census(max_components=1024)
    assert not rest.any()
    jobs = [(u, int(c["first_cell"])) for u in range(8) for c in comps[u][:n[u]]]
    census_digests = np.array([int(c["digest"]) for u in range(8) for c in comps[u][:n[u]]], dtype=np.uint64)
    assert len(jobs) > 8
    stage.configure(len(jobs), neighbourhood="moore")
    stage.isolate(np.array(jobs, dtype=np.uint32), 0, ens, "origin", True)
    states = list(stage.read_state())
    rec, dig = canon_and_check(stage, [("ash", k) for k in range(len(jobs))], states)
    np.testing.assert_array_equal(dig[:, 0], census_digests)
    key_of = {}
    for d, k in zip(census_digests.tolist(), rec["key"].tolist()):
        assert key_of.setdefault(d, k) == k
    n_keys, n_digests = len(set(rec["key"].tolist())), len(set(census_digests.tolist()))
    print("ash objects %d, distinct census digests %d, distinct keys %d" % (len(jobs), n_digests, n_keys))
    assert n_keys <= n_digests
    assert rec["population"].tolist() == [int(c["population"]) for u in range(8) for c in comps[u][:n[u]]]


def test_ordering_and_read_only(ens):
    """A step queued and not waited for lies in front of the canon; the call changes neither states, records nor stats."""
    first = host.random_fill(W, seed=9, and_rounds=1)
    rules = moore_rules(*SHIP)
    hold(ens, [first, cc.state("shapes")])
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    ens.step(3)  # queued, not synchronised
    rec, dig = ens.canon(digests=True)
    stepped = [ol.packed_run(G, first, rules, 3), ol.packed_run(G, cc.state("shapes"), rules, 3)]
    for u in range(2):
        kc.assert_record(rec[u], dig[u], host.canon(stepped[u]), "after 3 steps, universe %d" % u)
    np.testing.assert_array_equal(ens.read_state(), np.stack(stepped))
    before = (ens.read_state().tobytes(), ens.summaries(), bytes(ens.stats()))
    ens.canon()
    ens.canon(1, 1, digests=True)
    assert (ens.read_state().tobytes(), ens.summaries(), bytes(ens.stats())) == before
    ens.step(1)  # and the ensemble goes on
    np.testing.assert_array_equal(ens.read_state()[0], ol.packed_step(G, stepped[0], rules))


def test_refusals(ens):
    lib = _capi.load()
    out = (_capi.CanonStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    dig = (C.c_uint64 * (4 * 48))(*([7] * (4 * 48)))
    ms = C.c_float(-1.0)

    def refused(code, pattern, handle, first, count, out_):
        rc = lib.ca3d_ensemble_canon(handle, first, count, out_, dig, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(dig) == [7] * (4 * 48) and ms.value == -1.0, msg

    refused(-1, "NULL", None, 0, 2, out)
    refused(-2, "configure", ens._h, 0, 2, out)  # an unconfigured handle
    ens.configure(4, neighbourhood="moore")
    refused(-1, "NULL", ens._h, 0, 2, None)
    refused(-2, "universe 0", ens._h, 0, 2, out)  # no state anywhere
    ens.upload_state(0, np.stack([cc.state("shapes")] * 2))
    refused(-2, "universe 2", ens._h, 1, 2, out)  # universe 2 has none
    ens.upload_state(2, np.stack([cc.state("corners")] * 2))
    before = (ens.read_state().tobytes(), ens.summaries())
    refused(-1, "universes", ens._h, 0, 0, out)  # count 0
    refused(-1, "universes", ens._h, 3, 2, out)  # a range past n
    refused(-1, "universes", ens._h, 4, 1, out)
    refused(-1, "universes", ens._h, 0, 5, out)
    assert (ens.read_state().tobytes(), ens.summaries()) == before
    with pytest.raises(Ca3dError) as e:
        ens.canon(3, 2)
    assert e.value.code == -1
    # canon_phases: both ValueErrors come before anything is queued
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    for bad, kw in (([4, 0, 4, 4], {}), ([4, 65, 4, 4], {}), ([4, 4, 4, 9], dict(max_period=8)), ([4, 4], {})):
        with pytest.raises(ValueError):
            ens.canon_phases(bad, **kw)
    assert (ens.read_state().tobytes(), ens.summaries()) == before
    assert lib.ca3d_ensemble_canon(ens._h, 0, 4, out, None, None) == 0  # digests and gpu_ms are nullable
    assert bytes(out) != b"\x5a" * C.sizeof(out) and list(dig) == [7] * (4 * 48)
