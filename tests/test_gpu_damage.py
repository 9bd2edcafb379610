"""`ca3d_ensemble_damage` on the GPU (the nine kernels of csrc/ca_damage.hip) against `host.damage`, the numpy restatement of the
definition in include/ca3d.h, fed with CPU trajectories (chains of `host.ensemble_step`, which tests/test_ensemble_boundary_cpu.py pins
to the CPU oracle): every field of every record, every word of every curve and every word of every image, exactly.
tests/test_damage_cpu.py checks `host.damage` itself against a brute force. Universes are 64^3 by construction."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import census_cases as cc
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_envelope import SHIP_TABLES, hold, make_ensemble, mask, snapshot

pytestmark = pytest.mark.gpu

G, W = 64, 8192
KINDS = ("von neumann", "moore", "clustered")
NEVER, HEALED, SELF = host.DAMAGE_NEVER, host.DAMAGE_HEALED, host.DAMAGE_SELF
EMPTY = np.zeros(W, dtype=np.uint32)
FULL = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
_u32p = C.POINTER(C.c_uint32)


def plain(kind, born, survive):
    """The tables born / survive of the kind; clustered: the same pair in all three classes, cut to each class's counts."""
    if kind != "clustered":
        return (born, survive)
    return (tuple(born & ((1 << n) - 1) for n in (27, 13, 9)), tuple(survive & ((1 << n) - 1) for n in (27, 13, 9)))


def grow(kind):
    """Born at count 1, survive at 0 and 2 (clustered: in all three classes): a single cell spreads through every face it touches."""
    return plain(kind, 1 << 1, 0b101)


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


_CHAINS, _WANT = {}, {}


def chain(key, state, kind, tables, boundary, p):
    """S_0 .. S_p of `state` under host.ensemble_step, kept for the run under (key, kind, boundary): `key` names state and rule."""
    t = _CHAINS.setdefault((key, kind, boundary), [np.ascontiguousarray(state, dtype=np.uint32)])
    assert np.array_equal(t[0], state), key
    while len(t) <= p:
        t.append(host.ensemble_step(t[-1], kind, tables, boundary))
    return np.stack(t[:p + 1])


def want(key, state, kind, tables, p, boundary="reference", twin=None, flips=()):
    """`host.damage` of the two CPU trajectories: (curve, record, D_P), computed once and left unchanged. `key` names state, twin,
    flips and rule."""
    full = (key, kind, boundary, p)
    if full not in _WANT:
        first = host.damage_twin(state, twin, flips)
        out = host.damage_of_phases(chain((key, "S"), state, kind, tables, boundary, p), chain((key, "T"), first, kind, tables, boundary, p))
        for a in out:
            a.setflags(write=False)
        _WANT[full] = out
    return _WANT[full]


def same_record(got, exp, where):
    for f in host.DAMAGE_DTYPE.names:
        assert np.array_equal(got[f], exp[f]), (where, f, got[f], exp[f])
    assert got.tobytes() == exp.tobytes(), where


def check_all(rec, curve, wants, where=""):
    """Records and curve rows of one call against wants[k] of `want`; the curve's columns behind steps[k] are zero."""
    assert rec.shape == (len(wants),) and rec.dtype == host.DAMAGE_DTYPE
    for k, w in enumerate(wants):
        same_record(rec[k], w[1], (where, k))
        if curve is not None:
            n = len(w[0])
            assert curve[k, :n].tolist() == w[0].tolist(), (where, k, curve[k].tolist(), w[0].tolist())
            assert not curve[k, n:].any(), (where, k)


# ---------------------------------------------------------------------------------------------- a lone flip

#: the eight corners; astride the word seam x = 31 | 32; astride the wave seams z = 3 | 4 and 59 | 60; the lane ends y = 0 and 63
LONE = list(itertools.product((0, 63), repeat=3)) + [(31, 20, 20), (32, 20, 20), (20, 20, 3), (20, 20, 4), (20, 20, 59), (20, 20, 60),
                                                     (20, 0, 20), (20, 63, 20)]


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_lone_flip_in_an_empty_universe(ens, kind, boundary):
    """The difference is the single-cell evolution under born-at-1, so every wrong face, seam or lane end shows: 16 cells x P = 1 .. 6
    in one launch, records and curves."""
    tables = grow(kind)
    jobs = [(cell, p) for cell in LONE for p in range(1, 7)]
    hold(ens, kind, tables, [EMPTY] * len(jobs), boundary)
    before = snapshot(ens)
    rec, curve = ens.damage([p for _, p in jobs], flips=[[cell] for cell, _ in jobs], curve=True)
    assert curve.shape == (len(jobs), 7) and ens.damage_gpu_ms() > 0.0
    wants = [want(("lone", cell), EMPTY, kind, tables, p, boundary, flips=[cell]) for cell, p in jobs]
    check_all(rec, curve, wants, (kind, boundary))
    assert (rec["initial_distance"] == 1).all() and (rec["max_distance"] > 1).all()
    assert snapshot(ens) == before


@pytest.mark.parametrize("kind", KINDS)
def test_the_boundaries_give_different_curves(ens, kind):
    """A + face wraps in reference mode and a - face is dead: the cell in the corner (0, 0, 0) is seen through three faces on a torus
    and in reference mode and through none in a closed cube, the cell in the corner (63, 63, 63) on a torus alone. The mode is the
    ensemble's CURRENT one: it is switched between the calls."""
    tables = grow(kind)
    cells = [(0, 0, 0), (63, 63, 63)]
    hold(ens, kind, tables, [EMPTY] * 2)
    got = {}
    for boundary in host.ENSEMBLE_BOUNDARIES:
        ens.set_boundary(boundary)
        rec, curve = ens.damage(6, flips=[[c] for c in cells], curve=True)
        check_all(rec, curve, [want(("lone", c), EMPTY, kind, tables, 6, boundary, flips=[c]) for c in cells], boundary)
        got[boundary] = curve.tolist()
    assert got["reference"][0] != got["closed"][0] and got["reference"][1] == got["closed"][1] != got["torus"][1], got
    assert len({str(v) for v in got.values()}) == 3


# ---------------------------------------------------------------------------------------------- healing

@pytest.mark.parametrize("kind", ("von neumann", "moore"))
def test_the_healing_row(ens, kind):
    """B none / S2: the end cells of a straight row die every step, 9, 7, 5, 3, 1, 0. The row as a twin UNIVERSE against an empty source,
    along x across the word seam and along z across a wave seam; three flips in a row heal at 2. The curve is zero to the stride's end
    and the image of D_P is empty."""
    tables = plain(kind, 0, 1 << 2)
    row_x = host.cells_to_words(G, [(28 + i, 20, 26) for i in range(9)])
    row_z = host.cells_to_words(G, [(20, 23, 28 + i) for i in range(9)])
    three = [(30 + i, 5, 7) for i in range(3)]
    marker = host.random_fill(W, seed=6, and_rounds=3)
    hold(ens, kind, tables, [EMPTY, EMPTY, EMPTY, row_x, row_z, marker, marker, marker])
    rec, curve = ens.damage([7, 9, 4], twins=[3, 4, SELF], flips=[[], [], three], dst=ens, dst_first=5, image=True, curve=True)
    wants = [want("row x", EMPTY, kind, tables, 7, twin=row_x), want("row z", EMPTY, kind, tables, 9, twin=row_z),
             want("three", EMPTY, kind, tables, 4, flips=three)]
    check_all(rec, curve, wants, kind)
    assert curve.shape == (3, 10)
    assert curve[0].tolist() == [9, 7, 5, 3, 1, 0, 0, 0, 0, 0] and curve[1].tolist() == curve[0].tolist() and curve[2].tolist() == [3, 1] + [0] * 8
    assert rec["healed_at"].tolist() == [5, 5, 2] and rec["flags"].tolist() == [HEALED] * 3 and rec["distance_sum"].tolist() == [25, 25, 4]
    assert tuple(rec["touched_min"][0]) == (28, 20, 26, 0) and tuple(rec["touched_max"][0]) == (36, 20, 26, 0)
    assert tuple(rec["touched_min"][1]) == (20, 23, 28, 0) and tuple(rec["touched_max"][1]) == (20, 23, 36, 0)
    assert not ens.read_state(5, 3).any()  # the markers are gone: D_P is empty
    np.testing.assert_array_equal(ens.read_state(0, 5), np.stack([EMPTY, EMPTY, EMPTY, row_x, row_z]))
    # healed exactly at P, and one step short of it
    rec = ens.damage([5, 4], twins=[3, 4])
    check_all(rec, None, [want("row x", EMPTY, kind, tables, 5, twin=row_x), want("row z", EMPTY, kind, tables, 4, twin=row_z)])
    assert rec["healed_at"].tolist() == [5, NEVER] and rec["flags"].tolist() == [HEALED, 0] and rec["final_distance"].tolist() == [0, 1]


@pytest.mark.parametrize("kind", ("von neumann", "clustered"))
def test_full_against_empty_at_the_longest(ens, kind):
    """B none / S all: the empty source stays empty, the all-ones twin full: d_t = 262 144 at every t. At P = 4096 every wave's partial
    is at its largest and distance_sum = 262 144 x 4 097 = 1 074 003 968 is near a word's end. One source universe."""
    tables = plain(kind, 0, (1 << 27) - 1 if kind == "clustered" else (1 << 7) - 1)
    hold(ens, kind, tables, [EMPTY, FULL])
    exp = host.damage(EMPTY, kind, tables, 4096, twin=FULL)  # (two still lifes: it stops stepping at once)
    assert int(exp[1]["distance_sum"]) == 1074003968 and int(exp[1]["healed_at"]) == NEVER and int(exp[1]["max_at"]) == 0
    rec, curve = ens.damage([4096], twins=[1], curve=True)
    check_all(rec, curve, [exp], kind)
    assert int(rec["distance_sum"][0]) == 1074003968 and curve.shape == (1, 4097) and (curve == 1 << 18).all()
    assert tuple(rec["damage_max"][0]) == tuple(rec["touched_max"][0]) == (63, 63, 63, 0)
    np.testing.assert_array_equal(ens.read_state(), np.stack([EMPTY, FULL]))


# ---------------------------------------------------------------------------------------------- soups

def soup_rule(kind):
    """A rule under which one flipped cell spreads in dense and in thin soups alike (on the CPU: 1, 4, 28, 64, 107, 242, 306 in a soup of
    density 1/2 under the Moore one): Moore B4-6/S5-9, the same with edges and corners tables of their own, von Neumann B3/S2-4."""
    if kind == "von neumann":
        return (mask("3", 7), mask("2-4", 7))
    if kind == "moore":
        return (mask("4-6"), mask("5-9"))
    return ((mask("4-6"), mask("6", 13), mask("4", 9)), (mask("5-9"), mask("5-7", 13), mask("3-5", 9)))


def flip_of(k):
    """A cell that depends on k alone, off no particular seam."""
    r = np.random.default_rng(1000 + k)
    return tuple(int(v) for v in r.integers(0, 64, 3))


@pytest.mark.parametrize("kind", KINDS)
def test_steps_that_differ_inside_one_launch(ens, kind):
    """Dense soups with one random flip each and P of 1, 2, 3, 4, 8 and 5 in one launch; the curve with its tightest stride, with a
    wide one whose every word is written, and not at all."""
    tables = soup_rule(kind)
    states = [host.random_fill(W, seed=50 + k) for k in range(6)]
    steps = [1, 2, 3, 4, 8, 5]
    flips = [[flip_of(k)] for k in range(6)]
    hold(ens, kind, tables, states)
    wants = [want(("soup", k), states[k], kind, tables, steps[k], flips=flips[k]) for k in range(6)]
    before = snapshot(ens)
    rec, curve = ens.damage(steps, flips=flips, curve=True)
    check_all(rec, curve, wants, kind)
    assert curve.shape == (6, 9) and int(rec["final_distance"][4]) > 1  # the damage spreads
    check_all(ens.damage(steps, flips=flips), None, wants, kind)  # curve NULL
    # a wide stride through the C entry point: every word of the array is written
    lib = _capi.load()
    stride = 21
    wide = np.full((6, stride), 0x5A5A5A5A, dtype=np.uint32)
    out = np.zeros(6, dtype=host.DAMAGE_DTYPE)
    fl = np.full((6, 4), host.DAMAGE_NO_FLIP, dtype=np.uint32)
    fl[:, 0] = [host.damage_flip_word(f[0]) for f in flips]
    p = np.array(steps, dtype=np.uint32)
    assert lib.ca3d_ensemble_damage(ens._h, 0, 6, p.ctypes.data_as(_u32p), None, fl.ctypes.data_as(_u32p), None, 0, 0,
                                    out.ctypes.data_as(C.POINTER(_capi.DamageStruct)), wide.ctypes.data_as(_u32p), stride, None) == 0
    check_all(out, wide, wants, (kind, "wide"))
    assert snapshot(ens) == before


@pytest.mark.parametrize("b", [1, 3])
def test_one_and_three_universes(ens, b):
    tables = soup_rule("moore")
    states = [host.random_fill(W, seed=50 + k) for k in range(b)]
    steps = [4, 3, 2][:b]
    flips = [[flip_of(k)] for k in range(b)]
    hold(ens, "moore", tables, states)
    rec, curve = ens.damage(steps, flips=flips, curve=True)
    check_all(rec, curve, [want(("soup", k), states[k], "moore", tables, steps[k], flips=flips[k]) for k in range(b)], b)


def test_more_universes_than_compute_units_over_a_range(ens, nursery):
    """310 universes, damage over 7 .. 306 with 1 .. 4 steps in turn, the images into a second ensemble of 300."""
    tables = soup_rule("moore")
    pool = [host.random_fill(W, seed=50 + k) for k in range(4)] + [host.random_fill(W, seed=60 + k, and_rounds=2) for k in range(3)]
    marker = host.random_fill(W, seed=6, and_rounds=3)
    picks = [(k * 5) % len(pool) for k in range(300)]
    steps = [1 + (k * 3) % 4 for k in range(300)]
    hold(ens, "moore", tables, [marker] * 7 + [pool[i] for i in picks] + [marker] * 3)
    nursery.configure(300, neighbourhood="moore")
    wants = [want(("pool", i), pool[i], "moore", tables, p, flips=[flip_of(i)]) for i, p in zip(picks, steps)]
    before = snapshot(ens)
    rec, curve = ens.damage(steps, first=7, flips=[[flip_of(i)] for i in picks], dst=nursery, image=True, curve=True)
    check_all(rec, curve, wants, "300 of 310")
    got = nursery.read_state()
    for k in range(300):
        np.testing.assert_array_equal(got[k], wants[k][2], err_msg=f"image {k}")
    assert snapshot(ens) == before
    assert [s.step for s in nursery.summaries(0, 3)] == [0, 0, 0]
    # a smaller second call reuses the staging array
    again = ens.damage(steps[93:98], first=100, flips=[[flip_of(i)] for i in picks[93:98]])
    assert again.tobytes() == rec[93:98].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_twins(ens, kind):
    """Every twin pointing at one shared universe, with and without flips on top; a twin named as the universe itself, and
    CA3D_DAMAGE_SELF, with no flips: no perturbation, healed at 0. A twin's rule is never read: the shared universe has another."""
    tables = soup_rule(kind)
    states = [host.random_fill(W, seed=70 + k, and_rounds=1) for k in range(4)]
    shared = host.random_fill(W, seed=80, and_rounds=1)
    silent = plain(kind, 0, 0)
    hold(ens, kind, [tables] * 4 + [silent], states + [shared])
    flips = [[], [flip_of(1)], [flip_of(2), flip_of(3)], []]
    before = snapshot(ens)
    rec, curve = ens.damage([3] * 4, twins=[4] * 4, flips=flips, curve=True)
    check_all(rec, curve, [want(("shared", k), states[k], kind, tables, 3, twin=shared, flips=flips[k]) for k in range(4)], kind)
    assert (rec["initial_distance"] > 1000).all()
    rec, curve = ens.damage([3] * 4, twins=[0, SELF, 2, SELF], curve=True)
    assert not curve.any() and rec["healed_at"].tolist() == [0] * 4 and rec["flags"].tolist() == [HEALED] * 4
    for k in range(4):
        same_record(rec[k], want(("itself", k), states[k], kind, tables, 3)[1], k)
    assert snapshot(ens) == before


# ---------------------------------------------------------------------------------------------- the image

@pytest.mark.parametrize("kind", KINDS)
def test_the_image(ens, nursery, kind):
    """Rules of 1, 2 and 6 words. first = 5 in an ensemble of 16: D_P of source k lands in universe dst_first + k of a second ensemble,
    in both buffers (a step from either parity is the CPU's), with records at step 0; COPY_RULES brings the source's rule, and without it
    the destination keeps its own. Then into the same ensemble, and a census of the damaged regions."""
    tables = soup_rule(kind)
    states = [host.random_fill(W, seed=90 + k, and_rounds=(0, 1, 0)[k]) for k in range(3)]
    marker = host.random_fill(W, seed=6, and_rounds=3)
    hold(ens, kind, tables, [marker] * 5 + states + [marker] * 8)
    steps, flips = [2, 3, 1], [[flip_of(k)] for k in range(3)]
    wants = [want(("image", k), states[k], kind, tables, steps[k], flips=flips[k]) for k in range(3)]
    silent = plain(kind, 0, 0)  # nothing is born, nothing survives
    before = snapshot(ens)
    for copy_rules in (True, False):
        hold(nursery, kind, silent, [marker] * 7)
        rec = ens.damage(steps, first=5, flips=flips, dst=nursery, dst_first=2, image=True, copy_rules=copy_rules)
        check_all(rec, None, wants, (kind, copy_rules))
        got = nursery.read_state()
        for k in range(3):
            np.testing.assert_array_equal(got[2 + k], wants[k][2], err_msg=f"image {k}")
        np.testing.assert_array_equal(got[[0, 1, 5, 6]], np.stack([marker] * 4))
        for k, s in enumerate(nursery.summaries(2, 3)):
            assert s.step == 0 and not s.has_previous and (s.births, s.deaths) == (0, 0), k
            assert s.population == int(rec["final_distance"][k]), k
        # one step from the buffer the image was written to, one more from the other one
        rule = tables if copy_rules else silent
        one = host.ensemble_step(wants[1][2], kind, rule)
        nursery.step(1)
        np.testing.assert_array_equal(nursery.read_state(3, 1)[0], one, err_msg=f"{copy_rules}: step 1")
        nursery.step(1)
        np.testing.assert_array_equal(nursery.read_state(3, 1)[0], host.ensemble_step(one, kind, rule), err_msg=f"{copy_rules}: step 2")
        s = nursery.summaries(3, 1)[0]
        assert s.step == 2 and s.has_previous
    assert snapshot(ens) == before
    # into the same ensemble, behind the sources; the census of an image is host.census of D_P
    rec = ens.damage(steps, first=5, flips=flips, dst=ens, dst_first=9, image=True, copy_rules=True)
    check_all(rec, None, wants, (kind, "same"))
    np.testing.assert_array_equal(ens.read_state(5, 3), np.stack(states))
    np.testing.assert_array_equal(ens.read_state(9, 3), np.stack([w[2] for w in wants]))
    comps, n, rest = ens.census(9, 3, max_components=16)
    for k in range(3):
        exp, exp_n, exp_rest = host.census(wants[k][2], 16)
        assert (int(n[k]), int(rest[k])) == (exp_n, exp_rest), k
        assert comps[k].tobytes() == exp.tobytes(), k
    assert int(n[2]) >= 1


def test_ordering(ens, nursery):
    """A step queued and not waited for lies in front of the call; the image into a destination that has work queued on its own stream
    comes behind that work, and a step of the destination queued behind the call sees the image."""
    tables = soup_rule("moore")
    states = [host.random_fill(W, seed=50), host.random_fill(W, seed=61, and_rounds=2)]
    hold(ens, "moore", tables, states)
    hold(nursery, "moore", tables, [states[0]] * 2)
    ens.step(3)  # queued, not synchronised
    nursery.step(2)  # on the other stream, likewise
    flips = [[flip_of(0)], [flip_of(1)]]
    rec, curve = ens.damage([2, 3], flips=flips, dst=nursery, image=True, curve=True)
    nursery.step(1)
    stepped = [chain(("ordering", k), states[k], "moore", tables, "reference", 3)[3] for k in range(2)]
    wants = [want(("ordering stepped", k), stepped[k], "moore", tables, p, flips=flips[k]) for k, p in enumerate((2, 3))]
    check_all(rec, curve, wants, "ordering")
    got = nursery.read_state()
    for k in range(2):
        np.testing.assert_array_equal(got[k], host.ensemble_step(wants[k][2], "moore", tables), err_msg=str(k))
    np.testing.assert_array_equal(ens.read_state(), np.stack(stepped))
    assert ens.summaries()[0].step == 3 and nursery.summaries()[0].step == 1
    ens.step(1)  # and the source goes on
    np.testing.assert_array_equal(ens.read_state()[0], host.ensemble_step(stepped[0], "moore", tables))


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals(ens, nursery):
    lib = _capi.load()
    out = (_capi.DamageStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    curve = (C.c_uint32 * 40)(*([0x5A5A5A5A] * 40))
    good = (C.c_uint32 * 5)(4, 8, 1, 2, 3)
    ms = C.c_float(-1.0)
    IMAGE, COPY = _capi.DAMAGE_IMAGE_DAMAGE, _capi.DAMAGE_COPY_RULES

    def u32(*v):
        return (C.c_uint32 * len(v))(*v)

    def refused(code, pattern, src, first, count, steps, twins=None, flips=None, dst=None, dst_first=0, flags=0, out_=out, curve_=None, stride=0):
        rc = lib.ca3d_ensemble_damage(src, first, count, steps, twins, flips, dst, dst_first, flags, out_, curve_, stride, C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and list(good) == [4, 8, 1, 2, 3] and ms.value == -1.0, msg
        assert list(curve) == [0x5A5A5A5A] * 40, msg

    refused(-1, "NULL", None, 0, 2, good)
    refused(-2, "configure", ens._h, 0, 2, good)  # an unconfigured handle
    ens.configure(8, neighbourhood="moore")
    refused(-1, "out is NULL", ens._h, 0, 2, good, out_=None)
    refused(-1, "steps is NULL", ens._h, 0, 2, None)
    refused(-2, "upload_state.*universe 0", ens._h, 0, 2, good)  # no state anywhere
    ens.upload_state(0, np.stack([cc.state("shapes")] * 2))
    refused(-2, "upload_state.*universe 2", ens._h, 1, 2, good)  # universe 2 has none
    refused(-2, r"twins\[1\].*upload_state.*universe 5", ens._h, 0, 2, good, twins=u32(SELF, 5))  # nor has the twin
    ens.upload_state(2, np.stack([cc.state("corners")] * 6))
    refused(-2, "set_rules.*universe 0", ens._h, 0, 4, good)  # states everywhere, rules nowhere
    ens.set_rule_tables(0, [SHIP_TABLES[0]] * 2, [SHIP_TABLES[1]] * 2)
    refused(-2, "set_rules.*universe 2", ens._h, 1, 2, good)  # universe 2 has none
    # a twin's rule is never read: universe 7 has none
    assert lib.ca3d_ensemble_damage(ens._h, 0, 2, good, u32(7, 7), None, None, 0, 0, out, None, 0, None) == 0
    C.memset(out, 0x5A, C.sizeof(out))
    ens.set_rule_tables(0, [SHIP_TABLES[0]] * 8, [SHIP_TABLES[1]] * 8)
    refused(-2, "configure.*destination", ens._h, 0, 2, good, dst=nursery._h, flags=IMAGE)  # an unconfigured destination
    nursery.configure(6, neighbourhood="von neumann")
    nursery.upload_state(0, np.stack([cc.state("shapes")] * 6))
    before = (snapshot(ens), nursery.read_state().tobytes())
    refused(-1, "universes", ens._h, 0, 0, good)  # count 0
    refused(-1, "universes", ens._h, 7, 2, good)  # a range past n
    refused(-1, "universes", ens._h, 8, 1, good)
    refused(-1, "universes", ens._h, 0, 9, good)
    refused(-1, r"steps\[1\].*universe 3", ens._h, 2, 4, u32(4, 0, 4, 4))  # a step count of 0
    refused(-1, r"steps\[3\].*universe 3", ens._h, 0, 4, u32(4, 4, 4, host.CANON_MAX_PERIOD + 1))
    refused(-1, r"twins\[2\] is 8 \(universe 3\)", ens._h, 1, 3, good, twins=u32(0, SELF, 8))  # a twin outside the ensemble
    none = host.DAMAGE_NO_FLIP
    refused(-1, r"flips\[1\]\[2\] is 0x40 \(universe 2\)", ens._h, 1, 2, good, flips=u32(0, none, none, none, 1, none, 64, none))  # x = 64
    refused(-1, r"flips\[0\]\[0\].*universe 0", ens._h, 0, 1, good, flips=u32(0x4000, none, none, none))  # y = 64
    refused(-1, r"flips\[0\]\[1\].*universe 0", ens._h, 0, 1, good, flips=u32(0, 0x400000, none, none))  # z = 64
    refused(-1, r"flips\[0\]\[3\].*universe 0", ens._h, 0, 1, good, flips=u32(0, 0, 0, 0x01000000))  # a top byte
    refused(-1, "curve_stride is 8", ens._h, 0, 2, good, curve_=curve, stride=8)  # max(steps) = 8 needs 9
    refused(-1, "unknown bits", ens._h, 0, 2, good, flags=2)
    refused(-1, "unknown bits", ens._h, 0, 2, good, dst=nursery._h, flags=IMAGE | 0x200)
    refused(-1, "dst is NULL", ens._h, 0, 2, good, flags=IMAGE)  # the image bit without a destination
    refused(-1, "no image", ens._h, 0, 2, good, dst=nursery._h)  # a destination without the image bit
    refused(-1, "no image", ens._h, 0, 2, good, flags=COPY)  # rules to copy and nowhere to
    refused(-1, "images into universes", ens._h, 0, 4, good, dst=nursery._h, dst_first=3, flags=IMAGE)  # 3 + 4 of 6
    refused(-1, "images into universes", ens._h, 0, 2, good, dst=nursery._h, dst_first=6, flags=IMAGE)
    refused(-1, "source universe 3 lies among the destinations", ens._h, 0, 4, good, dst=ens._h, dst_first=3, flags=IMAGE)  # the same ensemble
    refused(-1, "source universe 2 lies among the destinations", ens._h, 2, 2, good, dst=ens._h, dst_first=1, flags=IMAGE)
    refused(-1, "twin 1: source universe 5 lies among the destinations", ens._h, 0, 2, good, twins=u32(SELF, 5), dst=ens._h, dst_first=4, flags=IMAGE)
    refused(-5, "CA3D_DAMAGE_COPY_RULES.*neighbourhood", ens._h, 0, 2, good, dst=nursery._h, flags=IMAGE | COPY)  # Moore into von Neumann
    assert (snapshot(ens), nursery.read_state().tobytes()) == before
    with pytest.raises(Ca3dError) as e:
        ens.damage([4, 0, 4, 4])
    assert e.value.code == -1
    with pytest.raises(Ca3dError) as e:
        ens.damage(4, image=True)  # no dst
    assert e.value.code == -1
    with pytest.raises(ValueError):
        ens.damage([4, 4], flips=[[(0, 0, 64)], []])
    with pytest.raises(ValueError):
        ens.damage([4, 4], flips=[[(0, 0, 0)] * 5, []])
    # gpu_ms is nullable; without COPY_RULES the kinds may differ; the destinations right behind the sources are fine; a stride of
    # max(steps) + 1 is enough, and the stride is not looked at without a curve
    assert lib.ca3d_ensemble_damage(ens._h, 0, 4, good, None, None, None, 0, 0, out, None, 0, None) == 0
    assert bytes(out) != b"\x5a" * C.sizeof(out)
    assert lib.ca3d_ensemble_damage(ens._h, 0, 2, good, None, None, nursery._h, 2, IMAGE, out, None, 0, None) == 0
    assert lib.ca3d_ensemble_damage(ens._h, 0, 4, good, u32(4, 5, 6, 7), None, ens._h, 4, IMAGE, out, None, 0, None) == -1  # twins among them
    assert lib.ca3d_ensemble_damage(ens._h, 0, 2, good, u32(2, 3), None, ens._h, 4, IMAGE, out, None, 0, None) == 0
    assert lib.ca3d_ensemble_damage(ens._h, 0, 2, good, None, None, None, 0, 0, out, curve, 9, None) == 0
    assert list(curve)[18:] == [0x5A5A5A5A] * 22 and list(curve)[:18] == [0] * 18  # no perturbation: two rows of nine zeros
    # a scalar step count is that of every universe from `first` on; one cell for every universe
    np.testing.assert_array_equal(ens.damage(2, first=6), ens.damage([2, 2], first=6))
    np.testing.assert_array_equal(ens.damage(2, first=6, flips=(1, 2, 3)), ens.damage([2, 2], first=6, flips=[[(1, 2, 3)]] * 2))
