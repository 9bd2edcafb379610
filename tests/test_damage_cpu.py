"""The host side of damage spreading (`ca3d_ensemble_damage`, include/ca3d.h): `host.damage`, the numpy restatement of the definition,
against a brute force that does not go through it — a state and its perturbed twin stepped as two trajectories by the CPU oracle
(tests/test_ensemble_boundary_cpu.py's `oracle_states`: the packed oracle in reference mode, the unpacked one on a torus and inside a
128^3 array in closed mode), unpacked and compared cell by cell —; closed forms; the symbol, the struct and the Python and JS
surfaces. All comparisons are exact. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graded_lib as gl
from cellularautomatons3d_amd import _capi, host
from cellularautomatons3d_amd.ensemble import Ensemble
from test_ensemble_boundary_cpu import grow_rule, oracle_states, rule_of, tables_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, W = 64, 8192
KINDS = ("von neumann", "moore", "clustered")
NEVER = host.DAMAGE_NEVER


def cells(words):
    return gl.unpack(G, words).astype(bool)  # [z, y, x]


def box(c):
    """(min, max) as (x, y, z, 0) of a [z, y, x] cell array; zeros for an empty one."""
    if not c.any():
        return (0, 0, 0, 0), (0, 0, 0, 0)
    idx = [np.flatnonzero(c.any(axis=ax)) for ax in ((0, 1), (0, 2), (1, 2))]  # x, y, z
    return tuple(int(i[0]) for i in idx) + (0,), tuple(int(i[-1]) for i in idx) + (0,)


def brute(kind, rule, boundary, state, steps, twin=None, flips=()):
    """Curve, record fields and D_P by the definition: both trajectories from the oracle, every comparison cell by cell."""
    t0 = cells(state if twin is None else twin).copy()
    for x, y, z in flips:
        t0[z, y, x] ^= True
    chains = [[np.ascontiguousarray(first, dtype=np.uint32)] + oracle_states(kind, rule, boundary, first, steps) for first in (state, gl.pack(G, t0))]
    s, t = ([cells(w) for w in chain] for chain in chains)
    d = [a != b for a, b in zip(s, t)]
    curve = [int(x.sum()) for x in d]
    zeros = [i for i, v in enumerate(curve) if v == 0]
    touched = np.logical_or.reduce(d)
    want = {"steps": steps, "flags": 1 if zeros else 0, "healed_at": zeros[0] if zeros else NEVER, "final_distance": curve[-1],
            "initial_distance": curve[0], "max_distance": max(curve), "max_at": curve.index(max(curve)), "distance_sum": sum(curve),
            "damage_min": box(d[-1])[0], "damage_max": box(d[-1])[1], "touched_min": box(touched)[0], "touched_max": box(touched)[1]}
    return curve, want, gl.pack(G, d[-1]), chains


def as_dict(rec):
    return {n: (int(rec[n]) if rec[n].ndim == 0 else tuple(int(v) for v in rec[n])) for n in rec.dtype.names}


def check(kind, rule, boundary, state, steps, twin=None, flips=(), what=""):
    curve, rec, last = host.damage(state, kind, tables_of(kind, rule), steps, boundary, twin=twin, flips=flips)
    wcurve, want, wlast, chains = brute(kind, rule, boundary, state, steps, twin, flips)
    assert rec.dtype == host.DAMAGE_DTYPE and rec.shape == () and curve.dtype == np.uint32 and curve.shape == (steps + 1,), what
    assert curve.tolist() == wcurve, what
    assert as_dict(rec) == want, what
    assert last.dtype == np.uint32 and last.shape == (W,) and np.array_equal(last, wlast), what
    # and over the same two trajectories, already stepped
    curve2, rec2, last2 = host.damage_of_phases(np.stack(chains[0]), np.stack(chains[1]))
    assert curve2.tolist() == wcurve and as_dict(rec2) == want and np.array_equal(last2, wlast), what
    assert np.array_equal(host.damage_twin(state, twin, flips), chains[1][0]), what
    return curve, rec, last


def plain(kind, born, survive):
    """The rule born / survive (masks) of the kind; clustered: in the main class, the side classes silent."""
    r = gl._rule("plain", born, survive)
    return gl.clustered("main", r) if kind == "clustered" else r


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", KINDS)
def test_soups_against_two_oracle_trajectories(kind, boundary):
    """A dense soup (density 1/2) with one flip and a sparse one (2^-4) with three, under coded rules; the flips lie on a corner, on the
    word seam and on a wave seam."""
    dense, sparse = host.seeded_state(G, 21, 0), host.seeded_state(G, 22, 3)
    _, rec, _ = check(kind, rule_of(kind, 1), boundary, dense, 3, flips=[(31, 63, 4)], what=(kind, boundary, "dense"))
    assert int(rec["initial_distance"]) == 1 and tuple(rec["touched_min"]) != tuple(rec["touched_max"])
    check(kind, rule_of(kind, 2), boundary, sparse, 2, flips=[(0, 0, 0), (32, 20, 59), (63, 63, 63)], what=(kind, boundary, "sparse"))


@pytest.mark.parametrize("kind", KINDS)
def test_twins_flips_and_a_doubled_flip(kind):
    """Another universe as the twin, with and without flips on top; a cell listed twice cancels, so (a, b, a) is b alone and (a, a) with
    the universe itself is no perturbation at all."""
    rule = rule_of(kind, 0)
    state, other = host.seeded_state(G, 31, 2), host.seeded_state(G, 32, 2)
    a, b = (5, 6, 7), (40, 41, 42)
    check(kind, rule, "reference", state, 2, twin=other, what=(kind, "twin"))
    check(kind, rule, "torus", state, 2, twin=other, flips=[a, b], what=(kind, "twin and flips"))
    one = check(kind, rule, "reference", state, 2, flips=[b], what=(kind, "b"))
    twice = check(kind, rule, "reference", state, 2, flips=[a, b, a], what=(kind, "a b a"))
    assert one[0].tolist() == twice[0].tolist() and as_dict(one[1]) == as_dict(twice[1]) and np.array_equal(one[2], twice[2])
    curve, rec, last = check(kind, rule, "reference", state, 2, flips=[a, a], what=(kind, "a a"))
    assert curve.tolist() == [0, 0, 0] and int(rec["healed_at"]) == 0 and not last.any()


@pytest.mark.parametrize("kind", KINDS)
def test_a_lone_flip_grows_by_the_boundary(kind):
    """One flipped cell in an empty universe under born-at-1: the difference IS the single-cell evolution. A + face wraps in reference
    mode and a - face is dead, so the cell in the corner (0, 0, 0) is seen through three faces on a torus and in reference mode and
    through none in a closed cube, and the cell in the corner (63, 63, 63) on a torus alone: the pair of curves tells the three apart."""
    rule = grow_rule(kind)
    empty = np.zeros(W, dtype=np.uint32)
    curves = {b: tuple(tuple(check(kind, rule, b, empty, 2, flips=[c], what=(kind, b, c))[0].tolist()) for c in ((0, 0, 0), (63, 63, 63)))
              for b in host.ENSEMBLE_BOUNDARIES}
    assert len(set(curves.values())) == 3, curves
    assert curves["reference"][0] != curves["closed"][0] and curves["reference"][1] == curves["closed"][1] != curves["torus"][1], curves
    assert all(c[0] == 1 for pair in curves.values() for c in pair)


@pytest.mark.parametrize("kind", KINDS)
def test_full_against_empty_under_born_never_survive_always(kind):
    """B none / S all: the empty source stays empty and the all-ones twin stays full, so d_t = 262 144 at every t, nothing heals, the
    first maximum is at 0, both boxes are the whole cube. At P = 4096 the sum is 262 144 x 4 097 = 1 074 003 968, near a word's end."""
    bits = 7 if kind == "von neumann" else 27
    rule = plain(kind, 0, (1 << bits) - 1)
    empty, full = np.zeros(W, dtype=np.uint32), np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    curve, rec, last = check(kind, rule, "reference", empty, 3, twin=full, what=(kind, "P = 3"))
    assert curve.tolist() == [1 << 18] * 4 and int(rec["distance_sum"]) == 4 << 18
    curve, rec, last = host.damage(empty, kind, tables_of(kind, rule), 4096, twin=full)
    assert curve.shape == (4097,) and (curve == 1 << 18).all() and np.array_equal(last, full)
    assert as_dict(rec) == {"steps": 4096, "flags": 0, "healed_at": NEVER, "final_distance": 1 << 18, "initial_distance": 1 << 18,
                            "max_distance": 1 << 18, "max_at": 0, "distance_sum": 1074003968, "damage_min": (0, 0, 0, 0),
                            "damage_max": (63, 63, 63, 0), "touched_min": (0, 0, 0, 0), "touched_max": (63, 63, 63, 0)}
    assert 262144 * 4097 == 1074003968 < 1 << 32


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("kind", ("von neumann", "moore"))
def test_a_healing_row(kind, axis):
    """B none / S2 against an empty source: nothing is ever born; of a straight row only the inner cells have exactly two live
    neighbours (in a row no two cells are diagonal neighbours, so the Moore count is the von Neumann one), so the two end cells die
    every step: 9, 7, 5, 3, 1, 0 — healed at 5. Three flips in a row: 3, 1, 0 — healed at 2."""
    rule = plain(kind, 0, 1 << 2)
    empty = np.zeros(W, dtype=np.uint32)

    def row(n):
        return [tuple(28 + i if a == axis else 20 + 3 * a for a in range(3)) for i in range(n)]  # across the word seam along x

    curve, rec, last = check(kind, rule, "reference", empty, 7, twin=host.cells_to_words(G, row(9)), what=(kind, axis, "row of 9"))
    assert curve.tolist() == [9, 7, 5, 3, 1, 0, 0, 0] and int(rec["healed_at"]) == 5 and int(rec["flags"]) == host.DAMAGE_HEALED
    assert (int(rec["max_distance"]), int(rec["max_at"]), int(rec["distance_sum"]), int(rec["final_distance"])) == (9, 0, 25, 0) and not last.any()
    assert tuple(rec["damage_min"]) == tuple(rec["damage_max"]) == (0, 0, 0, 0)
    lo, hi = row(9)[0], row(9)[-1]
    assert tuple(rec["touched_min"]) == lo + (0,) and tuple(rec["touched_max"]) == hi + (0,)
    curve, rec, _ = check(kind, rule, "reference", empty, 4, flips=row(3), what=(kind, axis, "three flips"))
    assert curve.tolist() == [3, 1, 0, 0, 0] and int(rec["healed_at"]) == 2
    # healed exactly at P, and one step short of it
    assert int(host.damage(empty, kind, tables_of(kind, rule), 2, flips=row(3))[1]["healed_at"]) == 2
    short = host.damage(empty, kind, tables_of(kind, rule), 1, flips=row(3))[1]
    assert (int(short["flags"]), int(short["healed_at"]), int(short["final_distance"])) == (0, NEVER, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_no_perturbation(kind):
    state = host.seeded_state(G, 41, 1)
    curve, rec, last = check(kind, rule_of(kind, 3), "closed", state, 3, what=(kind, "itself"))
    assert curve.tolist() == [0] * 4 and not last.any()
    assert as_dict(rec) == {**{n: 0 for n in ("healed_at", "final_distance", "initial_distance", "max_distance", "max_at", "distance_sum")}, "steps": 3,
                            "flags": host.DAMAGE_HEALED, **{n: (0, 0, 0, 0) for n in ("damage_min", "damage_max", "touched_min", "touched_max")}}


def test_refusals():
    first = np.zeros(W, dtype=np.uint32)
    for bad in (0, host.CANON_MAX_PERIOD + 1):
        with pytest.raises(ValueError):
            host.damage(first, "moore", (0, 0), bad)
    with pytest.raises(ValueError):
        host.damage(first, "moore", (0, 0), 1, flips=[(0, 0, 0)] * 5)
    with pytest.raises(ValueError):
        host.damage(first, "moore", (0, 0), 1, flips=[(64, 0, 0)])
    with pytest.raises(ValueError):
        host.damage(first, "moore", (0, 0), 1, twin=np.zeros(100, dtype=np.uint32))
    with pytest.raises(ValueError):
        host.damage_of_phases(np.zeros((1, W), dtype=np.uint32), np.zeros((1, W), dtype=np.uint32))
    with pytest.raises(ValueError):
        host.damage_of_phases(np.zeros((3, W), dtype=np.uint32), np.zeros((2, W), dtype=np.uint32))
    assert host.damage_flip_word((1, 2, 3)) == 0x030201


def test_symbol_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_damage\(ca3d_ensemble_t \*src, uint32_t first, uint32_t count, const uint32_t \*steps", header, flags=re.M)
    assert re.search(r"typedef struct ca3d_damage\s*\{[^}]*uint32_t steps;[^}]*uint32_t flags;[^}]*uint32_t healed_at;[^}]*uint32_t final_distance;"
                     r"[^}]*uint32_t initial_distance;[^}]*uint32_t max_distance;[^}]*uint32_t max_at;[^}]*uint32_t distance_sum;"
                     r"[^}]*uint8_t damage_min\[4\], damage_max\[4\];[^}]*uint8_t touched_min\[4\], touched_max\[4\];[^}]*\} ca3d_damage;", header)
    for name, value in (("HEALED", 1), ("FLIPS", 4), ("SELF", 0xFFFFFFFF), ("NO_FLIP", 0xFFFFFFFF), ("IMAGE_DAMAGE", 1), ("COPY_RULES", 0x100)):
        assert re.search(r"^#define CA3D_DAMAGE_%s (0x)?%xu\b" % (name, value), header, flags=re.M | re.I), name
    assert (host.DAMAGE_HEALED, host.DAMAGE_FLIPS, host.DAMAGE_SELF, host.DAMAGE_NO_FLIP, host.DAMAGE_NEVER) == (1, 4, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert (_capi.DAMAGE_IMAGE_DAMAGE, _capi.DAMAGE_COPY_RULES) == (1, 0x100)
    assert "ca3d_ensemble_damage" in bound and hasattr(lib, "ca3d_ensemble_damage") and len(bound["ca3d_ensemble_damage"]) == 13
    assert C.sizeof(_capi.DamageStruct) == 48 == host.DAMAGE_DTYPE.itemsize
    assert [(n, host.DAMAGE_DTYPE.fields[n][1]) for n in host.DAMAGE_DTYPE.names] == \
        [(n, getattr(_capi.DamageStruct, n).offset) for n, _ in _capi.DamageStruct._fields_]
    declared = set(re.findall(r"^(?:int|const char \*|void) ?\*?(ca3d_\w+)\(", header, flags=re.M))
    assert declared == set(bound), declared ^ set(bound)
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    mk = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bca_damage\.o\b", mk, flags=re.M)


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.DamageStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    steps = (C.c_uint32 * 2)(4, 4)
    ms = C.c_float(-1.0)
    assert lib.ca3d_ensemble_damage(None, 0, 2, steps, None, None, None, 0, 0, out, None, 0, C.byref(ms)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(steps) == [4, 4] and ms.value == -1.0


def test_python_and_js_surfaces():
    for name in ("damage", "damage_gpu_ms"):
        assert callable(getattr(Ensemble, name)), name
    for name in ("DAMAGE_DTYPE", "damage", "damage_of_phases", "damage_twin", "damage_flip_word", "DAMAGE_HEALED", "DAMAGE_SELF", "DAMAGE_NO_FLIP", "DAMAGE_FLIPS"):
        assert hasattr(host, name), name
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    assert re.search(r"^\tdamage\(steps, opts\)$", js, flags=re.M) and "ensembleDamage(" in js
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert '{"ensembleDamage", js_ensemble_damage}' in napi and "ca3d_ensemble_damage(" in napi
