"""The host side of the envelope over a period (`ca3d_ensemble_envelope`, include/ca3d.h): `host.envelope`, the numpy restatement of the
definition, against a brute force that does not go through it — the unpacked cells of every phase of an oracle trajectory
(oracle_lib.packed_step) in reference mode, of a chain of `host.ensemble_step` in torus and closed mode, ORed, ANDed and counted cell
by cell —; the symbol, the struct and the Python and JS surfaces. All comparisons are exact. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import canon_cases as kc
import oracle_lib as ol
from cellularautomatons3d_amd import _capi, host
from cellularautomatons3d_amd.ensemble import Ensemble
from test_gpu_moving import SHIP, moore_rules, ship

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, W = 64, 8192
OSCILLATOR = ((15, 15, 15), (16, 15, 15), (15, 16, 15), (15, 15, 16))  # Moore B4/S4, period 2, population 4 each step


def mask(s, bits=27):
    m = 0
    for v in host.rules_components_to_values(s):
        m |= 1 << v
    return m & ((1 << bits) - 1)


def cells(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def pack(c):
    return np.packbits(np.ascontiguousarray(c, dtype=np.uint8).ravel(), bitorder="little").view("<u4").astype(np.uint32)


def box(c):
    """(min, max) as (x, y, z, 0) of a [z, y, x] cell array; zeros for an empty one."""
    if not c.any():
        return (0, 0, 0, 0), (0, 0, 0, 0)
    idx = [np.flatnonzero(c.any(axis=ax)) for ax in ((0, 1), (0, 2), (1, 2))]  # x, y, z
    return tuple(int(i[0]) for i in idx) + (0,), tuple(int(i[-1]) for i in idx) + (0,)


def brute(states):
    """The record's fields and the three images of the phases S_0 .. S_P by the definition, cell by cell."""
    p = len(states) - 1
    c = [cells(s).astype(bool) for s in states]
    env, sta = np.zeros((G, G, G), bool), np.ones((G, G, G), bool)
    heat = pops = 0
    for t in range(p):
        env |= c[t]
        sta &= c[t]
        pops += int(c[t].sum())
        heat += int((c[t] != c[t + 1]).sum())
    rot = env & ~sta
    want = {"period": p, "flags": int(np.array_equal(c[p], c[0])), "heat": heat, "population_sum": pops, "envelope_population": int(env.sum()),
            "stator_population": int(sta.sum()), "envelope_min": box(env)[0], "envelope_max": box(env)[1], "rotor_min": box(rot)[0],
            "rotor_max": box(rot)[1], "reserved": (0, 0)}
    return want, pack(env), pack(sta), pack(rot)


def as_dict(rec):
    return {n: (int(rec[n]) if rec[n].ndim == 0 else tuple(int(v) for v in rec[n])) for n in rec.dtype.names}


def check(first, kind, tables, period, boundary, states, what):
    """host.envelope of `first` against the brute force over `states`, S_0 .. S_period from another stepper."""
    rec, env, sta, rot = host.envelope(first, kind, tables, period, boundary)
    want, wenv, wsta, wrot = brute(states)
    assert rec.dtype == host.ENVELOPE_DTYPE and rec.shape == (), what
    assert as_dict(rec) == want, what
    for got, exp in ((env, wenv), (sta, wsta), (rot, wrot)):
        assert got.dtype == np.uint32 and got.shape == (W,) and np.array_equal(got, exp), what
    # and over the same phases, already stepped
    rec2, env2, sta2, rot2 = host.envelope_of_phases(np.stack(states))
    assert as_dict(rec2) == want and np.array_equal(env2, wenv) and np.array_equal(sta2, wsta) and np.array_equal(rot2, wrot), what
    return rec


def oracle_states(first, rules, period):
    s = [np.ascontiguousarray(first, dtype=np.uint32)]
    for _ in range(period):
        s.append(ol.packed_step(G, s[-1], rules))
    return s


def chain_states(first, kind, tables, boundary, period):
    s = [np.ascontiguousarray(first, dtype=np.uint32)]
    for _ in range(period):
        s.append(host.ensemble_step(s[-1], kind, tables, boundary))
    return s


B4S4 = (mask("4"), mask("4"))
SHIP_TABLES = (mask(SHIP[0]), mask(SHIP[1]))


def test_the_four_cell_oscillator():
    """SURVEY's Moore B4/S4 seed: a corner (15,15,15) of the cube {15,16}^3 and its three neighbours along the axes. Each of the four has
    three live neighbours and dies; each of the cube's four other cells touches all four and is born; nothing outside the cube touches
    more than three. So the phases are the two halves of the cube: E is the cube, 8 cells, box (15,15,15) .. (16,16,16); A is empty;
    the rotor is E, 8 cells, the same box; every step changes all 8 cells, heat 16 over P = 2; population_sum 4 + 4; and S_2 = S_0."""
    first = host.cells_to_words(G, OSCILLATOR)
    rules = moore_rules("4", "4")
    rec = check(first, "moore", B4S4, 2, "reference", oracle_states(first, rules, 2), "B4/S4, P = 2")
    assert as_dict(rec) == {"period": 2, "flags": host.ENVELOPE_RETURNS, "heat": 16, "population_sum": 8, "envelope_population": 8, "stator_population": 0,
                            "envelope_min": (15, 15, 15, 0), "envelope_max": (16, 16, 16, 0), "rotor_min": (15, 15, 15, 0), "rotor_max": (16, 16, 16, 0),
                            "reserved": (0, 0)}
    d = host.envelope_derived(rec)
    assert int(d["rotor_population"]) == 8 and float(d["volatility"]) == 1.0 and float(d["heat_per_step"]) == 8.0 and bool(d["returns"])
    # P = 3 ends in the other phase: no RETURNS, heat 24
    rec3 = check(first, "moore", B4S4, 3, "reference", oracle_states(first, rules, 3), "B4/S4, P = 3")
    assert int(rec3["flags"]) == 0 and int(rec3["heat"]) == 24 and int(rec3["population_sum"]) == 12 and int(rec3["envelope_population"]) == 8


@pytest.mark.parametrize("boundary", ("torus", "closed"))
def test_the_oscillator_on_a_seam_and_against_a_face(boundary):
    """Rolled astride the x, y and z seams at once (torus) or pushed into the corner of the - faces (closed): against chains of
    host.ensemble_step. On the torus the cube wraps and the numbers are those of the middle of the universe."""
    first = pack(np.roll(cells(host.cells_to_words(G, OSCILLATOR)), shift=(-16, -16, -16), axis=(0, 1, 2))) if boundary == "torus" else \
        host.cells_to_words(G, [(x - 15, y - 15, z - 15) for x, y, z in OSCILLATOR])
    for p in (2, 3):
        rec = check(first, "moore", B4S4, p, boundary, chain_states(first, "moore", B4S4, boundary, p), (boundary, p))
        if boundary == "torus":
            assert int(rec["envelope_population"]) == 8 and int(rec["heat"]) == 8 * p and bool(int(rec["flags"])) == (p == 2)
            assert tuple(rec["envelope_min"]) == (0, 0, 0, 0) and tuple(rec["envelope_max"]) == (63, 63, 63, 0)  # through all three seams


def test_a_still_life():
    """The 2 x 2 x 2 block under B6/S5-7: every cell has seven neighbours. Rotor empty, heat 0."""
    rules = moore_rules(*SHIP)
    block = kc.shape_words("block")
    assert np.array_equal(ol.packed_step(G, block, rules), block) and block.any()
    for p in (1, 5):
        rec = check(block, "moore", SHIP_TABLES, p, "reference", oracle_states(block, rules, p), ("block", p))
        assert int(rec["heat"]) == 0 and int(rec["flags"]) == host.ENVELOPE_RETURNS
        assert int(rec["envelope_population"]) == int(rec["stator_population"]) == 8 and int(rec["population_sum"]) == 8 * p
        assert tuple(rec["rotor_min"]) == tuple(rec["rotor_max"]) == (0, 0, 0, 0)
        assert int(host.envelope_derived(rec)["rotor_population"]) == 0 and float(host.envelope_derived(rec)["volatility"]) == 0.0


def test_the_doubled_glider():
    """tests/test_gpu_moving.py's ship "a": a swept volume and no RETURNS, at its period and at twice that."""
    t = ship("a")
    for p in (4, 8):
        rec = check(t[0], "moore", SHIP_TABLES, p, "reference", [t[k] for k in range(p + 1)], ("glider", p))
        assert int(rec["flags"]) == 0 and int(rec["population_sum"]) == sum(int(cells(t[k]).sum()) for k in range(p))
        assert int(rec["envelope_population"]) > 10 and int(rec["heat"]) > 0
    # in the other two modes, clear of the faces, nothing differs
    for boundary in ("torus", "closed"):
        rec = check(t[0], "moore", SHIP_TABLES, 4, boundary, chain_states(t[0], "moore", SHIP_TABLES, boundary, 4), ("glider", boundary))
        assert as_dict(rec) == as_dict(host.envelope(t[0], "moore", SHIP_TABLES, 4)[0])


def test_an_empty_universe():
    empty = np.zeros(W, dtype=np.uint32)
    rec = check(empty, "moore", SHIP_TABLES, 3, "reference", oracle_states(empty, moore_rules(*SHIP), 3), "empty")
    assert as_dict(rec) == {**{n: 0 for n in ("heat", "population_sum", "envelope_population", "stator_population")}, "period": 3,
                            "flags": host.ENVELOPE_RETURNS, "reserved": (0, 0),
                            **{n: (0, 0, 0, 0) for n in ("envelope_min", "envelope_max", "rotor_min", "rotor_max")}}
    assert float(host.envelope_derived(rec)["volatility"]) == 0.0


def test_period_one():
    """E = A = S_0, the rotor is empty, heat = popcount(S_0 ^ S_1): a von Neumann soup and a clustered one."""
    first = host.random_fill(W, seed=3, and_rounds=2)
    rules = ol.Rules.from_strings(neighbourhood="von neumann", born="3", survive="2,3")
    states = oracle_states(first, rules, 1)
    rec, env, sta, rot = host.envelope(first, "von neumann", (mask("3", 7), mask("2,3", 7)), 1)
    check(first, "von neumann", (mask("3", 7), mask("2,3", 7)), 1, "reference", states, "vn, P = 1")
    assert np.array_equal(env, first) and np.array_equal(sta, first) and not rot.any()
    assert int(rec["heat"]) == int(ol.popcount(states[0] ^ states[1])) and int(rec["population_sum"]) == int(ol.popcount(first))
    assert int(rec["envelope_population"]) == int(rec["stator_population"]) == int(ol.popcount(first))
    tables = ((mask("6"), mask("3-5", 13), mask("", 9)), (mask("5-7"), mask("", 13), mask("1-8", 9)))
    for boundary in host.ENSEMBLE_BOUNDARIES:
        check(first, "clustered", tables, 2, boundary, chain_states(first, "clustered", tables, boundary, 2), ("clustered", boundary))


def test_refusals():
    first = np.zeros(W, dtype=np.uint32)
    for bad in (0, host.CANON_MAX_PERIOD + 1):
        with pytest.raises(ValueError):
            host.envelope(first, "moore", B4S4, bad)
    with pytest.raises(ValueError):
        host.envelope_of_phases(np.zeros((1, W), dtype=np.uint32))
    with pytest.raises(ValueError):
        host.envelope_of_phases(np.zeros((2, 100), dtype=np.uint32))


def test_symbol_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_envelope\(ca3d_ensemble_t \*src, uint32_t first, uint32_t count, const uint32_t \*periods", header, flags=re.M)
    assert re.search(r"typedef struct ca3d_envelope\s*\{[^}]*uint32_t period;[^}]*uint32_t flags;[^}]*uint32_t heat;[^}]*uint32_t population_sum;"
                     r"[^}]*uint32_t envelope_population;[^}]*uint32_t stator_population;[^}]*uint8_t envelope_min\[4\], envelope_max\[4\];"
                     r"[^}]*uint8_t rotor_min\[4\], rotor_max\[4\];[^}]*uint32_t reserved\[2\];[^}]*\} ca3d_envelope;", header)
    for name, value in (("RETURNS", 1), ("IMAGE_ENVELOPE", 1), ("IMAGE_STATOR", 2), ("IMAGE_ROTOR", 4), ("COPY_RULES", 0x100)):
        assert re.search(r"^#define CA3D_ENVELOPE_%s (0x)?%xu\b" % (name, value), header, flags=re.M), name
    assert host.ENVELOPE_RETURNS == 1 and host.ENVELOPE_IMAGES == {"envelope": 1, "stator": 2, "rotor": 4} and _capi.ENVELOPE_COPY_RULES == 0x100
    assert list(host.ENVELOPE_IMAGES) == ["envelope", "stator", "rotor"]  # the order the images are written in
    assert "ca3d_ensemble_envelope" in bound and hasattr(lib, "ca3d_ensemble_envelope") and len(bound["ca3d_ensemble_envelope"]) == 9
    assert C.sizeof(_capi.EnvelopeStruct) == 48 == host.ENVELOPE_DTYPE.itemsize
    assert [(n, host.ENVELOPE_DTYPE.fields[n][1]) for n in host.ENVELOPE_DTYPE.names] == \
        [(n, getattr(_capi.EnvelopeStruct, n).offset) for n, _ in _capi.EnvelopeStruct._fields_]
    declared = set(re.findall(r"^(?:int|const char \*|void) ?\*?(ca3d_\w+)\(", header, flags=re.M))
    assert declared == set(bound), declared ^ set(bound)
    mk = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bca_envelope\.o\b", mk, flags=re.M)


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.EnvelopeStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    periods = (C.c_uint32 * 2)(4, 4)
    ms = C.c_float(-1.0)
    assert lib.ca3d_ensemble_envelope(None, 0, 2, periods, None, 0, 0, out, C.byref(ms)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(periods) == [4, 4] and ms.value == -1.0


def test_python_and_js_surfaces():
    for name in ("envelope", "envelope_gpu_ms"):
        assert callable(getattr(Ensemble, name)), name
    for name in ("ENVELOPE_DTYPE", "envelope", "envelope_of_phases", "envelope_derived", "ENVELOPE_RETURNS", "ENVELOPE_IMAGES"):
        assert hasattr(host, name), name
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    assert re.search(r"^\tenvelope\(periods, opts\)$", js, flags=re.M) and "ensembleEnvelope(" in js
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert '{"ensembleEnvelope", js_ensemble_envelope}' in napi and "ca3d_ensemble_envelope(" in napi
