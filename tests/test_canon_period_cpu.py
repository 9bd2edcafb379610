"""The host side of canon over a period (`ca3d_ensemble_canon_period`, include/ca3d.h): `host.canon_period`, the numpy restatement of the
definition, against a brute force that goes through neither it nor `host.canon` — canon_cases.brute of every phase of an oracle
trajectory (oracle_lib.packed_step), CLOSED by canon_cases.turned(., 0), the shift from `host.state_summary`'s boxes —; the symbol, the
struct and the Python and JS surfaces. All comparisons are exact. No GPU."""
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
FULL = (1 << 48) - 1


def brute_period(states):
    """-> (key, phase, orientation, symmetry, population, closed, shift, keys) of the phases S_0 .. S_p by the definition, the slow way."""
    p = len(states) - 1
    per = [kc.brute(states[t]) for t in range(p)]
    keys = [k for k, _, _, _ in per]
    t = keys.index(min(keys))
    first, last = host.state_summary(G, states[0]), host.state_summary(G, states[p])
    closed = bool(np.array_equal(kc.turned(states[0], 0), kc.turned(states[p], 0)))
    shift = (0, 0, 0)
    if closed and first["population"]:
        shift = tuple(int(b) - int(a) for a, b in zip(first["box_min"], last["box_min"]))
    return keys[t], t, per[t][1], per[t][2], int(host.state_summary(G, states[t])["population"]), closed, shift, keys


def check(states, what):
    rec, keys = host.canon_period(np.stack(states))
    key, phase, orientation, symmetry, population, closed, shift, want_keys = brute_period(states)
    assert rec.dtype == host.CANON_PERIOD_DTYPE and keys.dtype == np.uint64 and keys.shape == (len(states) - 1,), what
    assert keys.tolist() == want_keys, what
    assert (int(rec["key"]), int(rec["phase"]), int(rec["orientation"]), int(rec["symmetry"]), int(rec["population"])) == \
        (key, phase, orientation, symmetry, population), what
    assert bool(int(rec["flags_shift"]) & host.CANON_CLOSED) == closed, what
    assert host.unpack_shift(rec["flags_shift"]) == shift, what
    assert int(rec["flags_shift"]) & 0xFE == 0, what
    return rec, keys


def test_the_glider_over_its_period():
    """tests/test_gpu_moving.py's ship "a" under Moore B6/S5-7: four steps bring it back one cell along x and y."""
    t = ship("a")
    rec, keys = check([t[k] for k in range(5)], "glider, p = 4")
    assert int(rec["flags_shift"]) & host.CANON_CLOSED
    assert host.unpack_shift(rec["flags_shift"]) == host.moved_by(G, t[0], t[4]) == (1, 1, 0)
    assert int(rec["key"]) == min(int(host.canon(t[k])[0]["key"]) for k in range(4))
    # the same key whichever phase the universe is in
    for start in range(1, 4):
        other, _ = host.canon_period(np.stack([t[start + k] for k in range(5)]))
        assert int(other["key"]) == int(rec["key"]) and int(other["flags_shift"]) == int(rec["flags_shift"]), start


def test_the_glider_over_an_untrue_period():
    t = ship("a")
    rec, keys = check([t[k] for k in range(4)], "glider, p = 3")
    assert int(rec["flags_shift"]) == 0 and keys.shape == (3,)
    rec8, _ = check([t[k] for k in range(9)], "glider, p = 8")
    assert int(rec8["flags_shift"]) & host.CANON_CLOSED and host.unpack_shift(rec8["flags_shift"]) == (2, 2, 0)


def test_a_still_life():
    """The 2 x 2 x 2 block if the rule keeps it, else the first fixed point a soup under the rule reaches."""
    rules = moore_rules(*SHIP)
    block = kc.shape_words("block")
    nxt = ol.packed_step(G, block, rules)
    if not np.array_equal(nxt, block):
        state = host.random_fill(W, seed=1, and_rounds=0)
        for _ in range(512):
            nxt = ol.packed_step(G, state, rules)
            if np.array_equal(nxt, state):
                break
            state = nxt
        block = state
        assert np.array_equal(ol.packed_step(G, block, rules), block) and block.any()
    rec, keys = check([block, ol.packed_step(G, block, rules)], "still life, p = 1")
    assert int(rec["flags_shift"]) == host.CANON_CLOSED and int(rec["phase"]) == 0
    assert int(rec["key"]) == int(keys[0]) == int(host.canon(block)[0]["key"])


def test_the_empty_universe():
    empty = np.zeros(W, dtype=np.uint32)
    rec, keys = check([empty, empty, empty], "empty, p = 2")
    assert [int(rec[f]) for f in ("key", "symmetry", "orientation", "phase", "population", "flags_shift")] == [0, FULL, 0, 0, 0, host.CANON_CLOSED]
    assert not keys.any()
    # an empty S_0 whose S_p is not empty (a rule that bears cells out of nothing would do that): not CLOSED, shift 0
    rec, keys = check([empty, kc.shape_words("block")], "empty, then something")
    assert [int(rec[f]) for f in ("key", "symmetry", "phase", "flags_shift")] == [0, FULL, 0, 0]
    # and a state that dies: not CLOSED either
    rec, _ = check([kc.shape_words("cell"), empty], "a cell, then nothing")
    assert int(rec["flags_shift"]) == 0


def test_unpack_shift_and_refusals():
    assert host.unpack_shift(1 | 0xFF << 8 | 0x02 << 16 | 0x80 << 24) == (-1, 2, -128)
    assert host.unpack_shift(0) == (0, 0, 0)
    with pytest.raises(ValueError):
        host.canon_period(np.zeros((1, W), dtype=np.uint32))
    with pytest.raises(ValueError):
        host.canon_period(np.zeros((2, 100), dtype=np.uint32))


def test_symbol_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_canon_period\(ca3d_ensemble_t \*e, uint32_t first, uint32_t count, const uint32_t \*periods", header, flags=re.M)
    assert re.search(r"typedef struct ca3d_canon_period\s*\{[^}]*uint64_t key;[^}]*uint64_t symmetry;[^}]*uint32_t orientation;[^}]*uint32_t phase;"
                     r"[^}]*uint32_t population;[^}]*uint32_t flags_shift;[^}]*\} ca3d_canon_period;", header)
    assert re.search(r"^#define CA3D_CANON_CLOSED 1u\b", header, flags=re.M) and host.CANON_CLOSED == 1
    assert re.search(r"^#define CA3D_CANON_MAX_PERIOD 4096u\b", header, flags=re.M) and host.CANON_MAX_PERIOD == 4096
    assert "ca3d_ensemble_canon_period" in bound and hasattr(lib, "ca3d_ensemble_canon_period")
    assert len(bound["ca3d_ensemble_canon_period"]) == 8
    assert C.sizeof(_capi.CanonPeriodStruct) == 32 == host.CANON_PERIOD_DTYPE.itemsize
    assert [(n, host.CANON_PERIOD_DTYPE.fields[n][1]) for n in host.CANON_PERIOD_DTYPE.names] == \
        [(n, getattr(_capi.CanonPeriodStruct, n).offset) for n, _ in _capi.CanonPeriodStruct._fields_]
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    declared = set(re.findall(r"^(?:int|const char \*|void) ?\*?(ca3d_\w+)\(", header, flags=re.M))
    assert declared == set(bound), declared ^ set(bound)
    mk = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bca_canon_period\.o\b", mk, flags=re.M)
    assert re.search(r"^%\.o: %\.hip .*\bca_ensemble_step\.inc\b", mk, flags=re.M)


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.CanonPeriodStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    keys = (C.c_uint64 * 8)(*([7] * 8))
    periods = (C.c_uint32 * 2)(4, 4)
    ms = C.c_float(-1.0)
    assert lib.ca3d_ensemble_canon_period(None, 0, 2, periods, out, keys, 4, C.byref(ms)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(keys) == [7] * 8 and ms.value == -1.0


def test_python_and_js_surfaces():
    for name in ("canon_period", "canon_period_gpu_ms", "canon_phases"):
        assert callable(getattr(Ensemble, name)), name
    for name in ("CANON_PERIOD_DTYPE", "canon_period", "unpack_shift", "CANON_CLOSED", "CANON_MAX_PERIOD"):
        assert hasattr(host, name), name
    assert "canon_period" in Ensemble.canon_phases.__doc__
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    assert re.search(r"^\tcanonPeriod\(opts\)$", js, flags=re.M) and "ensembleCanonPeriod(" in js
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert '{"ensembleCanonPeriod", js_ensemble_canon_period}' in napi and "ca3d_ensemble_canon_period(" in napi
