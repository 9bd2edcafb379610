"""The host side of rule usage (`ca3d_ensemble_usage`, include/ca3d.h): `host.usage`, the numpy restatement of the definition, against
histograms that do not go through it — graded_lib's `coverage` (26 shifted copies a cell, reference and torus), a cell-by-cell brute
force for the closed cube —, over one step and over three; the identities of the record; the symbol, the struct and the Python and JS
surfaces. All comparisons are exact. No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import graded_lib as gl
from cellularautomatons3d_amd import _capi, host
from cellularautomatons3d_amd.ensemble import Ensemble
from test_ensemble_boundary_cpu import grow_rule, rule_of, tables_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, W, CELLS = 64, 8192, 64 ** 3
KINDS = ("von neumann", "moore", "clustered")
# kind -> [(class index, first bin, key of graded_lib's counts)]
LOOKS_UP = {"von neumann": [(0, host.USAGE_MAIN, "F")], "moore": [(0, host.USAGE_MAIN, "T")],
            "clustered": [(0, host.USAGE_MAIN, "T"), (1, host.USAGE_EDGES, "E"), (2, host.USAGE_CORNERS, "C")]}


@pytest.fixture(scope="module")
def graded():
    return {name: gl.graded_state(G, axis, reverse) for name, (axis, reverse) in gl.ORIENTATIONS.items()}


def record_of(kind, coverages):
    """The record the coverages {key: [2, N]} of the phases add up to: every field, built here field by field."""
    dead, alive = np.zeros(host.USAGE_BINS, dtype=np.int64), np.zeros(host.USAGE_BINS, dtype=np.int64)
    for cov in coverages:
        for _, base, key in LOOKS_UP[kind]:
            n = gl.SIZES[key]
            dead[base:base + n] += cov[key][0]
            alive[base:base + n] += cov[key][1]
    want = {"steps": len(coverages), "flags": 0, "used_born": [0, 0, 0], "used_survive": [0, 0, 0], "dead": dead.tolist(), "alive": alive.tolist(),
            "reserved": [0, 0]}
    for i, (base, n) in enumerate(((0, 27), (27, 13), (40, 9))):
        want["used_born"][i] = sum(1 << c for c in range(n) if dead[base + c])
        want["used_survive"][i] = sum(1 << c for c in range(n) if alive[base + c])
    return want


def as_dict(rec):
    return {n: (int(rec[n]) if rec[n].ndim == 0 else [int(v) for v in rec[n]]) for n in rec.dtype.names}


def closed_coverage(cells):
    """{key: [2, N]} of a closed cube by brute force, cell by cell: every live cell adds one to the class count of each of its 26
    neighbours that lies inside the cube; a cell nobody reached has count zero in every class."""
    seen = {}
    for x, y, z in cells:
        for dx, dy, dz in itertools.product((-1, 0, 1), repeat=3):
            moved = abs(dx) + abs(dy) + abs(dz)
            p = (x + dx, y + dy, z + dz)
            if moved and all(0 <= v < G for v in p):
                seen.setdefault(p, [0, 0, 0])[moved - 1] += 1
    live = set(cells)
    cov = {k: np.zeros((2, n), dtype=np.int64) for k, n in gl.SIZES.items() if k in "TFEC"}
    for p in live | set(seen):
        f, e, c = seen.get(p, (0, 0, 0))
        for key, v in (("F", f), ("E", e), ("C", c), ("T", f + e + c)):
            cov[key][int(p in live), v] += 1
    for key in cov:
        cov[key][0, 0] += CELLS - len(live | set(seen))
    return cov


def test_the_graded_states_reach_every_bin(graded):
    """What the exact comparisons below and on the GPU rest on: no bin of any class is empty in any of the four states."""
    least = {k: min(int(gl.coverage(G, w)[k].min()) for w in graded.values()) for k in "TFEC"}
    print(least)
    assert all(v > 0 for v in least.values()), least


@pytest.mark.parametrize("boundary", ("reference", "torus"))
@pytest.mark.parametrize("kind", KINDS)
def test_one_step_against_coverage(graded, kind, boundary):
    for name, words in graded.items():
        cov = gl.coverage(G, words, torus=boundary == "torus")
        rec = host.usage(words, kind, tables_of(kind, rule_of(kind, 0)), 1, boundary)
        assert rec.dtype == host.USAGE_DTYPE and rec.shape == (), name
        assert as_dict(rec) == record_of(kind, [cov]), name


@pytest.mark.parametrize("kind", KINDS)
def test_one_step_in_a_closed_cube_cell_by_cell(kind):
    rng = np.random.default_rng(77)
    # clumps in two opposite corners, on a face and on an edge, and a sprinkle anywhere: a few hundred cells, counts of every class
    cells = set()
    for lo, n in (((0, 0, 0), 70), ((60, 60, 60), 70), ((30, 60, 10), 50), ((0, 60, 33), 50)):
        cells |= {tuple(int(lo[i] + v[i]) for i in range(3)) for v in rng.integers(0, 4, size=(n, 3))}
    cells |= {tuple(int(c) for c in v) for v in rng.integers(0, G, size=(150, 3))}
    cells = sorted(cells)
    assert 200 < len(cells) < 600
    words = host.cells_to_words(G, cells)
    want = record_of(kind, [closed_coverage(cells)])
    assert as_dict(host.usage(words, kind, tables_of(kind, grow_rule(kind)), 1, "closed")) == want
    # and the other two boundaries differ from it on this state: the faces matter
    for other in ("reference", "torus"):
        assert as_dict(host.usage(words, kind, tables_of(kind, grow_rule(kind)), 1, other)) != want


@pytest.mark.parametrize("boundary", ("reference", "torus"))
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_against_a_chain(graded, kind, boundary):
    rule = rule_of(kind, 1)
    tables = tables_of(kind, rule)
    chain = [graded["zr"]]
    for _ in range(2):
        chain.append(host.ensemble_step(chain[-1], kind, tables, boundary))
    assert not np.array_equal(chain[0], chain[1]) and not np.array_equal(chain[1], chain[2])
    want = record_of(kind, [gl.coverage(G, w, torus=boundary == "torus") for w in chain])
    assert as_dict(host.usage(chain[0], kind, tables, 3, boundary)) == want
    assert as_dict(host.usage_of_phases(chain, kind, boundary)) == want
    # the counts are the step's own: looked up in the tables, they give the chain's next state
    cells, counts = host._ensemble_counts(chain[0], kind, boundary)
    nxt = np.zeros_like(cells)
    for count, r in zip(counts, rule if kind == "clustered" else (rule,)):
        nxt |= gl.lookup(cells, count, r.born, r.survive)
    assert np.array_equal(gl.pack(G, nxt), chain[1])


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", KINDS)
def test_identities(kind, boundary):
    """Per class sum(dead) + sum(alive) = 262 144 P; a class's alive[] sums to the envelope's population_sum; births and deaths follow
    from the histogram and the table; a table bit outside the used masks changes nothing."""
    P = 4
    rule = rule_of(kind, 2)
    tables = tables_of(kind, rule)
    words = host.seeded_state(G, 31, 2)
    rec = host.usage(words, kind, tables, P, boundary)
    env = host.envelope(words, kind, tables, P, boundary)[0]
    for i, base, key in LOOKS_UP[kind]:
        n = gl.SIZES[key]
        assert int(rec["dead"][base:base + n].sum()) + int(rec["alive"][base:base + n].sum()) == CELLS * P
        assert int(rec["alive"][base:base + n].sum()) == int(env["population_sum"])
    looked_up = sum(gl.SIZES[key] for _, _, key in LOOKS_UP[kind])
    assert int(rec["dead"].sum()) + int(rec["alive"].sum()) == CELLS * P * len(LOOKS_UP[kind])
    assert not rec["dead"][looked_up:].any() or kind == "clustered"
    chain = [words]
    for _ in range(P):
        chain.append(host.ensemble_step(chain[-1], kind, tables, boundary))
    if kind == "clustered":
        with pytest.raises(ValueError):
            host.usage_births_deaths(rec, kind, tables)
    else:
        cells = [gl.unpack(G, w).astype(bool) for w in chain]
        births = sum(int((~a & b).sum()) for a, b in zip(cells, cells[1:]))
        deaths = sum(int((a & ~b).sum()) for a, b in zip(cells, cells[1:]))
        assert host.usage_births_deaths(rec, kind, tables) == (births, deaths) and births and deaths


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", KINDS)
def test_dont_care_bits_change_nothing(kind, boundary):
    """Flip every table bit that was never read, and the chain stays: on a soup under a coded rule, and on a sparse one that grows slowly, where
    the high counts of every class stay unread."""
    slow = gl._rule("born at 2", 1 << 2, 0b111)
    slow = (slow, slow, slow) if kind == "clustered" else slow
    for words, rule, P, some in ((host.seeded_state(G, 31, 2), rule_of(kind, 2), 4, False), (host.seeded_state(G, 32, 6), slow, 2, True)):
        tables = tables_of(kind, rule)
        rec = host.usage(words, kind, tables, P, boundary)
        born_dc, survive_dc = host.usage_dont_care(rec, kind)
        if kind == "clustered":
            assert any(born_dc) and any(survive_dc) or not some
            flipped = [b ^ d for b, d in zip(tables[0], born_dc)], [s ^ d for s, d in zip(tables[1], survive_dc)]
        else:
            assert born_dc[1:] == (0, 0) and survive_dc[1:] == (0, 0)
            assert born_dc[0] and survive_dc[0] or not some
            flipped = tables[0] ^ born_dc[0], tables[1] ^ survive_dc[0]
        want, got = words, words
        for t in range(P):
            want, got = host.ensemble_step(want, kind, tables, boundary), host.ensemble_step(got, kind, flipped, boundary)
            assert np.array_equal(want, got), t
        assert want.any()


def test_full_and_empty_in_closed_form():
    full, empty = np.full(W, 0xFFFFFFFF, dtype=np.uint32), np.zeros(W, dtype=np.uint32)
    rec = host.usage(full, "moore", (0, (1 << 27) - 1), 5, "torus")
    assert int(rec["alive"][26]) == CELLS * 5 and int(rec["alive"].sum()) == CELLS * 5 and not rec["dead"].any()
    assert tuple(rec["used_survive"]) == (1 << 26, 0, 0) and tuple(rec["used_born"]) == (0, 0, 0)
    rec = host.usage(empty, "clustered", ([0, 0, 0], [0, 0, 0]), 2, "closed")
    assert [int(rec["dead"][b]) for b in (0, 27, 40)] == [2 * CELLS] * 3 and int(rec["dead"].sum()) == 6 * CELLS and not rec["alive"].any()
    # a full closed cube under von Neumann: 62^3 cells see six neighbours, a face's interior five, an edge's four, a corner three
    rec = host.usage(full, "von neumann", (0, 0x7F), 1, "closed")
    assert [int(v) for v in rec["alive"][:7]] == [0, 0, 0, 8, 12 * 62, 6 * 62 * 62, 62 ** 3]


def test_refusals():
    first = np.zeros(W, dtype=np.uint32)
    for bad in (0, host.CANON_MAX_PERIOD + 1):
        with pytest.raises(ValueError):
            host.usage(first, "moore", (0, 0), bad)
    with pytest.raises(ValueError):
        host.usage(first, "hex", (0, 0), 1)
    with pytest.raises(ValueError):
        host.usage(first, "moore", (0, 0), 1, "mirror")
    with pytest.raises(ValueError):
        host.usage(np.zeros(100, dtype=np.uint32), "moore", (0, 0), 1)
    with pytest.raises(ValueError):
        host.usage_of_phases([], "moore")


def test_symbol_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_usage\(ca3d_ensemble_t \*e, uint32_t first, uint32_t count, const uint32_t \*steps /\* \[count\] \*/,\s*"
                     r"ca3d_usage \*out /\* \[count\] \*/, float \*gpu_ms /\* may be NULL \*/\);", header, flags=re.M)
    assert re.search(r"typedef struct ca3d_usage\s*\{[^}]*uint32_t steps;[^}]*uint32_t flags;[^}]*uint32_t used_born\[3\];[^}]*uint32_t used_survive\[3\];"
                     r"[^}]*uint32_t dead\[49\];[^}]*uint32_t alive\[49\];[^}]*uint32_t reserved\[2\];[^}]*\} ca3d_usage;", header)
    for name, value in (("MAIN", 0), ("EDGES", 27), ("CORNERS", 40), ("BINS", 49)):
        assert re.search(r"^#define CA3D_USAGE_%s %du\b" % (name, value), header, flags=re.M), name
    assert (host.USAGE_MAIN, host.USAGE_EDGES, host.USAGE_CORNERS, host.USAGE_BINS) == (0, 27, 40, 49)
    assert host.USAGE_CLASSES == {"main": (0, 27), "edges": (27, 13), "corners": (40, 9)}
    assert "ca3d_ensemble_usage" in bound and hasattr(lib, "ca3d_ensemble_usage") and len(bound["ca3d_ensemble_usage"]) == 6
    assert C.sizeof(_capi.UsageStruct) == 432 == host.USAGE_DTYPE.itemsize
    assert [(n, host.USAGE_DTYPE.fields[n][1]) for n in host.USAGE_DTYPE.names] == \
        [(n, getattr(_capi.UsageStruct, n).offset) for n, _ in _capi.UsageStruct._fields_]
    declared = set(re.findall(r"^(?:int|const char \*|void) ?\*?(ca3d_\w+)\(", header, flags=re.M))
    assert declared == set(bound), declared ^ set(bound)
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    mk = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bca_usage\.o\b", mk, flags=re.M)


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.UsageStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    steps = (C.c_uint32 * 2)(4, 4)
    ms = C.c_float(-1.0)
    assert lib.ca3d_ensemble_usage(None, 0, 2, steps, out, C.byref(ms)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(steps) == [4, 4] and ms.value == -1.0


def test_python_and_js_surfaces():
    for name in ("usage", "usage_gpu_ms"):
        assert callable(getattr(Ensemble, name)), name
    for name in ("USAGE_DTYPE", "usage", "usage_of_phases", "usage_dont_care", "usage_births_deaths", "USAGE_CLASSES", "USAGE_BINS"):
        assert hasattr(host, name), name
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    assert re.search(r"^\tusage\(steps, opts\)$", js, flags=re.M) and "ensembleUsage(" in js
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert '{"ensembleUsage", js_ensemble_usage}' in napi and "ca3d_ensemble_usage(" in napi
