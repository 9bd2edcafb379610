"""host.ensemble_step — the numpy definition of an ensemble universe's step under each boundary — against the CPU oracle, for all three
kinds (no GPU).

  reference  the packed oracle at G = 64, which IS the reference's boundary (- faces dead, + faces wrap);
  torus      the unpacked oracle at G = 64, toroidal at a power-of-two grid: the kind's offset lists, count-indexed tables; clustered is
             three calls (main, edges, corners lists) ORed;
  closed     the same toroidal oracle on a 128^3 array with the universe in its middle and everything outside the 64^3 cube zeroed
             after each step: nothing ever lives behind a face.
Both sides run their own chain of steps from the same state and are compared after 1, 2 and 5 of them."""
import itertools

import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol
from cellularautomatons3d_amd import host

G = 64
KINDS = {"von neumann": "vn", "moore": "moore", "clustered": "clustered"}  # host's name -> graded_lib's
CHECK_AT = (1, 2, 5)
MID = (21, 30, 42)  # a face or edge cell's free coordinates: off the word seam, different on every axis


def rule_of(kind, j):
    """Rule j of the kind's coded family (graded_lib): adjacent counts are answered differently, born and survive differ everywhere."""
    if kind == "clustered":
        return gl.coded_all(j)
    fam = gl.coded(gl.TABLES[KINDS[kind]])
    return fam[j % len(fam)]


def grow_rule(kind):
    """Born at count 1 (clustered: in all three classes), survive at 0 and 2: a single cell spreads through every face it touches."""
    r = gl._rule("born at 1", 1 << 1, 0b101)
    return (r, r, r) if kind == "clustered" else r


def tables_of(kind, rule):
    """What host.ensemble_step takes: the masks of Ensemble.set_rule_tables / set_clustered_tables."""
    if kind == "clustered":
        return [r.born for r in rule], [r.survive for r in rule]
    return rule.born, rule.survive


def lists_of(kind, rule):
    """[(offset list, count-indexed survive, count-indexed born)] for the unpacked oracle; the results are ORed."""
    def arr(mask, n):
        return np.array([mask >> c & 1 for c in range(n)], dtype=np.uint32)

    if kind == "clustered":
        return [(host.NEIGHBOURHOOD_MAP[name], arr(r.survive, n), arr(r.born, n)) for name, n, r in zip(("moore", "edges", "corners"), (27, 13, 9), rule)]
    n = gl.TABLES[KINDS[kind]]
    return [(host.NEIGHBOURHOOD_MAP[kind], arr(rule.survive, n), arr(rule.born, n))]


def torus_step(N, cells, lists):
    """One step of an N^3 torus of u32 cells [z, y, x] by the unpacked oracle."""
    out = np.zeros(N * N * N, dtype=np.uint32)
    for offs, survive, born in lists:
        out |= ol.unpacked_step(N, cells.ravel(), offs, survive, born)
    return out.reshape(N, N, N)


def oracle_states(kind, rule, boundary, words, steps):
    """[state after 1 .. steps steps], packed, by the oracle alone."""
    out = []
    if boundary == "reference":
        r = ol.Rules.from_strings(**gl.strings_of(KINDS[kind], rule))
        cur = np.ascontiguousarray(words, dtype=np.uint32)
        for _ in range(steps):
            cur = ol.packed_step(G, cur, r)
            out.append(cur)
        return out
    lists = lists_of(kind, rule)
    if boundary == "torus":
        cells = gl.unpack(G, words).astype(np.uint32)
        for _ in range(steps):
            cells = torus_step(G, cells, lists)
            out.append(gl.pack(G, cells))
        return out
    assert boundary == "closed"
    N, o = 2 * G, G // 2
    cube = (slice(o, o + G),) * 3
    big = np.zeros((N, N, N), dtype=np.uint32)
    big[cube] = gl.unpack(G, words)
    for _ in range(steps):
        stepped = torus_step(N, big, lists)
        big = np.zeros_like(stepped)
        big[cube] = stepped[cube]  # everything outside the cube is dead again
        out.append(gl.pack(G, big[cube]))
    return out


def check(kind, rule, boundary, words, what):
    want = oracle_states(kind, rule, boundary, words, max(CHECK_AT))
    cur = np.ascontiguousarray(words, dtype=np.uint32)
    tables = tables_of(kind, rule)
    for t in range(1, max(CHECK_AT) + 1):
        cur = host.ensemble_step(cur, kind, tables, boundary)
        if t in CHECK_AT:
            assert np.array_equal(cur, want[t - 1]), f"{kind}, {boundary}, {what}: differs from the oracle after {t} steps"
    return cur


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_soups(kind, boundary):
    """A dense fill (density 1/2) and a sparse one (2^-4), under two rules each."""
    for j, (seed, rounds) in enumerate(((11, 0), (12, 3))):
        words = host.seeded_state(G, seed, rounds)
        for rule in (rule_of(kind, j), grow_rule(kind)):
            check(kind, rule, boundary, words, f"seed {seed}, and_rounds {rounds}")


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_graded_states_reach_every_count(kind, boundary):
    """The graded states of graded_lib: the dense end lies on a + face on every axis and, reversed, on the - face of z."""
    for j, (name, (axis, reverse)) in enumerate(gl.ORIENTATIONS.items()):
        words = gl.graded_state(G, axis, reverse)
        check(kind, rule_of(kind, j), boundary, words, f"graded along {name}")


def face_cells():
    """The 26 cells on the 6 faces, 12 edges and 8 corners of the cube: every coordinate 0, free, or 63, not all free."""
    out = []
    for pick in itertools.product((0, 1, 2), repeat=3):
        if pick != (1, 1, 1):
            out.append(tuple((0, MID[i], G - 1)[p] for i, p in enumerate(pick)))
    assert len(out) == 26
    return out


@pytest.mark.parametrize("boundary", host.ENSEMBLE_BOUNDARIES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_single_cells_on_faces_edges_and_corners(kind, boundary):
    rule = grow_rule(kind)
    for cell in face_cells():
        last = check(kind, rule, boundary, host.cells_to_words(G, [cell]), f"one cell at {cell}")
        assert last.any()


def test_modes_differ_and_agree_where_they_must():
    """One cell in a corner under Moore, born at 1: it and the cells that see it are alive afterwards. In the reference's boundary a cell
    on a + face looks across it (coordinate 64 is 0) and one on a - face does not, so the cell at the origin is seen from all 26 sides and
    the one in the far corner from 7. Away from every face the three boundaries agree."""
    tables = tables_of("moore", grow_rule("moore"))
    corner = host.cells_to_words(G, [(0, 0, 0)])
    got = {b: int(gl.unpack(G, host.ensemble_step(corner, "moore", tables, b)).sum()) for b in host.ENSEMBLE_BOUNDARIES}
    assert got == {"reference": 27, "torus": 27, "closed": 8}
    corner = host.cells_to_words(G, [(G - 1, G - 1, G - 1)])
    got = {b: int(gl.unpack(G, host.ensemble_step(corner, "moore", tables, b)).sum()) for b in host.ENSEMBLE_BOUNDARIES}
    assert got == {"reference": 8, "torus": 27, "closed": 8}
    inside = host.cells_to_words(G, [MID])
    states = [host.ensemble_step(inside, "moore", tables, b) for b in host.ENSEMBLE_BOUNDARIES]
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])


def test_refusals():
    words = np.zeros(8192, dtype=np.uint32)
    with pytest.raises(ValueError):
        host.ensemble_step(words, "moore", (0, 0), "mirror")
    with pytest.raises(ValueError):
        host.ensemble_step(words, "hex", (0, 0), "torus")
    with pytest.raises(ValueError):
        host.ensemble_step(words[:100], "moore", (0, 0), "torus")
