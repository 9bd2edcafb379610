"""Graded states and rule families — TEST INFRASTRUCTURE shared by test_graded_cpu.py and test_gpu_rule_tables.py.

A graded state is dense enough at one end to reach every count a cell can have (a random fill at density 1/2 holds one or two cells
of a 64^3 grid with 24 or more live neighbours), and the two rule families give every table bit an answer of its own. `class_counts`
is a plain numpy restatement of the three neighbour classes; test_graded_cpu.py pins it to the oracle."""
from collections import namedtuple

import numpy as np

from cellularautomatons3d_amd import host

AXES = {"x": 2, "y": 1, "z": 0}  # the axis of a [z, y, x] cell array
# (axis, reverse) by name: the dense end meets the + face (which wraps) on every axis and, reversed, the dead - face of z
ORIENTATIONS = {"z": ("z", False), "y": ("y", False), "x": ("x", False), "zr": ("z", True)}
SEEDS = (501, 502, 503)
# entries of a table: von Neumann faces, the Moore total, and the clustered classes main (the Moore total), edges, corners
TABLES = {"vn": 7, "moore": 27, "main": 27, "edges": 13, "corners": 9}
CLASSES = ("main", "edges", "corners")


def unpack(G, words):
    """Packed words -> uint8 cells [z, y, x]: bit k of word i is x = 32 (i mod cols) + k."""
    w = np.ascontiguousarray(words, dtype="<u4").ravel()
    assert w.size == (G // 32) * G * G
    return np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G)


def pack(G, cells):
    """uint8 / bool cells [z, y, x] -> packed words."""
    c = np.ascontiguousarray(cells).astype(np.uint8)
    assert c.shape == (G, G, G)
    return np.packbits(c.ravel(), bitorder="little").view("<u4").astype(np.uint32)


def graded_state(G, axis, reverse=False, seeds=SEEDS):
    """Three independent host.random_fill bit planes number every cell n = 0 .. 7; a cell is alive iff n < min(9 c // G, 8), c its
    coordinate on `axis` (G - 1 - c reversed): the density rises from 0 to 1 in steps of 1/8 and the last block is full."""
    n_words = (G // 32) * G * G
    n = sum(unpack(G, host.random_fill(n_words, seed=s)) << k for k, s in enumerate(seeds))
    c = np.arange(G)
    if reverse:
        c = G - 1 - c
    thr = np.minimum(9 * c // G, 8)
    shape = [1, 1, 1]
    shape[AXES[axis]] = G
    return pack(G, n < thr.reshape(shape))


def _neighbour(cells, d, axis):
    """cells at coordinate + d on `axis` with the project's boundary: coordinate -1 is dead, coordinate G wraps to 0."""
    if d == 0:
        return cells
    out = np.roll(cells, -d, axis=axis)
    if d < 0:
        idx = [slice(None)] * 3
        idx[axis] = 0
        out[tuple(idx)] = 0
    return out


def class_counts(G, words):
    """(F, E, C) per cell, int32 [z, y, x]: live face (0 .. 6), edge (0 .. 12) and corner (0 .. 8) neighbours, from 26 shifted copies,
    each axis applying its own boundary. The Moore total is T = F + E + C."""
    cells = unpack(G, words)
    out = [np.zeros((G, G, G), dtype=np.int32) for _ in range(4)]
    for dz in (-1, 0, 1):
        sz = _neighbour(cells, dz, 0)
        for dy in (-1, 0, 1):
            sy = _neighbour(sz, dy, 1)
            for dx in (-1, 0, 1):
                out[abs(dx) + abs(dy) + abs(dz)] += _neighbour(sy, dx, 2)
    return out[1], out[2], out[3]


def counts_of(G, words):
    """dict(F, E, C, T) of class_counts."""
    F, E, C = class_counts(G, words)
    return {"F": F, "E": E, "C": C, "T": F + E + C}


def lookup(alive, count, born, survive):
    """The table pair (masks) applied cell by cell: a dead cell is born at bit `count` of born, a live one survives at that bit of
    survive."""
    count = count.astype(np.uint32)
    return np.where(alive.astype(bool), (np.uint32(survive) >> count) & 1, (np.uint32(born) >> count) & 1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ rule families

Rule = namedtuple("Rule", "name born survive born_str survive_str")  # masks (bit c = at count c) and the same as rule strings


def mask_string(mask):
    return ",".join(str(c) for c in range(32) if mask >> c & 1)


def _rule(name, born, survive):
    return Rule(name, born, survive, mask_string(born), mask_string(survive))


def one_hot(N):
    """2 N rules over a table of N entries: only born bit k, then only survive bit k."""
    return [_rule(f"born bit {k}", 1 << k, 0) for k in range(N)] + [_rule(f"survive bit {k}", 0, 1 << k) for k in range(N)]


def coded_bits(N):
    return (N - 1).bit_length()


def coded(N):
    """2 ceil(log2 N) rules: rule j is born at count c iff bit j of c is set and survives at the other counts; the second half swaps
    born and survive. Any two counts are answered differently by some rule, and born and survive differ at every count."""
    full = (1 << N) - 1
    sel = [sum(1 << c for c in range(N) if c >> j & 1) for j in range(coded_bits(N))]
    return [_rule(f"coded bit {j}, born where set", m, full & ~m) for j, m in enumerate(sel)] + \
           [_rule(f"coded bit {j}, survive where set", full & ~m, m) for j, m in enumerate(sel)]


SILENT = _rule("silent", 0, 0)


def clustered(cls, rule):
    """The clustered rule (main, edges, corners) in which only class `cls` fires."""
    return tuple(rule if c == cls else SILENT for c in CLASSES)


def coded_all(j):
    """All three classes coded at once: class s runs coded rule (j + s) mod its family size."""
    fams = [coded(TABLES[c]) for c in CLASSES]
    return tuple(f[(j + s) % len(f)] for s, f in enumerate(fams))


def strings_of(kind, rule):
    """The keyword arguments of oracle_lib.Rules.from_strings / set_rule_strings. kind "vn" / "moore": `rule` is a Rule and the sides keep
    the silent default; kind "clustered": `rule` is a (main, edges, corners) triple of Rules."""
    if kind == "vn":
        return dict(neighbourhood="von neumann", born=rule.born_str, survive=rule.survive_str)
    if kind == "moore":
        return dict(neighbourhood="moore", born=rule.born_str, survive=rule.survive_str)
    assert kind == "clustered"
    m, e, c = rule
    return dict(neighbourhood="moore", born=m.born_str, survive=m.survive_str, born_edges=e.born_str, survive_edges=e.survive_str,
                born_corners=c.born_str, survive_corners=c.survive_str)


def name_of(kind, rule):
    if kind != "clustered":
        return f"{kind} table: {rule.name}"
    return "clustered " + "; ".join(f"{c} table: {r.name}" for c, r in zip(CLASSES, rule) if r is not SILENT)


def next_state(G, words, kind, rule, counts=None):
    """The next state from class_counts and the tables alone (no oracle)."""
    alive = unpack(G, words)
    n = counts_of(G, words) if counts is None else counts
    if kind == "vn":
        out = lookup(alive, n["F"], rule.born, rule.survive)
    elif kind == "moore":
        out = lookup(alive, n["T"], rule.born, rule.survive)
    else:
        out = np.zeros_like(alive)
        for r, key in zip(rule, "TEC"):
            out |= lookup(alive, n[key], r.born, r.survive)
    return pack(G, out)


def coverage(G, words, counts=None):
    """{"T" | "F" | "E" | "C": int64 [2, N]}: how many (alive, count) pairs of each kind the state holds."""
    alive = unpack(G, words).astype(np.int64)
    n = counts_of(G, words) if counts is None else counts
    sizes = {"T": 27, "F": 7, "E": 13, "C": 9}
    return {k: np.bincount((alive * sizes[k] + n[k]).ravel(), minlength=2 * sizes[k]).reshape(2, sizes[k]) for k in sizes}
