"""States and references shared by the torus census and isolate tests (tests/test_census_torus_cpu.py, test_isolate_torus_cpu.py,
test_gpu_census_torus.py, test_gpu_isolate_torus.py, test_js_census_torus.py). The crafted states are tests/census_cases.py's, rolled
so that their objects cross the word seam, a wave seam or a face; `reference(key, words, max_components, connectivity)` is
`host.census` of a state, computed once per run and never changed."""
import itertools

import numpy as np

import census_cases as cc
from cellularautomatons3d_amd import host

G, W = 64, 8192

#: the two rolls of the issue: half a cube on every axis, and one that puts x on the last column, y one row on and z in the middle of a wave
ROLLS = ((32, 32, 32), (63, 1, 33))
#: the crafted states that go through the rolls (every one but the 26 pair states: their seams are the 13 directions' below)
ROLLED = ["faces_x", "faces_y", "faces_z", "corners", "serpentine", "staircase", "shell_core", "shape_0", "shape_1", "shape_2", "shapes"]
#: those of them whose objects keep clear of every face before the roll: the closed census of the unrolled state names the same shapes
CLEAR = ["shell_core", "shape_0", "shape_1", "shape_2", "shapes"]
#: a soup in a 40^3 box at density 1 / 64, clear of the faces: a few hundred small objects, listed completely at 1024
SOUP = (G, 0xCA3D0013, 5, ((12, 12, 12), (51, 51, 51)))


def cells_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def words_of(cells):
    return np.packbits(np.asarray(cells, dtype=np.uint8).ravel(), bitorder="little").view("<u4").astype(np.uint32)


def rolled(words, d):
    """The state moved cyclically by d = (dx, dy, dz)."""
    return words_of(np.roll(cells_of(words), (d[2], d[1], d[0]), axis=(0, 1, 2)))


def seam_pair(d):
    """Two cells that face each other in direction d (one of the 13) THROUGH a seam on every axis d moves along: adjacent on the
    torus only. Axes d does not move along sit clear of the faces."""
    a = tuple(63 if s > 0 else 0 if s < 0 else 20 + 7 * i for i, s in enumerate(d))
    b = tuple((v + s) % G for v, s in zip(a, d))
    return [a, b]


def rod(axis, missing=()):
    """The 64 cells of a ring around `axis` through (21, 38, 10), without the coordinates in `missing`."""
    cells = []
    for v in range(G):
        if v in missing:
            continue
        c = [21, 38, 10]
        c[axis] = v
        cells.append(tuple(c))
    return cells


_STATES, _REF = {}, {}


def state(name, d=(0, 0, 0)):
    """Crafted state `name` of census_cases (or "soup") rolled by d, read-only."""
    k = (name, tuple(d))
    if k not in _STATES:
        base = host.seeded_state(*SOUP) if name == "soup" else cc.state(name)
        s = rolled(base, d) if any(d) else np.array(base, dtype=np.uint32)
        s.setflags(write=False)
        _STATES[k] = s
    return _STATES[k]


def reference(key, words, max_components, connectivity="torus"):
    """`host.census(words, max_components, connectivity)`, kept under `key` for the run."""
    k = (key, max_components, connectivity)
    if k not in _REF:
        comps, n, rest = host.census(words, max_components, connectivity)
        comps.setflags(write=False)
        _REF[k] = (comps, n, rest)
    return _REF[k]


def shapes(ref):
    """The sorted (population, digest) list of a complete census."""
    comps, n, rest = ref
    assert rest == 0
    return sorted((int(c["population"]), int(c["digest"])) for c in comps[:n])


def cells_list(words):
    """The live cells of a state as x + 64 y + 4096 z, ascending."""
    return np.flatnonzero(cells_of(words).ravel())


DIRECTIONS = cc.DIRECTIONS
assert len(DIRECTIONS) == 13 and len({tuple(sorted(seam_pair(d))) for d in DIRECTIONS}) == 13
assert sorted(itertools.chain.from_iterable(seam_pair((1, 1, 1)))) == [0, 0, 0, 63, 63, 63]
