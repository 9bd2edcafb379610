"""Crafted 64^3 states for the census tests (tests/test_census_cpu.py, tests/test_gpu_census.py, tests/test_js_census.py): what each is
built to catch, and the number of components it holds by construction. Every state is packed words; `reference(name, max_components)`
is `host.census` of it, computed once per module run and never changed."""
import itertools

import numpy as np

from cellularautomatons3d_amd import host

G = 64

#: the 13 directions of the 26-neighbourhood up to sign (first non-zero component positive)
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0) and next(c for c in d if c) > 0]
#: one asymmetric 12-cell shape, connected, box 6 x 3 x 4
SHAPE = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 1, 1))
#: where it is placed: clear of every seam; across x = 31 | 32 and z = 3 | 4; across z = 59 | 60
PLACES = ((1, 1, 1), (27, 40, 2), (50, 9, 57))


def words(cells):
    return host.cells_to_words(G, cells)


def shape_at(corner):
    return [tuple(c + o for c, o in zip(corner, cell)) for cell in SHAPE]


def faces(axis):
    """Two cells that face each other across the cube on `axis`: adjacent only if that axis wrapped."""
    out = []
    for v in (0, 63):
        c = [20, 37, 9]
        c[axis] = v
        out.append(tuple(c))
    return out


def corners():
    return list(itertools.product((0, 63), repeat=3))


def pair_bases(d):
    """Lower ends b of the pairs (b, b + k d) of direction d: the issue's (31, 5, 3), and three whose step crosses the word seam
    x = 31 | 32, a seam between lanes 16 apart (y = 15 | 16, 31 | 32, 47 | 48) and a wave seam (z = 3 | 4, 7 | 8, 59 | 60) on every
    axis the direction moves along."""
    dx, dy, dz = d
    bases = [(31, 5, 3)]
    for y, z in ((15, 3), (31, 7), (47, 59)):
        bases.append((31 if dx >= 0 else 32, y if dy >= 0 else y + 1, z if dz >= 0 else z + 1))
    return bases


def pairs(d, distance):
    """Four pairs of cells `distance` steps of d apart, far from one another: 4 components at distance 1, 8 at distance 2."""
    cells = []
    for b in pair_bases(d):
        cells += [b, tuple(c + distance * s for c, s in zip(b, d))]
    assert len(set(cells)) == 8 and all(0 <= v < G for c in cells for v in c)
    return cells


def serpentine():
    """Plane z = 10: the even rows filled, joined at alternating ends — one path of 2 079 cells, about 2 000 flood iterations."""
    cells = [(x, y, 10) for y in range(0, G, 2) for x in range(G)]
    cells += [(63 if (y // 2) % 2 == 0 else 0, y, 10) for y in range(1, G - 1, 2)]
    return cells


def staircase():
    """A staircase up through all 64 planes (x climbs every fourth plane) and down again beside itself at distance 2 in y, joined at
    the top only: one component, and the flood travels through the exchange both ways."""
    up = [(4 + z // 4, 20, z) for z in range(G)]
    down = [(4 + z // 4, 22, z) for z in range(G)]
    return up + [(4 + 63 // 4, 21, 63)] + down


def shell_and_core(corner=(27, 12, 2)):
    """A hollow 9^3 shell (across x = 31 | 32, z = 3 | 4 and 7 | 8) around a separate 3^3 core: overlapping boxes, two components."""
    cx, cy, cz = corner
    shell = [(cx + i, cy + j, cz + k) for i, j, k in itertools.product(range(9), repeat=3) if 0 in (i, j, k) or 8 in (i, j, k)]
    core = [(cx + i, cy + j, cz + k) for i, j, k in itertools.product(range(3, 6), repeat=3)]
    return shell + core


def _crafted():
    c = {}
    for axis, name in enumerate("xyz"):
        c["faces_" + name] = (words(faces(axis)), 2)
    c["corners"] = (words(corners()), 8)
    for d in DIRECTIONS:
        tag = "".join("-0+"[v + 1] for v in d)
        c["pairs1_" + tag] = (words(pairs(d, 1)), 4)
        c["pairs2_" + tag] = (words(pairs(d, 2)), 8)
    c["serpentine"] = (words(serpentine()), 1)
    c["staircase"] = (words(staircase()), 1)
    c["shell_core"] = (words(shell_and_core()), 2)
    for k, p in enumerate(PLACES):
        c["shape_%d" % k] = (words(shape_at(p)), 1)
    c["shapes"] = (words([cell for p in PLACES for cell in shape_at(p)]), 3)
    c["full"] = (np.full(host.words_per_buffer(G), 0xFFFFFFFF, dtype=np.uint32), 1)
    c["empty"] = (np.zeros(host.words_per_buffer(G), dtype=np.uint32), 0)
    return c


#: name -> (packed words, components by construction)
CRAFTED = _crafted()
#: name -> (arguments of host.seeded_state, components, live cells, the largest component) — counted on the CPU for the issue
SYNTHETIC = {
    "sparse": ((G, 0xCA3D0009, 8), 509, 518, 2),
    "giant": ((G, 77, 2, ((20, 20, 20), (43, 43, 43))), 190, 1739, 1306),
    "dense": ((G, 0xCA3D0004, 3), 6173, 16472, None),
}

_STATES, _REF = {}, {}


def state(name):
    if name not in _STATES:
        s = CRAFTED[name][0] if name in CRAFTED else host.seeded_state(*SYNTHETIC[name][0])
        s.setflags(write=False)
        _STATES[name] = s
    return _STATES[name]


def reference_of(key, words_, max_components):
    """`host.census(words_, max_components)`, kept under `key` for the run."""
    k = (key, max_components)
    if k not in _REF:
        comps, n, rest = host.census(words_, max_components)
        comps.setflags(write=False)
        _REF[k] = (comps, n, rest)
    return _REF[k]


def reference(name, max_components):
    return reference_of(name, state(name), max_components)
