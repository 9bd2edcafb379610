"""What the canon tests share (tests/test_canon_cpu.py, tests/test_gpu_canon.py, tests/test_js_canon.py): small shapes with the order of
their symmetry group, a brute force of `ca3d_ensemble_canon` that goes through neither `host.canon` nor `host.compose` — the WHOLE
unpacked 64^3 array under np.transpose and np.flip, moved to the origin, packed, `host.state_summary`'s digest — and `reference`,
`host.canon` of a state, computed once per run and never changed."""
import itertools

import numpy as np

import census_cases as cc
from cellularautomatons3d_amd import host

G, W = 64, 8192


def cells_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def words_of(cells):
    return np.packbits(np.asarray(cells, dtype=np.uint8).ravel(), bitorder="little").view("<u4").astype(np.uint32)


#: name -> (cells, the order of the symmetry group by construction)
SHAPES = {
    "cell": ([(20, 31, 4)], 48),
    "block": ([(31 + i, 5 + j, 3 + k) for i, j, k in itertools.product(range(2), repeat=3)], 48),
    "rod": ([(9, 60, 58 + k) for k in range(3)], 16),
    "flat_l": ([(40, 15, 16), (41, 15, 16), (40, 16, 16)], 4),
    "shape": (cc.shape_at(cc.PLACES[1]), 1),
    "slab": ([(x, 30 + j, 7 + k) for x in range(64) for j in range(3) for k in range(2)], 8),
}


def shape_words(name):
    return cc.words(SHAPES[name][0])


def to_origin(c):
    """The cells [z, y, x] translated so that their bounding box starts at the origin."""
    out = np.zeros_like(c)
    idx = np.nonzero(c)
    if idx[0].size:
        out[tuple(i - i.min() for i in idx)] = 1
    return out


def turned(words, o):
    """T_o of the state, as cells [z, y, x]: the whole array indexed [x, y, z], its axes permuted and mirrored, moved to the origin."""
    c = cells_of(words).transpose(2, 1, 0)  # [x, y, z]
    t = np.transpose(c, host.ORIENTATION_PERMS[o % 6])
    t = np.flip(t, axis=[i for i in range(3) if (o // 6) >> i & 1])
    return to_origin(np.ascontiguousarray(t.transpose(2, 1, 0)))


def brute(words):
    """-> (key, orientation, symmetry mask, digests u64[48]) by the definition, the slow way."""
    t0 = turned(words, 0)
    digests = np.zeros(48, dtype=np.uint64)
    symmetry = 0
    for o in range(48):
        t = turned(words, o)
        digests[o] = host.state_summary(G, words_of(t))["digest"]
        if np.array_equal(t, t0):
            symmetry |= 1 << o
    key = min(int(d) for d in digests)
    return key, [int(d) for d in digests].index(key), symmetry, digests


def mirrors(o):
    return int(round(np.linalg.det(host.orientation_matrix(o)))) == -1


_REF = {}


def reference(key, words):
    """`host.canon(words)`, kept under `key` for the run."""
    if key not in _REF:
        rec, dig = host.canon(words)
        dig.setflags(write=False)
        _REF[key] = (rec, dig)
    return _REF[key]


def assert_record(got_rec, got_dig, want, what):
    """A device (or addon) record and its 48 digests against `host.canon`'s, field by field."""
    rec, dig = want
    np.testing.assert_array_equal(np.asarray(got_dig, dtype=np.uint64), dig, err_msg=f"{what}: digests")
    for f in ("key", "symmetry", "orientation", "population", "box_min", "box_max"):
        assert int(got_rec[f]) == int(rec[f]), (what, f, int(got_rec[f]), int(rec[f]))
