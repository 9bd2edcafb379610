"""The torus census' host side (`ca3d_ensemble_census_connected` with CA3D_CONNECT_TORUS, include/ca3d.h): `host.census(...,
connectivity="torus")`, the numpy restatement of the definition, against `scipy.ndimage.label` of the state padded by one wrapped cell;
the cyclic box against the brute-force shortest covering interval and against the form the device uses; roll invariance of the
(population, digest) list; `connectivity="closed"` is the census as it was; the symbols and the refusals that need no device. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import census_cases as cc
import objects_torus_cases as tc
from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64


def labelled_on_the_torus(words):
    """[(first_cell, population)] of the torus components by scipy: the state padded by one cell with mode="wrap", labelled with the
    full 3 x 3 x 3 structure, every padded cell united with the cell it is a copy of."""
    ndimage = pytest.importorskip("scipy.ndimage")
    cells = tc.cells_of(words)
    padded = np.pad(cells, 1, mode="wrap")
    lab, n = ndimage.label(padded, structure=np.ones((3, 3, 3), dtype=int))
    parent = list(range(n + 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    source = np.pad(lab[1:-1, 1:-1, 1:-1], 1, mode="wrap")  # the label of the cell each padded cell copies
    shell = np.ones_like(lab, dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    for a, b in set(zip(lab[shell & (lab > 0)].tolist(), source[shell & (lab > 0)].tolist())):
        parent[find(a)] = find(b)
    inner = lab[1:-1, 1:-1, 1:-1].ravel()  # flat index = x + 64 y + 4096 z
    root = np.array([find(a) for a in range(n + 1)])[inner]
    out = []
    for r in np.unique(root[inner > 0]):
        at = np.flatnonzero((root == r) & (inner > 0))
        out.append((int(at[0]), int(at.size)))
    return sorted(out)


def brute_span(coords):
    """The shortest cyclic interval that covers the coordinates and starts at one of them, ties to the smallest start, by trying
    every start and every length."""
    S = set(int(c) % G for c in coords)
    best = None
    for s in sorted(S):
        e = next(e for e in range(1, G + 1) if S <= {(s + i) % G for i in range(e)})
        if best is None or e < best[1]:
            best = (s, e)
    return best


def device_span(coords):
    """The same from the occupancy mask as the kernels read it: the set bit whose predecessor is clear, and the number of set bits."""
    m = 0
    for c in coords:
        m |= 1 << (int(c) % G)
    full = (1 << G) - 1
    pred = ((m << 1) | (m >> (G - 1))) & full
    starts = m & ~pred & full
    assert m == full or bin(starts).count("1") == 1  # a single cyclic run
    return (0 if m == full else (starts & -starts).bit_length() - 1), bin(m).count("1")


CASES = [(name, d) for name in tc.ROLLED for d in tc.ROLLS] + [("full", (0, 0, 0)), ("empty", (0, 0, 0)), ("soup", (40, 50, 60)), ("giant", (33, 1, 63))]


@pytest.mark.parametrize("name,d", CASES)
def test_host_torus_census_against_scipy(name, d):
    words = tc.state(name, d)
    comps, n, rest = tc.reference((name, d), words, 1024)
    want = labelled_on_the_torus(words)
    assert rest == 0 and n == len(want)
    assert [(int(c["first_cell"]), int(c["population"])) for c in comps[:n]] == want
    assert not comps[n:].tobytes().strip(b"\0") and not comps["reserved"].any()
    if name in ("faces_x", "faces_y", "faces_z", "corners"):
        assert n == 1  # what the closed census splits in 2, 2, 2 and 8
    # the box: the general definition, and the single run the device relies on
    cells = tc.cells_of(words)
    for c in comps[:n]:
        zs, ys, xs = np.nonzero(tc.cells_of(host.isolate(words, int(c["first_cell"]), "keep", "torus")[0]))
        assert zs.size == int(c["population"])
        lo, hi = host.unpack_box(c["box_min"]), host.unpack_box(c["box_max"])
        for axis, v in enumerate((xs, ys, zs)):
            s, e = brute_span(v)
            assert host.torus_span(v) == (s, e) == device_span(v)
            assert (lo[axis], hi[axis]) == (s, s + e - 1)
    assert int(comps["population"][:n].sum()) == int(cells.sum())


def test_what_the_box_says_at_a_seam():
    for axis in range(3):
        ring = tc.rod(axis)
        comps, n, rest = host.census(host.cells_to_words(G, ring), 4, "torus")
        assert (n, rest, int(comps["population"][0])) == (1, 0, 64)
        assert host.unpack_box(comps["box_min"][0])[axis] == 0 and host.unpack_box(comps["box_max"][0])[axis] == 63
        for missing, start in (((0,), 1), ((63,), 0), ((31, 32), 33)):
            comps, n, rest = host.census(host.cells_to_words(G, tc.rod(axis, missing)), 4, "torus")
            assert (n, rest, int(comps["population"][0])) == (1, 0, 64 - len(missing)), (axis, missing)
            lo, hi = host.unpack_box(comps["box_min"][0])[axis], host.unpack_box(comps["box_max"][0])[axis]
            assert (lo, hi) == (start, start + 63 - len(missing)) and (hi >= 64) == (start + 63 - len(missing) >= 64)
        # the closed census of the rod with a gap in the middle finds two pieces
        assert host.census(host.cells_to_words(G, tc.rod(axis, (31, 32))), 4, "closed")[1] == 2
    assert host.torus_span([5, 37]) == (5, 33) and host.torus_span([5, 38]) == (38, 32) and host.torus_span(range(64)) == (0, 64)


@pytest.mark.parametrize("name", ["soup"] + tc.CLEAR)
def test_roll_invariance(name):
    """A state clear of the faces: the torus census of any roll of it names the shapes the closed census names."""
    base = tc.state(name)
    want = tc.shapes(tc.reference((name, "closed"), base, 1024, "closed"))
    if name == "soup":
        assert len(want) > 300
    for d in ((0, 0, 0), (30, 0, 0), (0, 31, 5), (40, 50, 60), (33, 1, 63)):
        assert tc.shapes(tc.reference((name, d), tc.state(name, d), 1024)) == want, d


def test_closed_is_the_census_as_it_was():
    for name in ("shapes", "corners", "giant"):
        old = cc.reference(name, 64)
        new = host.census(cc.state(name), 64, connectivity="closed")
        assert new[0].tobytes() == old[0].tobytes() and new[1:] == old[1:]
    assert host.CONNECTIVITIES == ("closed", "torus")
    with pytest.raises(ValueError):
        host.census(cc.state("empty"), 4, "open")


def test_symbols_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    for name, n_args in (("ca3d_ensemble_census_connected", 9), ("ca3d_ensemble_isolate_connected", 9)):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M) and hasattr(lib, name) and len(bound[name]) == n_args
    assert re.search(r"CA3D_CONNECT_CLOSED = 0,\s*CA3D_CONNECT_TORUS = 1", header)
    assert _capi.CONNECTIVITIES == {"closed": 0, "torus": 1}
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    assert "spans a whole ring" in header  # where equal shapes may have different digests


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.ComponentStruct * 4)()
    n, rest = (C.c_uint32 * 1)(77), (C.c_uint32 * 1)(77)
    assert lib.ca3d_ensemble_census_connected(None, 0, 1, 4, 1, out, n, rest, None) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert (n[0], rest[0]) == (77, 77) and not bytes(out).strip(b"\0")
    assert lib.ca3d_ensemble_isolate_connected(None, 0, None, 1, None, 0, 1, None, None) == -1
