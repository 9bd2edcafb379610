"""The census's host side (`ca3d_ensemble_census`, include/ca3d.h): `host.census`, the numpy restatement of the definition, against
`scipy.ndimage.label` with a full 3 x 3 x 3 structure on the crafted states of tests/census_cases.py and on the synthetic ones;
truncation; translation invariance of the digest; the symbol, the struct and the refusals that need no device. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import census_cases as cc
from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64


def cells_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def labelled(words):
    """The components by scipy: [(first_cell, population, box_min, box_max, digest)] in the order of their first cells."""
    ndimage = pytest.importorskip("scipy.ndimage")
    cells = cells_of(words)
    lab, n = ndimage.label(cells, structure=np.ones((3, 3, 3), dtype=int))
    out = []
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        part = lab[sl] == k
        zs, ys, xs = np.nonzero(part)
        z0, y0, x0 = (s.start for s in sl)
        first = int(((zs + z0) * 4096 + (ys + y0) * 64 + xs + x0).min())
        moved = np.zeros((G, G, G), dtype=np.uint8)
        moved[zs, ys, xs] = 1  # find_objects' slice is the bounding box: the component translated by -box_min
        digest = host.state_summary(G, np.packbits(moved.ravel(), bitorder="little").view("<u4"))["digest"]
        out.append((first, int(part.sum()), (x0, y0, z0), (sl[2].stop - 1, sl[1].stop - 1, sl[0].stop - 1), digest))
    assert len(out) == n
    return sorted(out)


def as_tuples(comps, n):
    return [(int(c["first_cell"]), int(c["population"]), host.unpack_box(c["box_min"]), host.unpack_box(c["box_max"]), int(c["digest"]))
            for c in comps[:n]]


@pytest.mark.parametrize("name", list(cc.CRAFTED) + ["sparse", "giant"])
def test_host_census_against_scipy(name):
    want = labelled(cc.state(name))
    comps, n, rest = cc.reference(name, 1024)
    assert rest == 0 and n == len(want)  # complete: nothing a truncated list could hide
    assert as_tuples(comps, n) == want
    assert not comps[n:].tobytes().strip(b"\0") and not comps["reserved"].any()
    if name in cc.CRAFTED:
        assert n == cc.CRAFTED[name][1]  # what the state was built to hold
    else:
        _, count, live, largest = cc.SYNTHETIC[name]
        assert (n, int(comps["population"].sum()), int(comps["population"].max())) == (count, live, largest)


def test_closed_faces_and_seams_by_construction():
    """No scipy: the counts the crafted states hold by construction, and what the lists look like."""
    for name, (_, count) in cc.CRAFTED.items():
        if name in ("serpentine", "full"):
            continue  # (long fills: the scipy comparison runs them once)
        comps, n, rest = cc.reference(name, 1024)
        assert (n, rest) == (count, 0), name
        assert np.all(np.diff(comps["first_cell"][:n].astype(np.int64)) > 0), name  # ordered by first cell
    comps, n, _ = cc.reference("corners", 1024)
    assert [host.unpack_box(b) for b in comps["box_min"][:n]] == [(x, y, z) for z in (0, 63) for y in (0, 63) for x in (0, 63)]
    comps, n, _ = cc.reference("shell_core", 1024)
    assert [int(p) for p in comps["population"][:2]] == [9 ** 3 - 7 ** 3, 27]  # the shell's first cell is the lower one
    assert host.unpack_box(comps["box_min"][0]) == (27, 12, 2) and host.unpack_box(comps["box_min"][1]) == (30, 15, 5)


def test_truncation():
    full, n_full, _ = cc.reference("sparse", 1024)
    comps, n, rest = cc.reference("sparse", 256)
    assert (n_full, n) == (509, 256)
    assert comps.tobytes() == full[:256].tobytes()  # the 256 first
    assert rest == 518 - int(comps["population"].sum()) and rest > 0
    comps, n, rest = host.census(cc.state("shapes"), 2)
    assert (n, rest) == (2, 12) and comps.shape == (2,)
    comps, n, rest = host.census(cc.state("shapes"), 5)
    assert (n, rest) == (3, 0) and not comps[3:].tobytes().strip(b"\0")
    comps, n, rest = cc.reference("dense", 1024)
    assert (n, rest) == (1024, 16472 - int(comps["population"].sum())) and rest > 0
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            host.census(cc.state("empty"), bad)


def test_digest_of_one_shape_at_three_translations():
    comps, n, _ = cc.reference("shapes", 64)
    assert n == 3 and len(set(int(d) for d in comps["digest"][:3])) == 1 and [int(p) for p in comps["population"][:3]] == [12] * 3
    assert [host.unpack_box(b) for b in comps["box_min"][:3]] == list(cc.PLACES)
    assert [host.unpack_box(b) for b in comps["box_max"][:3]] == [(x + 5, y + 2, z + 3) for x, y, z in cc.PLACES]
    at_origin = host.state_summary(G, host.cells_to_words(G, cc.SHAPE))["digest"]
    assert int(comps["digest"][0]) == at_origin
    # another shape of 12 cells has another digest
    other = host.cells_to_words(G, [(x, 0, 0) for x in range(12)])
    assert int(host.census(other, 1)[0]["digest"][0]) != at_origin


def test_unpack_box():
    assert host.unpack_box(5 | 63 << 8 | 17 << 16) == (5, 63, 17)
    assert host.unpack_box(np.uint32(0x003F3F3F)) == (63, 63, 63)


def test_symbol_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_census\(", header, flags=re.M)
    assert "ca3d_ensemble_census" in bound and hasattr(lib, "ca3d_ensemble_census")
    assert len(bound["ca3d_ensemble_census"]) == 8 and bound["ca3d_ensemble_census"][4] is C.POINTER(_capi.ComponentStruct)
    assert C.sizeof(_capi.ComponentStruct) == 32 == host.COMPONENT_DTYPE.itemsize
    for (name, ctype), field in zip(_capi.ComponentStruct._fields_, host.COMPONENT_DTYPE.names):  # the two layouts are one
        assert name == field and getattr(_capi.ComponentStruct, name).offset == host.COMPONENT_DTYPE.fields[field][1]
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    assert "CLOSED BOX" in header and "no face wraps" in header  # the header says which boundary the census uses


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.ComponentStruct * 4)()
    n, rest = (C.c_uint32 * 1)(77), (C.c_uint32 * 1)(77)
    assert lib.ca3d_ensemble_census(None, 0, 1, 4, out, n, rest, None) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert (n[0], rest[0]) == (77, 77) and not bytes(out).strip(b"\0")
