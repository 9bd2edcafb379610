"""The canon's host side (`ca3d_ensemble_canon`, include/ca3d.h): `host.canon`, the numpy restatement of the definition, against a brute
force that goes through neither it nor `host.compose` (canon_cases.brute: the whole unpacked array under np.transpose and np.flip,
moved to the origin, packed, `host.state_summary`'s digest, symmetry by array equality); the symmetry groups of small shapes; the key
of all 48 turned copies; the symbol, the struct and the Python and JS surfaces. All comparisons are exact. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import canon_cases as kc
import census_cases as cc
from cellularautomatons3d_amd import _capi, host
from cellularautomatons3d_amd.ensemble import Ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = (1 << 48) - 1


def closed(mask):
    """The orientations of `mask` are closed under orientation_matrix products."""
    group = host.symmetry_orientations(mask)
    ms = {o: host.orientation_matrix(o) for o in group}
    return all(host.orientation_from_matrix(ms[a] @ ms[b]) in ms for a in group for b in group)


@pytest.mark.parametrize("name", sorted(kc.SHAPES))
def test_canon_is_the_brute_force(name):
    words = kc.shape_words(name)
    cells, order = kc.SHAPES[name]
    key, o, sym, digests = kc.brute(words)
    assert bin(sym).count("1") == order and sym & 1  # the brute force decides: the group by construction
    rec, dig = host.canon(words)
    assert rec.dtype == host.CANON_DTYPE and dig.dtype == np.uint64 and dig.shape == (48,)
    np.testing.assert_array_equal(dig, digests)
    assert (int(rec["key"]), int(rec["orientation"]), int(rec["symmetry"])) == (key, o, sym)
    assert int(rec["population"]) == len(cells)
    s = host.state_summary(64, words)
    assert host.unpack_box(rec["box_min"]) == tuple(s["box_min"]) and host.unpack_box(rec["box_max"]) == tuple(s["box_max"])
    assert closed(sym)
    assert host.symmetry_orientations(sym) == [i for i in range(48) if sym >> i & 1]
    assert host.is_chiral(sym) == (not any(kc.mirrors(i) for i in host.symmetry_orientations(sym)))
    # digests[0] is the census digest of a universe that holds one object
    comps, n, rest = host.census(words, 2)
    assert (n, rest) == (1, 0) and int(comps[0]["digest"]) == int(dig[0])


def test_shape_is_asymmetric_and_chiral():
    rec, _ = host.canon(kc.shape_words("shape"))
    assert int(rec["symmetry"]) == 1 and host.symmetry_orientations(rec["symmetry"]) == [0]
    assert host.is_chiral(rec["symmetry"])
    for name in ("cell", "block", "rod", "flat_l", "slab"):
        assert not host.is_chiral(host.canon(kc.shape_words(name))[0]["symmetry"]), name
    assert not host.is_chiral(FULL) and host.is_chiral(1)
    # the 24 rotations: a group without a mirror
    rotations = sum(1 << o for o in range(48) if not kc.mirrors(o))
    assert host.is_chiral(rotations) and len(host.symmetry_orientations(rotations)) == 24


def test_full_and_empty_universe():
    full, empty = cc.state("full"), cc.state("empty")
    key, o, sym, digests = kc.brute(full)
    rec, dig = host.canon(full)
    np.testing.assert_array_equal(dig, digests)
    assert (int(rec["key"]), int(rec["orientation"]), int(rec["symmetry"])) == (key, o, sym) == (int(digests[0]), 0, FULL)
    assert int(rec["population"]) == 1 << 18 and int(rec["box_min"]) == 0 and int(rec["box_max"]) == 63 | 63 << 8 | 63 << 16
    assert int(rec["key"]) == host.state_summary(64, full)["digest"]
    rec, dig = host.canon(empty)
    assert not dig.any()
    assert [int(rec[f]) for f in ("key", "orientation", "symmetry", "population", "box_min", "box_max")] == [0, 0, FULL, 0, 0, 0]
    key, o, sym, digests = kc.brute(empty)
    assert (key, o, sym) == (0, 0, FULL) and not digests.any()


def test_crafted_states_and_a_soup_against_the_brute_force():
    """Several objects in one universe are one constellation; a dense state takes the same path as a small one."""
    states = {n: cc.state(n) for n in ("shapes", "shell_core", "corners", "staircase", "faces_x", "pairs2_+-+")}
    states["soup"] = host.random_fill(kc.W, seed=11, and_rounds=1)
    for name, words in states.items():
        key, o, sym, digests = kc.brute(words)
        rec, dig = host.canon(words)
        np.testing.assert_array_equal(dig, digests, err_msg=name)
        assert (int(rec["key"]), int(rec["orientation"]), int(rec["symmetry"])) == (key, o, sym), name
        assert closed(sym), name


def test_all_48_copies_at_three_places_share_one_key():
    """SHAPE turned by every orientation and put at three places: one key, 48 different census digests; `orientation` turns each copy
    into a state whose digest is the key."""
    state = cc.state("shape_1")
    keys, firsts = set(), set()
    for o in range(48):
        for at in cc.PLACES:
            copy, crec = host.compose([state], [(0, o, at)])
            assert int(crec["clipped"]) == 0
            rec, dig = host.canon(copy)
            keys.add(int(rec["key"]))
            firsts.add(int(dig[0]))
            assert int(rec["symmetry"]) == 1
            back, _ = host.compose([copy], [(0, int(rec["orientation"]), (0, 0, 0))])
            assert host.state_summary(64, back)["digest"] == int(rec["key"])
            assert sorted(int(d) for d in dig) == sorted(int(d) for d in kc.reference("shape_1", state)[1])
    assert len(keys) == 1 and len(firsts) == 48


def test_a_dense_soup_stays_quick():
    import time
    words = host.random_fill(kc.W, seed=5, and_rounds=0)
    t = time.perf_counter()
    host.canon(words)
    took = time.perf_counter() - t
    print("host.canon of a dense soup: %.3f s" % took)
    assert took < 1.0  # about 0.1 s is the aim; the bound only catches the uncropped, cell-by-cell form


def test_canon_refuses_a_wrong_size():
    with pytest.raises(ValueError):
        host.canon(np.zeros(100, dtype=np.uint32))


def test_symbol_struct_and_header():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int ca3d_ensemble_canon\(ca3d_ensemble_t \*e, uint32_t first, uint32_t count, ca3d_canon \*out", header, flags=re.M)
    assert re.search(r"typedef struct ca3d_canon\s*\{[^}]*uint64_t key;[^}]*uint64_t symmetry;[^}]*uint32_t orientation;[^}]*uint32_t population;"
                     r"[^}]*uint32_t box_min, box_max;[^}]*\} ca3d_canon;", header)
    assert "ca3d_ensemble_canon" in bound and hasattr(lib, "ca3d_ensemble_canon")
    assert len(bound["ca3d_ensemble_canon"]) == 6
    assert C.sizeof(_capi.CanonStruct) == 32 == host.CANON_DTYPE.itemsize
    assert [(n, host.CANON_DTYPE.fields[n][1]) for n in host.CANON_DTYPE.names] == [(n, getattr(_capi.CanonStruct, n).offset) for n, _ in _capi.CanonStruct._fields_]
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition only
    # _capi.SYMBOLS matches the header: every function the header declares is bound, and nothing else
    declared = set(re.findall(r"^(?:int|const char \*|void) ?\*?(ca3d_\w+)\(", header, flags=re.M))
    assert declared == set(bound), declared ^ set(bound)
    src = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "ca3d_ensemble.cpp")).read()
    assert re.search(r"^int ca3d_ensemble_canon\([^;{]*?\) CA3D_API_TRY\n\{\n", src, flags=re.S | re.M)
    mk = open(os.path.join(ROOT, "cellularautomatons3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*:=.*\bca_canon\.o\b", mk, flags=re.M)


def test_null_arguments_are_refused_without_a_device():
    lib = _capi.load()
    out = (_capi.CanonStruct * 2)()
    C.memset(out, 0x5A, C.sizeof(out))
    dig = (C.c_uint64 * 96)(*([7] * 96))
    ms = C.c_float(-1.0)
    assert lib.ca3d_ensemble_canon(None, 0, 2, out, dig, C.byref(ms)) == -1
    assert "NULL" in lib.ca3d_last_error().decode()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(dig) == [7] * 96 and ms.value == -1.0


def test_python_and_js_surfaces():
    for name in ("canon", "canon_gpu_ms", "canon_phases"):
        assert callable(getattr(Ensemble, name)), name
    for name in ("CANON_DTYPE", "canon", "symmetry_orientations", "is_chiral"):
        assert hasattr(host, name), name
    doc = Ensemble.canon_phases.__doc__
    assert "step" in doc and "EVERY universe" in doc and "ValueError" in doc
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    assert re.search(r"^\tcanon\(opts\)$", js, flags=re.M) and "ensembleCanon(" in js
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert '{"ensembleCanon", js_ensemble_canon}' in napi and "ca3d_ensemble_canon(" in napi
