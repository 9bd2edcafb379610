"""The torus isolate's host side (`ca3d_ensemble_isolate_connected` with CA3D_CONNECT_TORUS, include/ca3d.h): `host.isolate(...,
connectivity="torus")` of a state whose objects lie across the faces equals `host.isolate(..., "closed")` of the same state rolled
clear of the faces, up to the known shift; ORIGIN's digest is the torus census record's; `connectivity="closed"` is the isolate as it
was. No GPU."""
import numpy as np
import pytest

import census_cases as cc
import objects_torus_cases as tc
from cellularautomatons3d_amd import host

G, W = 64, 8192
PLACEMENTS = ("keep", "centre", "origin")


@pytest.mark.parametrize("d", tc.ROLLS + ((40, 50, 60),))
@pytest.mark.parametrize("name", tc.CLEAR)
def test_torus_isolate_is_the_closed_isolate_of_the_unrolled_state(name, d):
    """`name` keeps clear of the faces; rolled by d its objects cross seams. The torus isolate of the rolled state's cell c + d is the
    closed isolate of cell c: the same words under CENTRE and ORIGIN with the shift smaller by d modulo 64, the words rolled by d
    under KEEP."""
    base, moved = tc.state(name), tc.state(name, d)
    comps, n, rest = tc.reference((name, "closed"), base, 64, "closed")
    assert rest == 0 and n >= 1
    torus = tc.reference((name, d), moved, 64)
    assert torus[1] == n and torus[2] == 0
    for c in comps[:n]:
        cell = int(c["first_cell"])
        x, y, z = cell & 63, (cell >> 6) & 63, cell >> 12
        there = (x + d[0]) % G + G * ((y + d[1]) % G) + G * G * ((z + d[2]) % G)
        for placement in PLACEMENTS:
            want_words, want_pop, want_shift = host.isolate(base, cell, placement, "closed")
            words, pop, shift = host.isolate(moved, there, placement, "torus")
            assert words.dtype == np.uint32 and words.shape == (W,) and pop == want_pop == int(c["population"])
            if placement == "keep":
                assert shift == (0, 0, 0) == want_shift
                np.testing.assert_array_equal(words, tc.rolled(want_words, d))
            else:
                np.testing.assert_array_equal(words, want_words)  # the object in one piece, where the closed isolate puts it
                assert all(-63 <= s <= 31 and (s + dd - w) % G == 0 for s, dd, w in zip(shift, d, want_shift)), (shift, want_shift)
            if placement == "origin":
                lowest = int(tc.cells_list(host.isolate(moved, there, "keep", "torus")[0])[0])  # the object's first cell in the rolled state
                rec = [r for r in torus[0][:n] if int(r["first_cell"]) == lowest]
                assert len(rec) == 1 and int(rec[0]["digest"]) == host.state_summary(G, words)["digest"] == int(c["digest"])
                assert shift == tuple(-v for v in host.unpack_box(rec[0]["box_min"]))


def test_any_cell_selects_the_object_and_a_dead_cell_nothing():
    state = tc.state("shapes", (63, 1, 33))
    comps, n, _ = tc.reference(("shapes", (63, 1, 33)), state, 64)
    assert n == 3
    for c in comps[:n]:
        whole = host.isolate(state, int(c["first_cell"]), "keep", "torus")[0]
        cells = tc.cells_list(whole)
        assert cells.size == 12 and int(cells[0]) == int(c["first_cell"])
        for cell in (int(cells[5]), int(cells[-1])):
            for placement in PLACEMENTS:
                a, b = host.isolate(state, cell, placement, "torus"), host.isolate(state, int(c["first_cell"]), placement, "torus")
                np.testing.assert_array_equal(a[0], b[0])
                assert a[1:] == b[1:]
    dead = next(i for i in range(G ** 3) if i not in set(tc.cells_list(state).tolist()))
    words, pop, shift = host.isolate(state, dead, "centre", "torus")
    assert not words.any() and (pop, shift) == (0, (0, 0, 0))


def test_a_ring_is_not_moved_along_its_axis():
    for axis in range(3):
        state = host.cells_to_words(G, tc.rod(axis))
        cell = int(tc.cells_list(state)[17])
        for placement in PLACEMENTS:
            words, pop, shift = host.isolate(state, cell, placement, "torus")
            assert pop == 64 and shift[axis] == 0
            want = [0, 0, 0] if placement == "keep" else [-21, -38, -10] if placement == "origin" else [31 - 21, 31 - 38, 31 - 10]
            want[axis] = 0
            assert list(shift) == want
            np.testing.assert_array_equal(words, tc.rolled(state, shift))


def test_closed_is_the_isolate_as_it_was():
    for name in ("shapes", "corners", "shell_core"):
        state = cc.state(name)
        for c in cc.reference(name, 64)[0][:cc.reference(name, 64)[1]]:
            for placement in PLACEMENTS:
                old = host.isolate(state, int(c["first_cell"]), placement)
                new = host.isolate(state, int(c["first_cell"]), placement, connectivity="closed")
                assert old[0].tobytes() == new[0].tobytes() and old[1:] == new[1:]
    with pytest.raises(ValueError):
        host.isolate(cc.state("shapes"), 0, "keep", "open")
