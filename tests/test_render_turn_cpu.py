"""The render oracle and the turning helper (tests/render_turn.py) in the 24 orientations of the cube, on the CPU: before the oracle is
the reference for turned GPU frames (tests/test_gpu_render_turned.py) it is checked there itself — its cell walk against a brute-force
visibility search along all six axes, its whole frame against the frame of the same scene turned back — and the census at the end
shows what the turned set reaches that the suite's older poses do not: every sign octant and dominant axis of view and shadow rays."""
import numpy as np
import pytest

import oracle_lib as ol
import render_turn as rt
from cellularautomatons3d_amd import host


def test_the_24_rotations():
    assert len({q.tobytes() for q in rt.ROTATIONS}) == 24
    for q in rt.ROTATIONS:
        assert round(np.linalg.det(q)) == 1 and np.array_equal(q @ q.T, np.eye(3, dtype=np.int64))
        assert np.array_equal(host.orientation_matrix(host.orientation_from_matrix(q)), q)
    axes = [tuple(rt.ROTATIONS[k] @ np.array([0, 0, -1])) for k in rt.VIEW_AXIS_SIX]
    assert axes == [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] and 0 not in rt.VIEW_AXIS_SIX


@pytest.mark.parametrize("k", range(24))
def test_turn_cells_is_compose_at_64(k):
    """`host.compose` places a piece by its bounding box, turned by `orientation_from_matrix(Q)`: an independent implementation (index
    lists, not transposes). The turned box's low corner is where the rotation about the cube's centre takes it."""
    G = 64
    Q = rt.ROTATIONS[k]
    words = host.seeded_state(G, 1234, 4, box=((3, 9, 20), (40, 63, 51)))  # an off-centre box: a turn about the wrong centre shows
    zs, ys, xs = np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little").reshape(G, G, G))
    c = (xs, ys, zs)
    at = []
    for i in range(3):
        j = int(np.flatnonzero(Q[i])[0])
        at.append(int(c[j].min()) if Q[i, j] > 0 else G - 1 - int(c[j].max()))
    want, rec = host.compose([words], [(0, host.orientation_from_matrix(Q), at)])
    assert rec["clipped"] == 0 and rec["placed"] == xs.size > 1000
    np.testing.assert_array_equal(rt.turn_cells(words, G, Q), want)


def test_turns_of_an_asymmetric_shape_are_distinct_and_compose():
    G = 96  # not a power of two: three words a row
    shape = host.cells_to_words(G, [(5, 7, 11), (6, 7, 11), (7, 7, 11), (5, 8, 11), (5, 7, 12), (5, 7, 13), (5, 7, 14), (70, 1, 2)])
    turned = [rt.turn_cells(shape, G, q) for q in rt.ROTATIONS]
    assert len({t.tobytes() for t in turned}) == 24
    assert all(ol.popcount(t) == 8 for t in turned)
    np.testing.assert_array_equal(turned[0], shape)
    # a cell goes where the matrix takes its centre: (c + 1/2) / G - 1/2 -> Q @ that
    for q, t in zip(rt.ROTATIONS, turned):
        p = q @ (np.array([70, 1, 2]) * 2 + 1 - G)  # twice the centre's coordinate times G: integers
        x, y, z = (p + G - 1) // 2
        assert host.get_cell(G, t, int(x), int(y), int(z)) == 1
    # turning is a group action: turn by A, then by B = turn by B @ A
    for a, b in ((3, 17), (22, 5), (9, 9)):
        ba = rt.ROTATIONS[b] @ rt.ROTATIONS[a]
        np.testing.assert_array_equal(rt.turn_cells(turned[a], G, rt.ROTATIONS[b]), rt.turn_cells(shape, G, ba))
    with pytest.raises(ValueError):
        rt.turn_cells(shape, G, np.ones((3, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        rt.turn_cells(shape[:-1], G, rt.ROTATIONS[1])


def test_turn_view_and_light():
    vm = host.orbit_camera()
    for q in rt.ROTATIONS:
        m = rt.turn_view(vm, q).reshape(4, 4).T
        m0 = vm.reshape(4, 4).T
        np.testing.assert_array_equal(m[:3, :3], (q @ m0[:3, :3].astype(np.float64)).astype(np.float32))
        np.testing.assert_array_equal(m[:3, 3], (q @ m0[:3, 3].astype(np.float64)).astype(np.float32))
        np.testing.assert_array_equal(m[3], (0, 0, 0, 1))
        assert abs(np.linalg.det(m[:3, :3].astype(np.float64)) - 1) < 1e-6  # a camera the UI can produce, not a mirror image
        l = rt.turn_light((0.721, 1.0, 1.0, 5.0), q)
        assert l[3] == 5.0 and np.array_equal(np.float32(l[:3]), (q @ np.array([0.721, 1.0, 1.0])).astype(np.float32))


@pytest.mark.parametrize("k", rt.VIEW_AXIS_SIX)
def test_walk_equals_bruteforce_visibility_along_every_axis(k):
    """test_render_oracle.py::test_walk_equals_bruteforce_visibility looks down -z twice; here the view axis is +x, -x, +y, -y, +z and
    -z, each tilted by 0.25 rad, so that the oracle's walk steps in every direction: nearest visible cube among ALL live cells against
    the depth of `ol.render`, every third pixel, no mismatch."""
    G, W, H = 32, 64, 36
    cells, u = rt.turned_scene(host.random_fill(host.words_per_buffer(G), seed=3, and_rounds=4), G, rt.ROTATIONS[k], W, H,
                               host.orbit_camera(1.0, (1.0, 1.0, 0.0), 0.25))
    _, depth, _, _ = ol.render(cells, G, u, W, H)
    checked = hits = bad = 0
    for py in range(0, H, 3):
        for px in range(0, W, 3):
            d, cell = ol.primary_bruteforce(cells, G, u, W, H, px, py)
            checked += 1
            if d < 0:
                assert depth[py, px, 0] == 0.0
            else:
                hits += cell >= 0
                bad += abs(depth[py, px, 0] - d) > 1e-5
    assert checked == 264 and hits > 60 and bad == 0, (checked, hits, bad)


def _contract(a, b):
    """Per pixel: two oracle frames (light, depth, presentation) within the suite's contract of each other — RGB 2e-3, depth 1e-4 (both
    are float32; no binary16 target in between), presentation one step of 255."""
    ok_rgb = np.abs(a[0][..., :3] - b[0][..., :3]).max(-1) <= 2e-3
    ok_depth = np.abs(a[1][..., 0] - b[1][..., 0]) <= 1e-4
    ok_pres = np.abs(np.rint(np.clip(a[2], 0, 1) * 255.0) - np.rint(np.clip(b[2], 0, 1) * 255.0)).max(-1) <= 1.0
    return ok_rgb & ok_depth & ok_pres, ok_depth


@pytest.mark.parametrize("W,H,spp", [(320, 180, 1), (160, 90, 4)])
def test_oracle_frame_turns_with_the_scene(W, H, spp):
    """Cells, camera and light turned together by each of the 24 rotations: the oracle draws the untouched frame again, within the
    suite's own contract on >= 99.9 % of the pixels (the cap is the contract's; measured: >= 0.99984 at 320 x 180, >= 0.99951 at
    160 x 90 with four samples), with the same depth on EVERY pixel and the same number of shadow rays. With a material colour: the
    default black one colours a cell by its x and y index, which a turn changes (about 10 % of the pixels; the shader, not an error).

    What the pixels outside are (9 of 57 600 in 12 of the 24 rotations, none in the other 12; 7 of 14 400 at four samples): not the
    light gizmo and not silhouettes. `orbit_camera()` turns about the axis (1, 1, 0), so the camera sits in the plane x + y = 0 and so
    does every ray of the image diagonal px - py = (W - H) / 2 through the centre. That plane is a mirror plane of the cell grid: it
    cuts the cells with cx + cy = G - 1 through their vertical edges, and a ray in it that hits such a cell first hits it exactly ON
    the edge between its x face and its y face: |p.x - origin.x| == |p.y - origin.y| to the last bit. face_normal (the reference's
    :227-254) breaks that tie in the order x, y, z; the twelve rotations that swap the order of those two axes pick the other face,
    one of the two faces away from the light and the pixel is black in one frame and lit in the other — by up to 1.0. Both answers are
    the reference's. Asserted below: every pixel outside the contract lies on that diagonal and has the untouched depth."""
    G = 64
    cells = host.random_fill(host.words_per_buffer(G), seed=3, and_rounds=4)
    kw = dict(materialColor=(0.8, 0.2, 0.1))
    base = ol.render(cells, G, host.uniform_block(W, H, host.orbit_camera(), **kw), W, H, spp)
    assert base[0][..., :3].max() > 0.05
    py, px = np.mgrid[0:H, 0:W]
    diagonal = px - py == (W - H) // 2
    worst, differing = 1.0, 0
    for k, Q in enumerate(rt.ROTATIONS):
        c, u = rt.turned_scene(cells, G, Q, W, H, host.orbit_camera(), **kw)
        got = ol.render(c, G, u, W, H, spp)
        ok, ok_depth = _contract(got, base)
        assert ok.mean() >= 0.999, (k, ok.mean())
        assert ok_depth.all(), (k, ok_depth.mean())
        assert got[3] == base[3], (k, got[3], base[3])
        assert diagonal[~ok].all(), (k, np.argwhere(~ok & ~diagonal)[:5])
        assert k or ok.all()  # the identity
        worst = min(worst, ok.mean())
        differing += bool((~ok).any())
    print(f"turned oracle frames {W} x {H} @ {spp}: worst fraction within the contract {worst:.5f}; {differing} of 24 rotations differ anywhere")


OLD_POSES = (host.camera_matrix(), host.orbit_camera(), host.orbit_camera(1.2, (1.0, 0.3, 0.0), 0.8),
             host.camera_matrix((0.2, 0.6, 0.4), (1.0, 0.0, 0.0), -0.9))  # test_random_volume, test_small_live_box_frame, test_volume_rectangle_cases


def test_census_all_24_bins_against_12_and_3():
    """Why the turned tests exist, as a figure: ray directions binned by sign octant and dominant axis, 24 bins. Over the 24 rotations
    of one pose every bin holds at least 1 % of the hit pixels, for view rays and for the rays from hit point to light (measured: 4.16 %
    to 4.17 % each — the rotations act simply transitively on the bins). The four poses the renderer's tests used before fill 12 bins
    with view rays — none ascends in z — and 3 with shadow rays, all in the (+, +, +) octant."""
    G, W, H = 64, 320, 180
    cells = host.random_fill(host.words_per_buffer(G), seed=3, and_rounds=4)
    primary = np.zeros(24, dtype=np.int64)
    shadow = np.zeros(24, dtype=np.int64)
    for Q in rt.ROTATIONS:
        c, u = rt.turned_scene(cells, G, Q, W, H, host.orbit_camera())
        _, depth, _, n_shadow = ol.render(c, G, u, W, H)
        p, s = rt.ray_census(u, None, None, depth, W, H)
        assert p.sum() == s.sum() == n_shadow > 5000  # the pixels that hit a cell are the ones the oracle cast a shadow ray for
        primary += p
        shadow += s
    assert (primary >= 0.01 * primary.sum()).all(), dict(zip(rt.bin_names(), primary))
    assert (shadow >= 0.01 * shadow.sum()).all(), dict(zip(rt.bin_names(), shadow))

    G, W, H = 32, 64, 36
    cells = host.random_fill(host.words_per_buffer(G), seed=3, and_rounds=4)
    old_primary = np.zeros(24, dtype=np.int64)
    old_shadow = np.zeros(24, dtype=np.int64)
    for vm in OLD_POSES:
        u = host.uniform_block(W, H, vm)
        _, depth, _, n_shadow = ol.render(cells, G, u, W, H)
        p, s = rt.ray_census(u, vm, host.RENDER_DEFAULTS["light"], depth, W, H)
        assert p.sum() == s.sum() == n_shadow > 100
        old_primary += p
        old_shadow += s
    names = rt.bin_names()
    assert (old_primary > 0).sum() == 12 and not any(c for n, c in zip(names, old_primary) if n[2] == "+"), dict(zip(names, old_primary))
    assert [n for n, c in zip(names, old_shadow) if c] == ["+++ x", "+++ y", "+++ z"], dict(zip(names, old_shadow))
    print(f"bins filled: turned set {(primary > 0).sum()} / {(shadow > 0).sum()} of 24 (view / shadow rays), older poses "
          f"{(old_primary > 0).sum()} / {(old_shadow > 0).sum()}")
