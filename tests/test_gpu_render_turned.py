"""The renderer with scene, camera and light turned all 24 ways (tests/render_turn.py): the same pictures from code that sees every
sign and every dominant axis of a view ray and of a shadow ray. Every camera of the older renderer tests looks down -z and every light
sits at +z: their view rays fill 12 of the 24 (sign octant, dominant axis) bins, none ascending in z, their shadow rays 3
(tests/test_render_turn_cpu.py counts them). The sign-dependent code — the `neg` and `edge` masks of the packed-position walker
(render_stream.hip walk_advance_p), the sx / sy / sz selects of render.hip, render_device.inc and render_stream.hip, volume_rect's corner
projection, the sheet kernel's walk over its LDS copy, a walk ALONG the bit-packed x axis — runs here in all of them.

Every case goes through tests/test_gpu_render.py's own check (render_compare.compare): plain, scheduled, stream and stream-with-check
forms bit for bit, the oracle within the contract (RGB 2e-3, depth max(1e-4, one binary16 ulp), presentation 1/255 on >= 99.9 % of the
pixels), shadow-ray count, stats. The oracle itself is checked in the same orientations on the CPU (tests/test_render_turn_cpu.py).

Measured on an MI355X: the file's 217 tests take 10.9 s (the slowest, the 256^3 live box, 0.7 s a rotation); every GPU frame of every
case had ALL its pixels within the contract, so no kernel or oracle change came of it."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as ol
import render_turn as rt
from cellularautomatons3d_amd import host
from gpu_common import rules, set_rules
from render_compare import compare
from test_gpu_render import _moving_camera
from test_gpu_sheet import _check_tiles, _frames, _within_bar

pytestmark = pytest.mark.gpu

ALL = range(24)


@pytest.fixture(scope=lambda fixture_name, config: os.environ.get("CA3D_TEST_ENGINE_SCOPE", "module"))
def eng():
    # as in test_gpu_render.py: one engine per file by default, CA3D_TEST_ENGINE_SCOPE=function gives every test a fresh one
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


#: case -> rotation index -> (view-ray bins, shadow-ray bins) of the oracle frame the case was compared with
_CENSUS = {}


@functools.lru_cache(maxsize=None)
def _fill(G, seed, rounds):
    cells = host.random_fill(host.words_per_buffer(G), seed=seed, and_rounds=rounds)
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def _live_box():
    """256^3, random cells of density 1/8 inside x 8..40, y 150..200, z 200..250 and nothing elsewhere: the rotations carry the box into
    every corner of the volume."""
    cells = host.seeded_state(256, 77, 2, box=((8, 150, 200), (40, 200, 250)))
    cells.setflags(write=False)
    return cells


def _turned(eng, case, k, cells, G, W, H, spp, vm, min_ok=0.999, **overrides):
    c, u = rt.turned_scene(cells, G, rt.ROTATIONS[k], W, H, vm, **overrides)
    oracle = {}
    frac = compare(eng, c, G, u, W, H, spp, min_ok=min_ok, oracle=oracle)
    _CENSUS.setdefault(case, {})[k] = rt.ray_census(u, None, None, oracle["depth"], W, H, spp)
    print(f"{case} rotation {k}: {frac:.5f} of the pixels within the contract")
    return c, u


@pytest.mark.parametrize("k", ALL)
def test_dense_default_material(eng, k):
    """Position colouring (materialColor black) is the UI's default: the case a user sees."""
    _turned(eng, "dense", k, _fill(64, 3, 4), 64, 320, 180, 1, host.orbit_camera())


@pytest.mark.parametrize("k", ALL)
def test_dense_four_samples_material_overlay(eng, k):
    _turned(eng, "dense4", k, _fill(64, 3, 4), 64, 160, 90, 4, host.orbit_camera(), materialColor=(0.8, 0.2, 0.1), showDepthOverlay=1,
            roughness=0.6, cellSize=0.6)


@pytest.mark.parametrize("k", ALL)
def test_grid_96(eng, k):
    """Not a power of two: bricks are indexed by multiply-add, not shifts."""
    _turned(eng, "g96", k, _fill(96, 7, 4), 96, 160, 90, 1, host.orbit_camera())
    assert eng.info().grid_size == 96


@pytest.mark.parametrize("k", ALL)
def test_scattered_sparse(eng, k):
    """Density 2^-13, live cells everywhere: long walks that leave the grid through every face — the walker's `edge` test."""
    _turned(eng, "sparse", k, _fill(128, 17 + 128, 12), 128, 160, 90, 1, host.orbit_camera())


@pytest.mark.parametrize("k", ALL)
def test_off_centre_live_box(eng, k):
    """The occupancy skip, the live box's screen rectangle, the pixels filled without a trace and ca_render_packed_spread, with the
    box in every corner. (Not the evolved start-up seed: it is centred and nearly symmetric, so turning it tests little.)"""
    _, u = _turned(eng, "box", k, _live_box(), 256, 160, 90, 1, host.orbit_camera())
    v_skip = eng.render_stats().primary_cell_visits
    eng.set_option("render_skip", 0)
    try:
        eng.render(u, 160, 90, 1)
        v_plain = eng.render_stats().primary_cell_visits
    finally:
        eng.set_option("render_skip", 1)
    assert v_skip * 3 < v_plain, (v_skip, v_plain)  # the skip is at work (test_empty_space_skipping_on_a_sparse_volume's bound)


@pytest.mark.parametrize("k", ALL)
def test_camera_inside(eng, k):
    _turned(eng, "inside", k, _fill(64, 5, 5), 64, 160, 90, 1, host.camera_matrix((0.1, -0.05, 0.2), (0.0, 1.0, 0.0), 0.4), min_ok=0.995)


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("k", ALL)
def test_sheet_tile(eng, ens, k, spp):
    """ca_render_sheet64 walks its own LDS copy of the universe: one universe, one 64 x 64 tile, against `ca3d_render` of the same turned
    universe bit for bit in all three targets (test_gpu_sheet.py's definition: "render_skip" 0, "render_indirect" 0) and against the
    oracle within the contract."""
    w = h = 64
    c, u = rt.turned_scene(_fill(64, 3, 4), 64, rt.ROTATIONS[k], w, h, host.orbit_camera())
    ens.configure(1)
    ens.upload_state(0, c[None, :])
    sheets = ens.render_sheet(u, w, h, columns=1, spp=spp, light=True, depth=True)
    eng.configure(64)
    set_rules(eng, rules("default"))
    eng.set_option("render_skip", 0)
    eng.set_option("render_indirect", 0)
    try:
        frames = _frames(eng, [c], u, w, h, spp)
    finally:
        eng.set_option("render_skip", 1)
    _check_tiles(sheets, frames, w, h, 1)
    ok = _within_bar(*sheets, c, u, w, h, spp)
    print(f"sheet rotation {k} @ {spp}: {ok.mean():.5f} of the pixels within the contract")
    assert ok.mean() >= 0.999, ok.mean()


# ---- six rotations: the view axis -z taken to +x, -x, +y, -y, +z, -z ------------------------------------------------------------------

SIX = rt.VIEW_AXIS_SIX


@pytest.mark.parametrize("k", SIX)
def test_literal_frame_under_a_moving_camera(eng, k):
    """render_mode 1 against `ol.render_frame`: four lock-step frames under test_gpu_render.py's moving camera (its orbit), each side on
    its own history, both forms of the frame bit for bit; that test's tolerance (2e-3 RGB and depth on >= 99.9 % of the pixels)."""
    G, W, H = 32, 160, 90
    Q = rt.ROTATIONS[k]
    cells = rt.turn_cells(_fill(G, 11, 4), G, Q)
    light = rt.turn_light(host.RENDER_DEFAULTS["light"], Q)
    poses = [rt.turn_view(_moving_camera(f), Q) for f in range(4)]
    blocks = [host.uniform_block(W, H, vm, elapsed_time=0.1 + 0.137 * f, prev_view_mat=poses[f - 1] if f else None, light=light)
              for f, vm in enumerate(poses)]
    eng.configure(G)
    set_rules(eng, rules("default"))
    eng.upload_state(cells)
    eng.set_render_mode(True)
    try:
        frames = {}
        for bricks in (0, 1):
            eng.set_option("render_frame_bricks", bricks)
            eng.render(blocks[0], W, H, 1)
            eng.reset_render_history()
            frames[bricks] = [eng.render(u, W, H, 1) for u in blocks]
        for a, b in zip(frames[0], frames[1]):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
        pl = pd = None
        for f, u in enumerate(blocks):
            ol_light, ol_depth, _ = ol.render_frame(cells, G, u, W, H, pl, pd)
            pl, pd = ol_light.astype(np.float16).astype(np.float32), ol_depth.astype(np.float16).astype(np.float32)
            _, light_f, depth_f = frames[1][f]
            ok = (np.abs(light_f.astype(np.float32)[..., :3] - pl[..., :3]).max(-1) <= 2e-3) & \
                 (np.abs(depth_f.astype(np.float32)[..., 0] - pd[..., 0]) <= 2e-3)
            assert ok.mean() >= 0.999, (f, ok.mean())
        assert pl[..., :3].max() > 0.05
    finally:
        eng.set_option("render_frame_bricks", 1)
        eng.set_render_mode(False)


@pytest.mark.parametrize("k", SIX)
def test_legacy_renderer_over_the_unpacked_volume(eng, k):
    """One u32 per cell, the legacy shading: test_gpu_render.py's comparison, and the same geometry as the packed renderer sees."""
    from cellularautomatons3d_amd import LAYOUT_UNPACKED

    G, W, H = 64, 320, 180
    packed, u = rt.turned_scene(_fill(G, 3, 4), G, rt.ROTATIONS[k], W, H, host.orbit_camera(), light=(0.721, 1.0, 1.0, 1.5))
    cells = np.unpackbits(packed.view(np.uint8), bitorder="little").astype(np.uint32)
    eng.configure(G, LAYOUT_UNPACKED)
    try:
        set_rules(eng, rules("default"))
        eng.upload_state(cells)
        pres, light, depth = eng.render(u, W, H, 1)
    finally:
        eng.configure(G)
    olight, odepth, opres, _ = ol.render(cells, G, u, W, H, 1, legacy=True)
    ok = (np.abs(light.astype(np.float32)[..., :3] - olight[..., :3]).max(-1) <= 2e-3) & \
         (np.abs(depth.astype(np.float32)[..., 0] - odepth[..., 0].astype(np.float16).astype(np.float32)) <= 2e-3) & \
         (np.abs(pres.astype(np.float32) - np.rint(np.clip(opres, 0, 1) * 255.0)).max(-1) <= 1)
    assert ok.mean() >= 0.999, ok.mean()
    assert olight[..., :3].max() > 0.05
    set_rules(eng, rules("default"))
    eng.upload_state(packed)
    _, _, d2 = eng.render(u, W, H, 1)
    assert (np.abs(d2.astype(np.float32)[..., 0] - depth.astype(np.float32)[..., 0]) <= 2e-3).mean() >= 0.999


@pytest.mark.parametrize("k", SIX)
def test_indirect_lighting_mode(eng, k):
    """"render_indirect": the neighbour layer is chosen by the sign of the face normal, one table row per sign and axis."""
    G, W, H = 64, 320, 180
    cells, u = rt.turned_scene(_fill(G, 9, 2), G, rt.ROTATIONS[k], W, H, host.orbit_camera())
    eng.configure(G)
    set_rules(eng, rules("default"))
    eng.upload_state(cells)
    _, direct, _ = eng.render(u, W, H, 1)
    eng.set_option("render_indirect", 1)
    try:
        for spp in (1, 4):
            pres, light, depth = eng.render(u, W, H, spp)
            olight, odepth, opres, _ = ol.render(cells, G, u, W, H, spp, indirect=True)
            ok = np.abs(light.astype(np.float32)[..., :3] - olight[..., :3]).max(-1) <= 2e-3
            ok &= np.abs(pres.astype(np.float32) - np.rint(np.clip(opres, 0, 1) * 255.0)).max(-1) <= 1.0
            assert ok.mean() >= 0.999, (spp, ok.mean())
            if spp == 1:
                changed = np.abs(light.astype(np.float32)[..., :3] - direct.astype(np.float32)[..., :3]).max(-1) > 4e-3
                assert changed.mean() > 0.005, changed.mean()
    finally:
        eng.set_option("render_indirect", 0)


@pytest.fixture(scope="module")
def group():
    from cellularautomatons3d_amd import EngineGroup

    with EngineGroup([0] * 4) as g:
        g.configure(256, 4)
        r = rules("default")
        g.set_rules(r.main, r.edges, r.corners, r.survive, r.born)
        yield g


@pytest.mark.parametrize("k", SIX)
def test_engine_group_renders_the_frame_in_bands(eng, group, k):
    """ca3d_group_render, four slabs: each rank renders its band of image rows — bit-identical to one engine's frame (test_gpu_slab.py's
    comparison and sizes)."""
    G, W, H = 256, 640, 360
    cells, u = rt.turned_scene(_fill(G, 779, 4), G, rt.ROTATIONS[k], W, H, host.orbit_camera())
    group.upload_state(cells)
    eng.configure(G)
    set_rules(eng, rules("default"))
    eng.upload_state(cells)
    a = group.render(u, W, H, 4)
    b = eng.render(u, W, H, 4)
    for x, y, what in zip(a, b, ("presentation", "light", "depth")):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)
    assert a[0][..., :3].any()


def test_census_of_what_was_rendered(eng):
    """Over the 24 rotations of a case, every one of the 24 (octant, dominant axis) bins holds at least 1 % of the pixels that hit a
    cell, for view rays and for shadow rays: counted on the oracle frames the cases above were compared with (the dense case is
    rendered here if this test runs alone)."""
    for k in ALL:
        if k not in _CENSUS.get("dense", {}):
            _turned(eng, "dense", k, _fill(64, 3, 4), 64, 320, 180, 1, host.orbit_camera())
    names = rt.bin_names()
    for case, by_k in _CENSUS.items():
        if len(by_k) < 24:
            continue  # a case only partly selected on the command line
        primary = sum(p for p, _ in by_k.values())
        shadow = sum(s for _, s in by_k.values())
        assert primary.sum() >= 24 * 20, (case, primary.sum())  # the case shows cells at all
        assert (primary >= 0.01 * primary.sum()).all(), (case, dict(zip(names, primary)))
        assert (shadow >= 0.01 * shadow.sum()).all(), (case, dict(zip(names, shadow)))
        print(f"{case}: {primary.sum()} hit pixels over 24 rotations, smallest bin {primary.min()} view rays / {shadow.min()} shadow rays")
