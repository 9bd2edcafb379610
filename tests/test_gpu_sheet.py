"""The ensemble's contact sheet (`ca3d_ensemble_render_sheet`, kernel ca_render_sheet64) against its definition: tile k is, bit for
bit and in all three targets, the frame `ca3d_render` draws of universe first + k on an engine at 64^3 with "render_skip" 0 and
"render_indirect" 0. Every universe of a case has its own seed, so a tile drawn from the wrong universe cannot pass. The last test
compares whole sheets with the CPU oracle at tests/test_gpu_render.py's bar (RGB 2e-3, depth max(1e-4, one binary16 ulp), presentation
1/255 on >= 99.9 % of the pixels)."""
import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, host

pytestmark = pytest.mark.gpu

G = 64
INSIDE = ((0.1, 0.05, 0.2), (0.0, 1.0, 0.0), 0.4)  # a camera inside the volume


@pytest.fixture(scope="module")
def eng():
    """The engine that draws the frames the tiles are defined by."""
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    e.configure(G)
    e.set_option("render_skip", 0)
    e.set_option("render_indirect", 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def _frames(eng, states, u, w, h, spp):
    """[(presentation, light, depth, stats)] of `states`, one engine frame each."""
    out = []
    for s in states:
        eng.upload_state(s)
        out.append(eng.render(u, w, h, spp) + (eng.render_stats(),))
    return out


def _check_tiles(sheets, frames, w, h, columns):
    pres, light, depth = sheets
    H, W = host.sheet_shape(len(frames), w, h, columns)
    assert pres.shape == (H, W, 4) and light.shape == (H, W, 4) and depth.shape == (H, W, 2)
    for k, (p, l, d, _) in enumerate(frames):
        np.testing.assert_array_equal(host.sheet_tile(pres, k, w, h, columns), p, err_msg=f"presentation, tile {k}")
        np.testing.assert_array_equal(host.sheet_tile(light, k, w, h, columns).view(np.uint16), l.view(np.uint16), err_msg=f"light, tile {k}")
        np.testing.assert_array_equal(host.sheet_tile(depth, k, w, h, columns).view(np.uint16), d.view(np.uint16), err_msg=f"depth, tile {k}")


def _seed(ens, n, seed0, and_rounds=4):
    ens.configure(n)
    ens.seed_states(0, np.arange(seed0, seed0 + n), and_rounds)
    states = ens.read_state()
    assert len({s.tobytes() for s in states[:8]}) == min(n, 8)  # different universes
    return states


@pytest.mark.parametrize("spp", [1, 4])
def test_single_block(eng, ens, spp):
    states = _seed(ens, 1, 101)
    np.testing.assert_array_equal(states[0], host.seeded_state(G, 101, 4))
    u = host.uniform_block(16, 16, host.camera_matrix())
    sheets = ens.render_sheet(u, 16, 16, columns=1, spp=spp, light=True, depth=True)
    _check_tiles(sheets, _frames(eng, states, u, 16, 16, spp), 16, 16, 1)
    assert sheets[1][..., :3].max() > 0.05  # lit, not a black tile
    only = ens.render_sheet(u, 16, 16, columns=1, spp=spp)  # presentation alone: an array, not a tuple
    np.testing.assert_array_equal(only, sheets[0])


def test_empty_slot_and_sub_range(eng, ens):
    w, h, columns = 48, 32, 2
    states = _seed(ens, 3, 211)
    u = host.uniform_block(w, h, host.orbit_camera())
    frames = _frames(eng, states, u, w, h, 4)
    sheets = ens.render_sheet(u, w, h, columns=columns, spp=4, light=True, depth=True)
    assert sheets[0].shape == (2 * h, 2 * w, 4)
    _check_tiles(sheets, frames, w, h, columns)
    for s in sheets:  # the fourth slot: zero in every byte, also after a sheet that drew there
        assert not s[h:, w:].view(np.uint8).any()
    full = ens.render_sheet(u, w, h, columns=1, spp=4, light=True, depth=True)
    _check_tiles(full, frames, w, h, 1)
    again = ens.render_sheet(u, w, h, columns=columns, spp=4, light=True, depth=True)
    for s in again:
        assert not s[h:, w:].view(np.uint8).any()
    sub = ens.render_sheet(u, w, h, columns=columns, spp=4, first=1, count=2, light=True, depth=True)
    assert sub[0].shape == (h, 2 * w, 4)
    _check_tiles(sub, frames[1:], w, h, columns)
    assert ens.render_sheet(u, w, h, spp=4).shape == (2 * h, 2 * w, 4)  # columns=None: ceil(sqrt(3))


def test_more_universes_than_cus(eng, ens):
    w = h = 32
    states = _seed(ens, 300, 1000)
    u = host.uniform_block(w, h, host.camera_matrix())
    sheets = ens.render_sheet(u, w, h, columns=17, spp=1, first=5, count=290, light=True, depth=True)
    st = ens.sheet_stats()
    frames = _frames(eng, states[5:295], u, w, h, 1)
    _check_tiles(sheets, frames, w, h, 17)
    for s in sheets:  # 290 = 17 * 17 + 1: sixteen empty slots in the last row
        assert not s[17 * h:, w:].view(np.uint8).any()
    assert st.primary_rays == 290 * 1024
    for name in ("shadow_rays", "primary_cell_visits", "shadow_cell_visits"):
        want = sum(int(getattr(f[3], name)) for f in frames)
        assert int(getattr(st, name)) == want and want > 0, name
    assert st.gpu_ms > 0


def test_many_workgroups_per_universe(eng, ens):
    states = _seed(ens, 1, 307)
    u = host.uniform_block(256, 256, host.orbit_camera())
    sheets = ens.render_sheet(u, 256, 256, columns=1, spp=1, light=True, depth=True)
    _check_tiles(sheets, _frames(eng, states, u, 256, 256, 1), 256, 256, 1)


@pytest.mark.parametrize("w,h", [(1024, 16), (16, 1024)])
@pytest.mark.parametrize("columns", [1, 2])
def test_extreme_shapes(eng, ens, w, h, columns):
    states = _seed(ens, 2, 401)
    u = host.uniform_block(w, h, host.orbit_camera())
    sheets = ens.render_sheet(u, w, h, columns=columns, spp=1, light=True, depth=True)
    frames = _frames(eng, states, u, w, h, 1)
    _check_tiles(sheets, frames, w, h, columns)
    assert max(f[1][..., :3].max() for f in frames) > 0.05


def test_special_states(eng, ens):
    w = h = 32
    states = np.stack([np.zeros(8192, dtype=np.uint32), np.full(8192, 0xFFFFFFFF, dtype=np.uint32), host.seeded_state(G, 77, 7),
                       host.seeded_state(G, 78, 4, box=((40, 36, 44), (63, 63, 63)))])
    ens.configure(4)
    ens.upload_state(0, states)
    u = host.uniform_block(w, h, host.camera_matrix(*INSIDE))
    sheets = ens.render_sheet(u, w, h, columns=2, spp=4, light=True, depth=True)
    frames = _frames(eng, states, u, w, h, 4)
    _check_tiles(sheets, frames, w, h, 2)
    assert frames[0][3].shadow_rays == 0 and frames[0][2][..., 0].max() > 0  # the empty universe: the miss depth only
    assert max(f[1][..., :3].max() for f in frames) > 0.05
    # ... and seen from outside: the light gizmo before an empty universe
    u = host.uniform_block(w, h, host.camera_matrix())
    sheets = ens.render_sheet(u, w, h, columns=2, spp=4, light=True, depth=True)
    frames = _frames(eng, states, u, w, h, 4)
    _check_tiles(sheets, frames, w, h, 2)
    assert all(f[1][..., :3].max() > 0.05 for f in frames[1:])


def test_order_behind_steps(eng, ens):
    w = h = 32
    ens.configure(8)
    ens.set_rule_strings(0xFFFFFFFF, born="2,4", survive="1,3,5")
    ens.seed_states(0, np.arange(501, 509), 4)
    u = host.uniform_block(w, h, host.orbit_camera())
    ens.step(5)
    sheets = ens.render_sheet(u, w, h, columns=4, spp=1, light=True, depth=True)  # no synchronise in between
    states = ens.read_state()
    assert not np.array_equal(states[0], host.seeded_state(G, 501, 4))  # the steps ran
    _check_tiles(sheets, _frames(eng, states, u, w, h, 1), w, h, 4)
    again = ens.render_sheet(u, w, h, columns=4, spp=1, light=True, depth=True)
    for a, b in zip(sheets, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def _within_bar(pres, light, depth, cells, u, w, h, spp):
    """Per pixel: inside test_gpu_render.py's bar against the oracle's frame of `cells`."""
    olight, odepth, opres, _ = ol.render(cells, G, u, w, h, spp)
    od16 = odepth.astype(np.float16).astype(np.float32)
    ulp = np.maximum(np.spacing(od16.astype(np.float16)).astype(np.float32), 1e-4)
    ok_rgb = np.abs(light.astype(np.float32)[..., :3] - olight[..., :3]).max(-1) <= 2e-3
    ok_depth = np.abs(depth.astype(np.float32)[..., 0] - od16[..., 0]) <= ulp[..., 0]
    ok_pres = np.abs(pres.astype(np.float32) - np.rint(np.clip(opres, 0, 1) * 255.0)).max(-1) <= 1.0
    assert olight[..., :3].max() > 0.05  # lit
    return ok_rgb & ok_depth & ok_pres


@pytest.mark.parametrize("pose", ["default", "oblique"])
@pytest.mark.parametrize("spp", [1, 4])
def test_against_the_oracle(eng, ens, pose, spp):
    w, h, columns = 160, 96, 2
    states = _seed(ens, 4, 601)
    u = host.uniform_block(w, h, host.camera_matrix() if pose == "default" else host.orbit_camera())
    pres, light, depth = ens.render_sheet(u, w, h, columns=columns, spp=spp, light=True, depth=True)
    frames = _frames(eng, states, u, w, h, spp)
    ok_sheet = np.zeros(pres.shape[:2], dtype=bool)
    ok_engine = np.zeros(pres.shape[:2], dtype=bool)
    for k, s in enumerate(states):
        tiles = [host.sheet_tile(a, k, w, h, columns) for a in (pres, light, depth)]
        host.sheet_tile(ok_sheet, k, w, h, columns)[...] = _within_bar(*tiles, s, u, w, h, spp)
        host.sheet_tile(ok_engine, k, w, h, columns)[...] = _within_bar(*frames[k][:3], s, u, w, h, spp)
    assert ok_sheet.size == 61440
    print("fraction within the bar: sheet", ok_sheet.mean(), "engine", ok_engine.mean())
    assert ok_engine.mean() >= 0.999
    assert ok_sheet.mean() >= 0.999
    assert ok_sheet.mean() == ok_engine.mean()


def test_errors(ens):
    from cellularautomatons3d_amd import Ensemble

    u = host.uniform_block(32, 32, host.camera_matrix())

    def refused(e, code, text, **kw):
        args = dict(uniforms=u, tile_w=32, tile_h=32, columns=2, spp=1)
        args.update(kw)
        with pytest.raises(Ca3dError) as err:
            e.render_sheet(**args)
        assert err.value.code == code and text in str(err.value), str(err.value)

    fresh = Ensemble(0)
    try:
        refused(fresh, -2, "ca3d_ensemble_configure has not been called")
        with pytest.raises(Ca3dError) as err:
            fresh.sheet_stats()
        assert err.value.code == -2
    finally:
        fresh.close()
    ens.configure(6)  # no rules, and no rules ever set
    ens.seed_states(0, np.arange(701, 704), 4, count=None)
    refused(ens, -2, "universe 3", first=0, count=6)
    refused(ens, -2, "universe 3", first=2, count=2)
    refused(ens, -1, "universes", first=0, count=0)
    refused(ens, -1, "universes", first=4, count=3)
    refused(ens, -1, "universes", first=6, count=1)
    refused(ens, -1, "column", first=0, count=3, columns=0)
    for bad in (0, 8, 24, 1040, 2048):
        refused(ens, -1, "tile size", first=0, count=3, tile_w=bad)
        refused(ens, -1, "tile size", first=0, count=3, tile_h=bad)
    for bad in (0, 2, 3, 8):
        refused(ens, -1, "spp", first=0, count=3, spp=bad)
    refused(ens, -1, "2^26", first=0, count=3, tile_w=1024, tile_h=1024, columns=65)  # 66 560 x 1024 pixels
    with pytest.raises(ValueError):
        ens.render_sheet(u[:100], 32, 32, first=0, count=3)
    rc = ens._lib.ca3d_ensemble_render_sheet(ens._h, 0, 3, None, 32, 32, 2, 1, None, None, None)
    assert rc == -1 and "uniforms" in host_last_error(ens)
    # an ensemble whose rules were never set still draws; a call without outputs only enqueues, and the stats wait for it
    pres = ens.render_sheet(u, 32, 32, columns=2, first=0, count=3)
    assert pres[:32, :32, :3].max() > 0
    ens.upload_state(3, np.zeros((3, 8192), dtype=np.uint32))
    import ctypes as C
    assert ens._lib.ca3d_ensemble_render_sheet(ens._h, 0, 6, u.ctypes.data_as(C.POINTER(C.c_float)), 32, 32, 3, 4, None, None, None) == 0
    assert ens.sheet_stats().primary_rays == 6 * 1024 * 4


def host_last_error(ens):
    return ens._lib.ca3d_last_error().decode()
