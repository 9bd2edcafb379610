"""The renderer's parity check, shared by tests/test_gpu_render.py and tests/test_gpu_render_turned.py — TEST INFRASTRUCTURE.

Tolerance (SURVEY 8(a) row R-par, the contract stated in tests/test_gpu_render.py): on >= 99.9 % of pixels linear-light RGB abs error
<= 2e-3, depth abs error <= max(1e-4, one binary16 ulp of the stored value), presentation <= 1/255."""
import numpy as np

import oracle_lib as ol
from gpu_common import rules, set_rules


def compare(eng, cells, G, u, W, H, spp, rows=None, min_ok=0.999, oracle=None):
    """`oracle`, a dict, receives the oracle's frame ("light", "depth", "pres", "shadow_rays") for a caller that wants to look at it;
    nothing of what is asserted depends on it."""
    eng.configure(G)
    set_rules(eng, rules("default"))
    eng.upload_state(cells)
    # the plain kernel (one pixel per lane, samples in order), the in-wave scheduled one and the ray-stream passes (the default; also with
    # every decision of their interval filter checked against the slab test: a contradiction fails the call) must agree bit for bit
    eng.set_option("render_sched", 0)
    pres0, light0, depth0 = eng.render(u, W, H, spp)
    st0 = eng.render_stats()
    eng.set_option("render_sched", 1)
    for stream, check in ((0, 0), (1, 1), (1, 0)):
        eng.set_option("render_stream", stream)
        eng.set_option("render_stream_check", check)
        pres, light, depth = eng.render(u, W, H, spp)
        st1 = eng.render_stats()
        np.testing.assert_array_equal(pres, pres0)
        np.testing.assert_array_equal(light.view(np.uint16), light0.view(np.uint16))
        np.testing.assert_array_equal(depth.view(np.uint16), depth0.view(np.uint16))
        assert (st0.shadow_rays, st0.primary_cell_visits, st0.shadow_cell_visits) == (st1.shadow_rays, st1.primary_cell_visits, st1.shadow_cell_visits)
    olight, odepth, opres, oshadow = ol.render(cells, G, u, W, H, spp, rows)
    if oracle is not None:
        oracle.update(light=olight, depth=odepth, pres=opres, shadow_rays=oshadow)
    y0, y1 = rows if rows else (0, H)
    sl = slice(y0, y1)
    l = light[sl].astype(np.float32)
    d = depth[sl].astype(np.float32)
    od16 = odepth[sl].astype(np.float16).astype(np.float32)
    ulp = np.maximum(np.spacing(od16.astype(np.float16)).astype(np.float32), 1e-4)
    ok_rgb = np.abs(l[..., :3] - olight[sl][..., :3]).max(-1) <= 2e-3
    ok_depth = np.abs(d[..., 0] - od16[..., 0]) <= ulp[..., 0]
    want8 = np.rint(np.clip(opres[sl], 0, 1) * 255.0)
    ok_pres = np.abs(pres[sl].astype(np.float32) - want8).max(-1) <= 1.0
    frac = (ok_rgb & ok_depth & ok_pres).mean()
    assert frac >= min_ok, (frac, ok_rgb.mean(), ok_depth.mean(), ok_pres.mean())
    assert (light[sl][..., 3] == 1.0).all() and (depth[sl][..., 1] == 1.0).all()
    assert olight[sl][..., :3].max() > 0.05  # the scene is not empty
    if rows is None:
        st = eng.render_stats()
        assert st.primary_rays == W * H * spp
        assert abs(int(st.shadow_rays) - oshadow) <= max(4, int(0.001 * oshadow))
    return frac
