"""The lone-slab harness (tests/slab_lone.py) checked on the CPU: a stand-in with the engine's slab methods, whose sub-steps are the
oracle's plane-range step on two ping-pong buffers over `slab.batch_ranges`, is driven through every geometry the GPU tests use
(tests/test_gpu_slab_ranges.py) at G = 96. What the harness expects of an engine therefore follows from the reference semantics alone:
a failure on the GPU is the kernel's or the launcher's."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
import slab_lone as sl
from cellularautomatons3d_amd import LAYOUT_PACKED32, LAYOUT_UNPACKED, SLAB_PHASE_EDGES, SLAB_PHASE_INTERIOR, slab
from cellularautomatons3d_amd._capi import SLAB_OWNED, SLAB_RECV_HIGH, SLAB_RECV_LOW, SLAB_SEND_HIGH, SLAB_SEND_LOW
from gpu_common import rules


class OracleEngine:
    """One rank's slab with the `Engine` methods the harness calls, computed by the oracle (as tests/slab_oracle_backend.py does)."""

    def configure_slab(self, G, z0, nz, K, layout=LAYOUT_PACKED32):
        if nz == 0 or z0 + nz > G or K == 0 or K > nz:
            raise ValueError("bad slab")
        self.G, self.z0, self.nz, self.K, self.layout = G, z0, nz, K, layout
        self.pw = sl.plane_words(G, layout)
        self.L = nz + 2 * K
        self.bufs = [np.zeros(self.L * self.pw, dtype=np.uint32) for _ in range(2)]
        self.cur, self.pending, self.steps = 0, 0, 0

    def set_option(self, name, value):
        pass  # kernel forms: nothing to choose here

    def set_rules(self, main, edges, corners, survive, born):
        self.rules = ol.Rules(main, edges, corners, survive, born)

    def upload_state(self, owned):
        assert owned.size == self.nz * self.pw
        for b in self.bufs:
            b[:] = 0
            b[self.K * self.pw:(self.K + self.nz) * self.pw] = owned
        self.cur, self.pending, self.steps = 0, 0, 0

    def read_state(self):
        return self.bufs[self.cur][self.K * self.pw:(self.K + self.nz) * self.pw].copy()

    def synchronize(self):
        pass

    def slab_region_tensor(self, region):
        K, nz, pw = self.K, self.nz, self.pw
        first, count = {SLAB_SEND_LOW: (K, K), SLAB_SEND_HIGH: (nz, K), SLAB_RECV_LOW: (0, K), SLAB_RECV_HIGH: (K + nz, K), SLAB_OWNED: (K, nz)}[region]
        buf = self.bufs[(self.cur + self.pending) & 1]  # after an edge phase: the buffer its results are in
        return torch.from_numpy(buf[first * pw:(first + count) * pw].view(np.int32))

    def _step_range(self, src, dst, lo, hi):
        if hi <= lo:
            return
        if self.layout == LAYOUT_PACKED32:
            out = ol.packed_step_planes(self.G, src, self.z0 - self.K, lo, hi, self.rules)
        else:
            out = ol.unpacked_step_planes(self.G, src, lo, hi, self.rules.main, self.rules.survive, self.rules.born)
        dst[lo * self.pw:hi * self.pw] = out[lo * self.pw:hi * self.pw]

    def _run(self, n, zones):
        dead_bottom = self.layout == LAYOUT_PACKED32 and self.z0 == 0
        for zone in zones:
            for s in range(1, n + 1):
                lo, hi = slab.batch_ranges(self.nz, self.K, n, s, dead_bottom)[zone]
                self._step_range(self.bufs[(self.cur + s - 1) & 1], self.bufs[(self.cur + s) & 1], lo, hi)

    def slab_step(self, n):
        assert 1 <= n <= self.K and not self.pending
        self._run(n, ("all",))
        self.cur = (self.cur + n) & 1
        self.steps += n

    def slab_step_phase(self, n, phase):
        assert 1 <= n <= self.K
        if phase == SLAB_PHASE_EDGES:
            assert not self.pending
            self._run(n, ("low", "high"))
            self.pending = n
        else:
            assert phase == SLAB_PHASE_INTERIOR and self.pending == n
            self._run(n, ("interior",))
            self.pending = 0
            self.cur = (self.cur + n) & 1
            self.steps += n


G = 96
RULES = ["default", "clustered", "life2d", "vn_b24_s135"]
PACKED_GROUPS = {"even_split": sl.even_split_geometries, "short_edge": sl.short_edge_geometries, "nearly_whole": sl.nearly_whole_geometries,
                 "window": sl.window_geometries, "deep_ghost_top": sl.deep_ghost_top_geometries, "aligned_and_not": sl.aligned_and_not_geometries}


def _run_group(geometries, name, and_rounds):
    r = rules(name)
    traj = sl.trajectory(G, name, r, seed=96 + and_rounds, and_rounds=and_rounds)
    eng = OracleEngine()
    for z0, nz, K, batches in geometries:
        for phased in (False, True):
            sl.run_lone_slab(eng, traj, r, z0, nz, K, batches, phased)
            assert eng.steps == sum(batches)


@pytest.mark.parametrize("name", RULES)
@pytest.mark.parametrize("group", list(PACKED_GROUPS))
def test_harness_on_shapes_of_an_even_split_and_longer(group, name):
    _run_group(PACKED_GROUPS[group](G), name, and_rounds=0 if group != "window" else 2)


@pytest.mark.parametrize("name", RULES)
@pytest.mark.parametrize("and_rounds", [0, 2])
def test_harness_on_shapes_no_even_split_produces(name, and_rounds):
    """A high ghost that straddles plane G; slabs with 0 < z0 < K, whose low ghost reaches below the dead face."""
    _run_group(sl.uneven_split_geometries(G), name, and_rounds)


@pytest.mark.parametrize("max_value", [1, 2])
def test_harness_on_the_unpacked_ring(max_value):
    """The one-u32-per-cell layout is a torus only on power-of-two grids (the reference's -1 wrap): 64 instead of 96."""
    Gu = 64
    r = rules("default")
    traj = sl.trajectory(Gu, "default", r, seed=64, layout=LAYOUT_UNPACKED, max_value=max_value)
    assert int(traj(0).max()) == max_value
    eng = OracleEngine()
    for z0, nz, K, batches in sl.ring_geometries(Gu):
        for phased in (False, True):
            sl.run_lone_slab(eng, traj, r, z0, nz, K, batches, phased, layout=LAYOUT_UNPACKED)


def test_harness_notices_a_wrong_plane():
    """The comparisons bite: a stand-in that puts the dead face one plane too low (global plane 0 then reads the all-ones ghost below
    it) fails, and the message names the first differing word."""

    class Leaky(OracleEngine):
        def _step_range(self, src, dst, lo, hi):
            if hi <= lo:
                return
            out = ol.packed_step_planes(self.G, src, self.z0 - self.K + 1, lo, hi, self.rules)  # global z off by one
            dst[lo * self.pw:hi * self.pw] = out[lo * self.pw:hi * self.pw]

    r = rules("default")
    traj = sl.trajectory(G, "default", r, seed=96)
    with pytest.raises(AssertionError, match=r"first at global z \d+ \(slab plane \d+\), y \d+, word \d+"):
        sl.run_lone_slab(Leaky(), traj, r, 2, 30, 5, (5, 3), False)


# ---- the resident slab kernel's geometries (tests/test_gpu_resident_slab_depths.py runs them at 1024): 352 is the smallest multiple of
# 32 above the longest array (288 planes) + the largest z0 of a slab that is no top slab + the longest trajectory
RES_G = 352
RES_RULE = "vn_b24_s135"


@pytest.fixture(scope="module")
def res_traj():
    yield sl.trajectory(RES_G, RES_RULE, rules(RES_RULE), seed=RES_G)
    for key in [k for k in sl._TRAJECTORIES if k[0] == RES_G]:
        del sl._TRAJECTORIES[key]


@pytest.mark.parametrize("PZ", range(4, 37, 2))
def test_resident_slab_geometries_put_the_dead_face_everywhere(PZ):
    """Every depth: the constraints of a geometry (asserted where they are made) and the positions of the dead face a wrong kernel
    would show at — at 1024, where the GPU test runs, and at the grid of the stand-in below."""
    for G in (1024, RES_G):
        at = sl.assert_resident_slab_coverage(G, PZ)
        assert {"bottom", "low_inside", "low_last", "top", "top_first"} <= {label for label, _, _ in at}
        by_label = {g[0]: g for g in sl.resident_slab_geometries(G, PZ)}
        assert sl.resident_slab_thin(*by_label["thin"][2:]) and not any(label in ("middle", "thin") for label, _, _ in at)
    # a thread's second y-face entry: the last plane of a layer in the low ghost, and plane 32 / 33 of the last layer in the high ghost
    assert sorted((label, p) for label, _, p in at if p >= 32) == {34: [("low_last", 33), ("straddle", 32)], 36: [("low_last", 35), ("straddle", 33)]}.get(PZ, [])


@pytest.mark.parametrize("PZ", [4, 20, 36])
def test_harness_on_the_resident_slab_geometries(res_traj, PZ):
    r = rules(RES_RULE)
    eng = OracleEngine()
    for label, z0, nz, K, batches in sl.resident_slab_geometries(RES_G, PZ):
        for phased in (False, True) if sl.resident_slab_thin(nz, K, batches) else (False,):
            seen = []
            sl.run_lone_slab(eng, res_traj, r, z0, nz, K, batches, phased, after_batch=seen.append)
            assert tuple(seen) == batches and eng.steps == sum(batches), label


class NoDeadFace(OracleEngine):
    """The resident slab kernel without its dead-face masks: every plane of the array in every sub-step (the outermost go stale one per
    sub-step: planes beyond the array read as zeros), and no plane has a dead face below it."""

    def _run(self, n, zones):
        for s in range(1, n + 1):
            src = self.bufs[(self.cur + s - 1) & 1]
            padded = np.concatenate([np.zeros(self.pw, np.uint32), src, np.zeros(self.pw, np.uint32)])
            out = ol.packed_step_planes(self.G, padded, 1, 1, self.L + 1, self.rules)  # global z = 1 .. L + 1 < G: none is 0
            self.bufs[(self.cur + s) & 1][:] = out[self.pw:-self.pw]


@pytest.mark.parametrize("PZ", [4, 20, 34, 36])
def test_a_missing_dead_face_shows_exactly_where_it_is_counted(res_traj, PZ):
    """`resident_slab_dead_planes` counts a geometry when a kernel without the mask must leave a wrong owned plane: the stand-in
    without any dead face fails on exactly those, and passes the others (`middle`, `thin`: no such plane in the array). A straddling
    high ghost whose copy of plane 0 lies 7 planes out is not counted in a batch of 8, and does not show."""
    r = rules(RES_RULE)
    geometries = sl.resident_slab_geometries(RES_G, PZ)
    if PZ >= 34:
        label, z0, nz, K, batches = geometries[-1]
        geometries.append(("straddle_too_far", RES_G - nz - 7, nz, K, batches))  # 7 planes above the last owned one: 9 sub-steps away
    counted = {label for label, _, _ in sl.resident_slab_dead_planes(RES_G, PZ, geometries)}
    assert "straddle_too_far" not in counted
    for label, z0, nz, K, batches in geometries:
        if label in counted:
            with pytest.raises(AssertionError, match="owned planes"):
                sl.run_lone_slab(NoDeadFace(), res_traj, r, z0, nz, K, batches, False)
        else:
            sl.run_lone_slab(NoDeadFace(), res_traj, r, z0, nz, K, batches, False)


def test_launch_lengths_follow_the_product_split():
    """`launches` (what the GPU tests assert their residues on) against the ranges written out by hand."""
    # nz 33, K 4, batch of 4: whole sub-steps update [s, 41 - s); phased: low [s, 12 - s), high [29 + s, 41 - s), interior between
    assert sl.launches(33, 4, (4,), False, False) == [(39,), (37,), (35,), (33,)]
    assert sl.launches(33, 4, (4,), False, True) == [(10, 10), (8, 8), (6, 6), (4, 4), (19,), (21,), (23,), (25,)]
    # the slab that owns plane 0: its low ghost is never computed
    assert sl.launches(37, 3, (3,), True, False) == [(39,), (38,), (37,)]
    assert sl.launches(37, 3, (2,), True, True) == [(4, 6), (3, 4), (29,), (31,)]
    # thin: the edge phase runs whole sub-steps
    assert sl.launches(7, 3, (3,), False, True) == [(11,), (9,), (7,)]
