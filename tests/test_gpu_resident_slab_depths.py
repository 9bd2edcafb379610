"""The resident slab kernel (ca_resident_kernel.inc, resident_slab_run<LS, LB, PZ>) at every tile depth it is selected for: PZ = 4, 6
.. 36 planes per tile layer, 17 kernels compiled at run time, of which the even splits of tests/test_gpu_slab.py reach 20, 24, 34 and
36. What changes with PZ: the rows either side of a thread's own held in registers (PZ <= 16, with a second barrier in front of the
pass) or read four planes at a time inside the pass; a half-filled last chunk of the LDS image (PZ % 4 == 2); one or two words per
thread and y face (two at 34 and 36); no look-ahead plane in the pass at 4, 6 and 8; and the dead face below global plane 0, a run-time
plane index resolved in three places (the pass, the early first / last plane, the face pass).

One engine stands for one rank of a 1024^3 grid (tests/slab_lone.py: the oracle's full-grid states play its neighbours, every
comparison is exact); tests/test_slab_lone_cpu.py drives a CPU stand-in through the same geometries and shows that a kernel without the
dead face fails on exactly the geometries counted below."""
import pytest

import slab_lone as sl
from gpu_common import rules

pytestmark = pytest.mark.gpu

G = 1024
KERNEL = b"ca_resident_slab_vn(jit)"
# vn_b24_s135 goes by the parity of the count: each of the six neighbours decides in most cells. The start-up rule at the depths where
# the kernel's form changes (the shallowest, the last with rows in registers, the first without, the deepest).
RULES = {pz: ("vn_b24_s135", "default") if pz in (4, 16, 18, 36) else ("vn_b24_s135",) for pz in range(4, 37, 2)}


@pytest.fixture(scope="module", autouse=True)
def _drop_trajectories():
    """18 states of 128 MiB per rule, shared by all depths: gone with the module."""
    yield
    for key in [k for k in sl._TRAJECTORIES if k[0] == G and k[3] == 0 and k[2] == G + 1]:
        del sl._TRAJECTORIES[key]


@pytest.fixture
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("PZ", sorted(RULES))
def test_resident_slab_kernel_at_every_tile_depth(eng, PZ):
    """Every geometry whole, the thin one phased too (its edge phase is the resident launch, its interior phase commits it). Each batch
    must be ONE launch (a silent fall-back to the per-step kernels would make n), none may have timed out and been re-run, and a batch
    that ran as one resident launch leaves no state one step earlier behind (ca3d_summarize: has_previous == 0), whole or phased.

    Measured on an MI355X: 17 tests in 16.5 s; the first pays both oracle trajectories (17 steps of 1024^3 each) and takes 8.8 s, every
    other 0.2 .. 0.8 s."""
    geometries = sl.resident_slab_geometries(G, PZ)
    at = sl.assert_resident_slab_coverage(G, PZ)
    print(f"PZ {PZ}: geometries {[(g[0],) + g[1:] for g in geometries]}; dead face shows at (label, layer, position) {at}")
    assert any(sl.resident_slab_thin(nz, K, batches) for _, _, nz, K, batches in geometries)
    for name in RULES[PZ]:
        r = rules(name)
        traj = sl.trajectory(G, name, r, seed=G + 1, and_rounds=0)
        for label, z0, nz, K, batches in geometries:
            for phased in (False, True) if sl.resident_slab_thin(nz, K, batches) else (False,):
                what = f"PZ {PZ} {name} {label} {'phased' if phased else 'whole'}"
                count = [eng.info().launches_total]

                def one_launch(n):
                    now = eng.info().launches_total
                    assert now - count[0] == 1, f"{what}: a batch of {n} took {now - count[0]} launches"
                    count[0] = now
                    assert not eng.summary().has_previous, what

                sl.run_lone_slab(eng, traj, r, z0, nz, K, batches, phased, after_batch=one_launch)
                assert eng.info().kernel_name == KERNEL, (what, eng.info().kernel_name)
                assert eng.recovered_launches() == 0, what
