"""Host-side pieces of bench.py that need no GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_auto_ghost_keeps_a_share_on_the_resident_slab_kernel():
    """Ghost depth when none is given: 32, or the deepest of 32 / 16 / 8 with which a rank's share of a 1024^3 von Neumann grid still divides
    into 8 tile layers of an even number of planes <= 36 (ca_resident.hip, resident_slab_planes)."""
    assert bench.auto_ghost(1024, "default", 8) == 32   # 128 + 64 planes: 24 per layer
    assert bench.auto_ghost(1024, "default", 4) == 16   # 256 + 32: 36 per layer (with 32 ghost planes it would be 40)
    assert bench.auto_ghost(1024, "default", 2) == 32   # 512 + ...: no resident form, the default depth
    assert bench.auto_ghost(1024, "clustered", 4) == 32 and bench.auto_ghost(2048, "default", 8) == 32 and bench.auto_ghost(1024, "default", 1) == 32
    for world in (4, 8):
        k = bench.auto_ghost(1024, "vn_b24_s135", world)
        planes = 1024 // world + 2 * k
        assert planes % 8 == 0 and (planes // 8) % 2 == 0 and planes // 8 <= 36


def test_plain_run_checks_nothing_unless_full():
    """A plain run times the headline only: the oracle leg before the timed region is on by default with --full alone."""
    assert bench.parse(["--steps", "100", "--warmup", "5"]).verify_steps == 0
    assert bench.parse(["--steps", "100", "--warmup", "5", "--full"]).verify_steps == 45
    assert bench.parse(["--gpus", "4", "--full"]).verify_steps == bench.auto_ghost(1024, "default", 4) + 8
    assert bench.parse(["--steps", "100", "--verify-steps", "12"]).verify_steps == 12


def test_dump_state_is_exact_and_bounded(tmp_path):
    """--dump-outputs: uint32 state words survive as float64; a state beyond the byte budget becomes the same seeded sample every time."""
    import numpy as np

    words = np.random.default_rng(5).integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
    words[:2] = (0xFFFFFFFF, 0x80000001)
    bench.dump_state(str(tmp_path / "a"), "state", words, 1 << 20)
    got = np.load(tmp_path / "a" / "state.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), words)
    bench.dump_state(str(tmp_path / "b"), "state", words, 8 * 1000)
    bench.dump_state(str(tmp_path / "c"), "state", words, 8 * 1000)
    s1, s2 = np.load(tmp_path / "b" / "state.npy"), np.load(tmp_path / "c" / "state.npy")
    assert s1.size == 1000 and np.array_equal(s1, s2) and np.isin(s1, words.astype(np.float64)).all()
