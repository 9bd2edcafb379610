"""The JavaScript host path (north_star: host code stays Node.js over N-API)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def _node(*args, timeout=300):
    return subprocess.run([NODE, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_js_host_helpers_match_reference_fixtures():
    r = _node("tests/js/check_host_fixtures.js")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_js_cpu_stepper_hash_anchors():
    import json

    r = _node("oracle/js_stepper.js", "hash", "64", "8")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout)["hashes"] == "eaf84574 2a89e9f6 08947442 7e303b52 44d3c10e 3ca0f014 548cafef ae46dc87".split()


def test_js_engine_refuses_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = _node("-e", "const c=require('./cellularautomatons3d_amd/js/ca3d.js'); try{new c.Engine(0);process.exit(1)}catch(e){console.log(e.message)}")
    assert r.returncode == 0 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_js_engine_on_gpu(tmp_path):
    import oracle_lib as ol
    from cellularautomatons3d_amd import host

    W, H = 160, 90
    u = host.uniform_block(W, H, host.orbit_camera())
    u.tofile(tmp_path / "uniforms.f32")
    r = _node("tests/js/gpu_engine_check.js", str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
    state = np.fromfile(tmp_path / "state.u32", dtype=np.uint32)
    light = np.fromfile(tmp_path / "light.f16", dtype=np.float16).reshape(H, W, 4).astype(np.float32)
    pres = np.fromfile(tmp_path / "presentation.u8", dtype=np.uint8).reshape(H, W, 4)
    olight, _, opres, _ = ol.render(state, 128, u, W, H, 1)
    ok = (np.abs(light[..., :3] - olight[..., :3]).max(-1) <= 2e-3) & \
         (np.abs(pres.astype(np.float32) - np.rint(np.clip(opres, 0, 1) * 255)).max(-1) <= 1)
    assert ok.mean() >= 0.999


@pytest.mark.gpu
def test_js_engine_group_drives_the_slab_split_from_one_thread(tmp_path):
    """north_star: "host code stays JavaScript" + "Z-slabs across the 8 GPUs": EngineGroup (ca3d_group_*) from Node.js, 2 / 4 / 8
    slabs on GPU 0 over the peer-copy transport and one slab over RCCL (ncclCommInitAll + grouped exchange), states and a
    banded frame identical to one full-grid engine's."""
    from cellularautomatons3d_amd import host

    host.uniform_block(320, 176, host.orbit_camera()).tofile(tmp_path / "uniforms.f32")
    r = _node("tests/js/group_gpu_check.js", str(tmp_path), timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_node_bench_drives_several_slabs_from_one_thread():
    """js/bench.js --devices: the multi-GPU measurement of the north-star host (EngineGroup), rehearsed with four slabs on GPU 0;
    the state is first compared with a single grid's."""
    import json

    r = _node("cellularautomatons3d_amd/js/bench.js", "--devices", "0,0,0,0", "--grid", "512", "--ghost", "8", "--steps", "64", "--reps", "3",
              "--warmup", "16", "--check", "20")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["slabs"] == 4 and d["n_gpus"] == 1 and d["verified"]["state_matches_single_grid"] is True and d["value"] > 10
    # what the slabs ran on, from the engines: four slabs, ONE bus id here (a real 4-GPU run must show four)
    seen = d["devices_seen"]
    assert seen["slabs"] == 4 and seen["distinct_devices"] == 1 and len(seen["ranks"][0]["pci_bus_id"].split(":")) == 3
    assert [r["z0"] for r in seen["ranks"]] == [0, 128, 256, 384]


def test_facade_runs_the_unmodified_reference_host_with_a_mock_engine():
    """the WebGPU calls main_pathtraced.js + ui.js + MemoryManager.js, unmodified, make through init and five
    frames (recorded in tests/golden/reference_webgpu_calls.json) drive the navigator.gpu facade; a recording mock stands in
    for the engine."""
    r = _node("tests/js/facade_reference_mock.js")
    assert r.returncode == 0 and '"ok":true' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_facade_call_sequence_on_the_real_engine():
    r = _node("tests/js/facade_gpu_check.js")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]


@pytest.mark.gpu
def test_node_bench_reports_the_headline_metric(tmp_path):
    """The north-star host path (Node.js -> N-API -> libca3d.so) timed end to end: js/bench.js on a small run."""
    import json

    from cellularautomatons3d_amd import host

    host.uniform_block(1920, 1080, host.orbit_camera()).tofile(tmp_path / "u.f32")
    r = _node("cellularautomatons3d_amd/js/bench.js", "--grid", "256", "--steps", "256", "--warmup", "64", "--frames", "2",
              "--uniforms", str(tmp_path / "u.f32"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["kernel"].startswith("ca_resident_vn") and d["steps_per_launch"] == 256 and d["value"] > 100 and d["render"]["value"] > 10
    # a resident kernel is priced against vector-instruction issue (a fraction <= 1), not against HBM bytes it does not move
    rf = d["roofline"]
    # — and only against an instruction count profiled on the same kernel variant (rule, form options, device sources): the variant
    # that ran is on the line either way, the fraction when such a profile is committed
    assert rf["bound"] == "valu_issue" and rf["variant"].startswith("ca_resident_vn") and ";src=" in rf["variant"], rf
    if rf["frac"] is not None:
        assert rf["counter_source"] and 0.0 < rf["frac"] <= 1.0, rf
    else:
        assert "note" in rf
