"""The ensemble trace from Node.js (N-API addon -> libca3d.so): three von Neumann universes through Ensemble.stepTrace, against samples,
counts, (steps_done, reason) and final states computed here from the oracle (oracle_lib.packed_step, host.state_summary) and the
definition of include/ca3d.h as tests/test_gpu_trace.py restates it."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

# (born, survive, seed, and_rounds): an oscillator, a fixed point, one that dies
CASES = [("2", "1-3", 3, 5), ("1,3", "0-6", 1, 0), ("5,6", "4-6", 1, 0)]
MAX, EVERY = 32, 4


@pytest.mark.gpu
def test_js_trace_on_gpu(tmp_path):
    from test_gpu_trace import expected, trajectory

    cases, states = [], []
    for mask in (0, 3):
        for c in CASES:
            t = trajectory("von neumann", c, MAX)
            samples, count, done, reason = expected(t, 0, MAX, EVERY, mask, False)
            cases.append({"born": c[0], "survive": c[1], "seed": c[2], "andRounds": c[3], "stopMask": mask, "samples": samples.ravel().tolist(),
                          "nSamples": count, "stepsDone": done, "reason": reason})
            states.append(t[done])
    assert {c["reason"] for c in cases} >= {0, 2} and any(c["reason"] & 1 for c in cases)
    # states.bin: [mask][universe][8192] u32, little endian — the state each universe ends in
    np.stack(states).astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"maxSteps": MAX, "checkEvery": EVERY, "universes": len(CASES), "cases": cases}))
    r = subprocess.run([NODE, "tests/js/trace_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
