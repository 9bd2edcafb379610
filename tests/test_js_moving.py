"""Ensemble.stepUntilMoving from Node.js (N-API addon -> libca3d.so): the ships a, b and c of tests/test_gpu_moving.py in a Moore
ensemble, against expectations computed here from the oracle and the definition restated there."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.mark.gpu
def test_js_step_until_moving_on_gpu(tmp_path):
    import test_gpu_moving as m

    names = ["a", "b", "c"]
    trajs = [m.ship(n) for n in names]
    runs = []
    states = []
    for every in (1, 3):
        want = [m.expected(t, 0, 48, every, 15, False) for t in trajs]
        assert all(w[1] == m.MOVING for w in want)
        runs.append({"checkEvery": every, "maxSteps": 48, "stopMask": 15, "stepsDone": [w[0] for w in want], "reason": [w[1] for w in want],
                     "period": [w[2] for w in want], "shift": [int(v) for w in want for v in w[3]]})
        states += [t[w[0]] for t, w in zip(trajs, want)]
    # first.bin: the three start states; states.bin: [run][universe][8192] u32 after each run, little endian
    np.stack([t[0] for t in trajs]).astype("<u4").tofile(tmp_path / "first.bin")
    np.stack(states).astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"born": m.SHIP[0], "survive": m.SHIP[1], "runs": runs}))
    r = subprocess.run([NODE, "tests/js/moving_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
