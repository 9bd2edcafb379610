"""Compose from Node.js (N-API addon -> libca3d.so): the doubled glider of tests/test_gpu_moving.py beside a 2 x 2 x 2 block, turned six
ways through Ensemble.compose, then composed once more over what is there — against `host.compose` of the same states, and
step_until_moving on the turned ship alone against `host.orient_vector`."""
import itertools
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
def test_js_compose_on_gpu(tmp_path):
    from cellularautomatons3d_amd import host
    from test_gpu_moving import SHIP, glider

    block = host.cells_to_words(64, list(itertools.product((0, 1), repeat=3)))
    states = np.stack([glider("xy", (28, 30, 30)), block])
    orientations = [0, 13, 20, 27, 34, 47]  # one of each permutation
    layouts = [[[0, o, [30, 30, 30]], [1, 0, [5 + o, 60, 63]]] for o in orientations]  # the block: half of it beyond the +z face
    composed = [host.compose(states, [(u, o, tuple(at)) for u, o, at in layout]) for layout in layouts]
    assert all(rec.tolist() == (14, 14, 0, 4) for _, rec in composed)
    moving = [{"period": 4, "shift": list(host.orient_vector(o, (1, 1, 0)))} for o in orientations]
    over_layouts = [[[0, o, [31, 30, 30]]] for o in orientations[::-1]]
    over = [host.compose(states, [(u, o, tuple(at)) for u, o, at in layout], base=composed[k][0]) for k, layout in enumerate(over_layouts)]
    assert any(int(rec["overlap"]) > 0 for _, rec in over)
    states.astype("<u4").tofile(tmp_path / "states.bin")
    np.stack([w for w, _ in composed]).astype("<u4").tofile(tmp_path / "composed.bin")
    np.stack([w for w, _ in over]).astype("<u4").tofile(tmp_path / "over.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "universes": len(states), "born": SHIP[0], "survive": SHIP[1], "layouts": layouts,
        "records": [[int(v) for v in rec.tolist()] for _, rec in composed], "moving": moving,
        "over": {"layouts": over_layouts, "records": [[int(v) for v in rec.tolist()] for _, rec in over]}}))
    r = subprocess.run([NODE, "tests/js/compose_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
