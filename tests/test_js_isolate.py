"""Isolate from Node.js (N-API addon -> libca3d.so): the glider beside a block of tests/test_gpu_isolate.py — one census, two jobs,
step_until_moving on the nursery — and every component of the crafted `shapes` state, through Ensemble.isolate, against `host.isolate`
of the same states and the definition of step_until_moving on oracle trajectories."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import census_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.mark.gpu
def test_js_isolate_on_gpu(tmp_path):
    from cellularautomatons3d_amd import host
    from test_gpu_moving import MOVING, SHIP, STILL, Trajectory, expected, glider, moore_rules

    block = [(10 + i, 10 + j, 40 + k) for i, j, k in itertools.product((0, 1), repeat=3)]
    first = glider("xy", (28, 30, 30)) | host.cells_to_words(64, block)
    states = np.stack([cc.state("shapes"), first])
    comps, n, rest = cc.reference_of(("glider+block", 0), first, 8)
    assert (n, rest) == (2, 0)
    jobs = [[1, int(c["first_cell"])] for c in comps[:2]]
    centred = [host.isolate(first, cell, "centre") for _, cell in jobs]
    assert [r[1] for r in centred] == [10, 8] and centred[0][2] == (2, 0, 1)
    moving = []
    for words, _, _ in centred:
        done, reason, period, shift = expected(Trajectory(words, moore_rules(*SHIP)), 0, 64, 4, 15, False)
        moving.append({"stepsDone": done, "reason": reason, "period": period, "shift": list(shift)})
    assert (moving[0]["reason"], moving[0]["period"], moving[0]["shift"]) == (MOVING, 4, [1, 1, 0]) and moving[1]["reason"] & STILL
    comps, n, rest = cc.reference("shapes", 64)
    assert (n, rest) == (3, 0)
    crafted_jobs = [[0, int(c["first_cell"])] for c in comps[:3]]
    at_origin = [host.isolate(states[0], cell, "origin") for _, cell in crafted_jobs]
    assert [list(r[2]) for r in at_origin] == [[-v for v in p] for p in cc.PLACES]
    states.astype("<u4").tofile(tmp_path / "states.bin")
    np.stack([r[0] for r in centred]).astype("<u4").tofile(tmp_path / "glider.bin")
    np.stack([r[0] for r in at_origin]).astype("<u4").tofile(tmp_path / "crafted.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "universes": len(states),
        "glider": {"born": SHIP[0], "survive": SHIP[1], "universe": 1, "jobs": jobs, "population": [r[1] for r in centred],
                   "shift": [list(r[2]) for r in centred], "moving": moving},
        "crafted": {"jobs": crafted_jobs, "placement": "origin", "population": [r[1] for r in at_origin],
                    "shift": [list(r[2]) for r in at_origin]}}))
    r = subprocess.run([NODE, "tests/js/isolate_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
