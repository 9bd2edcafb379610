"""Rule usage from Node.js (N-API addon -> libca3d.so): one universe of every ensemble kind — a graded state under a coded rule on a
torus, over three steps — through Ensemble.usage, every field of the record against `host.usage` of the same state: what the Python
binding is held to."""
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
def test_js_usage_on_gpu(tmp_path):
    import graded_lib as gl
    from cellularautomatons3d_amd import host
    from test_ensemble_boundary_cpu import rule_of, tables_of

    G, P = 64, 3
    state = gl.graded_state(G, "z", True)
    cases = []
    for kind in host.ENSEMBLE_KINDS:
        born, survive = tables_of(kind, rule_of(kind, 1))
        rec = host.usage(state, kind, (born, survive), P, "torus")
        print(kind, [int(v) for v in rec["used_born"]], [int(v) for v in rec["used_survive"]], int(rec["dead"].sum()), int(rec["alive"].sum()))
        cases.append({"kind": kind, "born": born, "survive": survive,
                      "record": {"steps": P, "usedBorn": [int(v) for v in rec["used_born"]], "usedSurvive": [int(v) for v in rec["used_survive"]],
                                 "dead": [int(v) for v in rec["dead"]], "alive": [int(v) for v in rec["alive"]]}})
    np.stack([state, np.zeros_like(state)]).astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"boundary": "torus", "steps": P, "cases": cases}))
    r = subprocess.run([NODE, "tests/js/usage_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
