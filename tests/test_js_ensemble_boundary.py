"""Ensemble boundaries from Node.js (N-API addon -> libca3d.so): one torus and one closed case — face, edge and corner cells and a fill —
stepped through the addon, against the states Python's Ensemble reads back after the same steps, which tests/test_gpu_ensemble_boundary.py
holds to the definition; the first universe is compared with host.ensemble_step here as well."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

G = 64
# (kind, boundary, born, survive, steps): born at 1, survive at 0 and 2 — a cell on a face spreads through it or not
CASES = [("moore", "torus", 1 << 1, 0b101, 3), ("clustered", "closed", [1 << 1] * 3, [0b101] * 3, 2)]


@pytest.mark.gpu
def test_js_ensemble_boundaries_on_gpu(tmp_path):
    from cellularautomatons3d_amd import Ensemble, host

    first = np.stack([host.cells_to_words(G, [c]) for c in ((0, 0, 0), (G - 1, G - 1, G - 1), (0, 30, G - 1), (31, 0, 20))] + [host.seeded_state(G, 41, 3)])
    states, cases = [], []
    with Ensemble(0) as ens:
        for kind, boundary, born, survive, steps in CASES:
            ens.configure(len(first), neighbourhood="moore", clustered=kind == "clustered")
            ens.set_boundary(boundary)
            if kind == "clustered":
                ens.set_clustered_tables(0, born, survive)
            else:
                ens.set_rule_tables(0, born, survive)
            ens.upload_state(0, first)
            ens.step(steps)
            got = ens.read_state()
            want = first[0]
            for _ in range(steps):
                want = host.ensemble_step(want, kind, (born, survive), boundary)
            np.testing.assert_array_equal(got[0], want)
            states.append(got)
            cases.append({"kind": kind, "boundary": boundary, "born": born, "survive": survive, "steps": steps})
    first.astype("<u4").tofile(tmp_path / "first.bin")
    np.stack(states).astype("<u4").tofile(tmp_path / "states.bin")  # [case][universe][8192] u32, little endian
    (tmp_path / "expected.json").write_text(json.dumps({"universes": len(first), "cases": cases}))
    r = subprocess.run([NODE, "tests/js/ensemble_boundary_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
