"""Canon from Node.js (N-API addon -> libca3d.so): SHAPE of tests/census_cases.py at its three places, the empty universe and a 2 x 2 x 2
block through Ensemble.canon, then SHAPE turned six ways by Ensemble.compose — against `host.canon` of the same states, all 48
digests, 64-bit values as BigInt."""
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
def test_js_canon_on_gpu(tmp_path):
    import canon_cases as kc
    import census_cases as cc
    from cellularautomatons3d_amd import host

    block = host.cells_to_words(64, [(40 + i, 7 + j, 3 + k) for i, j, k in itertools.product((0, 1), repeat=3)])
    states = np.stack([cc.state("shape_0"), cc.state("shape_1"), cc.state("shape_2"), cc.state("empty"), block])
    want = [kc.reference(("js", k), s) for k, s in enumerate(states)]
    assert len({int(r["key"]) for r, _ in want[:3]}) == 1
    orientations = [0, 13, 20, 27, 34, 47]  # one of each permutation
    states.astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "universes": len(states), "orientations": orientations,
        "records": [{"key": str(int(r["key"])), "symmetry": str(int(r["symmetry"])), "orientation": int(r["orientation"]),
                     "population": int(r["population"]), "boxMin": list(host.unpack_box(r["box_min"])), "boxMax": list(host.unpack_box(r["box_max"]))}
                    for r, _ in want],
        "digests": [[str(int(d)) for d in dig] for _, dig in want]}))
    r = subprocess.run([NODE, "tests/js/canon_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
