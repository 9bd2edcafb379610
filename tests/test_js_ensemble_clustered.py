"""A clustered Ensemble from Node.js (N-API addon -> libca3d.so): four universes, states after a few steps and their records against
values computed here from the oracle (oracle_lib.packed_step, host.state_summary)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

KEYS = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")
# bench.py's clustered rule, edges only, corners only, plain Moore
RULES = [("5-7", "4-7", "4", "3-5", "3", "2-4"), ("", "", "3,4", "2-4", "", ""), ("", "", "", "", "2,3", "1-3"), ("5-7", "4-6", "27", "27", "27", "27")]
BITS = (27, 13, 9)
STEPS = (1, 3)  # compared after 1 and after 1 + 3 steps


@pytest.mark.gpu
def test_js_clustered_ensemble_on_gpu(tmp_path):
    import oracle_lib as ol
    from cellularautomatons3d_amd import host

    def mask(s, bits):
        m = 0
        for v in host.rules_components_to_values(s):
            m |= 1 << v
        return m & ((1 << bits) - 1)

    G, W = 64, 8192
    cases = []
    states = []
    for u, rule in enumerate(RULES):
        r = ol.Rules.from_strings(neighbourhood="moore", **dict(zip(KEYS, rule)))
        t = [host.random_fill(W, seed=301 + u, and_rounds=(0, 2, 5)[u % 3])]
        for _ in range(sum(STEPS)):
            t.append(ol.packed_step(G, t[-1], r))
        recs = []
        done = 0
        for n in STEPS:
            done += n
            d = host.state_summary(G, t[done], prev_words=t[done - 1])
            recs.append({"step": done, "population": int(d["population"]), "births": int(d["births"]), "deaths": int(d["deaths"]),
                         "digest": str(int(d["digest"])), "hasPrevious": bool(d["has_previous"]), "boxMin": [int(v) for v in d["box_min"]],
                         "boxMax": [int(v) for v in d["box_max"]]})
            states.append(t[done])
        cases.append({"rules": {"neighbourhood": "moore", "born": rule[0], "survive": rule[1], "bornEdges": rule[2], "surviveEdges": rule[3],
                                "bornCorners": rule[4], "surviveCorners": rule[5]},
                      "bornMasks": [mask(rule[2 * i], BITS[i]) for i in range(3)], "surviveMasks": [mask(rule[2 * i + 1], BITS[i]) for i in range(3)],
                      "seed": 301 + u, "andRounds": (0, 2, 5)[u % 3], "records": recs})
    # states.bin: [universe][check point][8192] u32, little endian
    np.stack(states).astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"steps": list(STEPS), "cases": cases}))
    r = subprocess.run([NODE, "tests/js/ensemble_clustered_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
