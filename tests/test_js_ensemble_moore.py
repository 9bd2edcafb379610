"""A Moore Ensemble from Node.js (N-API addon -> libca3d.so): six universes, states after a few steps and their records against
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

RULES = [("5-7", "4-6"), ("1", ""), ("", "0-26"), ("6", "5-7"), ("25,26", "24-26"), ("0", "0-26")]
STEPS = (1, 4)  # compared after 1 and after 1 + 4 steps


@pytest.mark.gpu
def test_js_moore_ensemble_on_gpu(tmp_path):
    import oracle_lib as ol
    from cellularautomatons3d_amd import host

    G, W = 64, 8192
    cases = []
    states = []
    for u, (b, s) in enumerate(RULES):
        r = ol.Rules.from_strings(neighbourhood="moore", born=b, survive=s)
        t = [host.random_fill(W, seed=201 + u, and_rounds=(0, 2, 5)[u % 3])]
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
        cases.append({"born": b, "survive": s, "seed": 201 + u, "andRounds": (0, 2, 5)[u % 3], "records": recs})
    # states.bin: [universe][check point][8192] u32, little endian
    np.stack(states).astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"steps": list(STEPS), "cases": cases}))
    r = subprocess.run([NODE, "tests/js/ensemble_moore_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
