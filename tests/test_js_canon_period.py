"""Canon over a period from Node.js (N-API addon -> libca3d.so): the four phases of tests/test_gpu_moving.py's glider, one of them
with an untrue period, and tests/test_gpu_cycle.py's period-4 Moore oscillator through Ensemble.canonPeriod — against
`host.canon_period` of the oracle's phases of the same states, the key of every phase, 64-bit values as BigInt."""
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
def test_js_canon_period_on_gpu(tmp_path):
    import oracle_lib as ol
    from cellularautomatons3d_amd import host
    from test_gpu_cycle import MOORE as CYCLE_MOORE
    from test_gpu_moving import SHIP, ship

    G, W = 64, 8192
    t = ship("a")
    b, s, seed, rounds = CYCLE_MOORE[0]
    rule = ol.Rules.from_strings(neighbourhood="moore", born=b, survive=s)
    soup = host.random_fill(W, seed=seed, and_rounds=rounds)
    for _ in range(192):  # into its cycle: the period is looked for on the way
        soup = ol.packed_step(G, soup, rule)
    p = next(q for q in range(1, 65) if np.array_equal(ol.packed_run(G, soup, rule, q), soup))
    assert p >= 2
    universes = [(t[k], SHIP, 4) for k in range(4)] + [(t[1], SHIP, 3), (soup, (b, s), p)]
    want = []
    for state, (born, survive), period in universes:
        rules = ol.Rules.from_strings(neighbourhood="moore", born=born, survive=survive)
        phases = [np.ascontiguousarray(state, dtype=np.uint32)]
        for _ in range(period):
            phases.append(ol.packed_step(G, phases[-1], rules))
        want.append(host.canon_period(np.stack(phases)))
    assert len({int(r["key"]) for r, _ in want[:4]}) == 1 and all(int(r["flags_shift"]) & 1 for r, _ in want[:4])
    assert int(want[4][0]["flags_shift"]) == 0 and int(want[5][0]["flags_shift"]) == 1
    np.stack([u[0] for u in universes]).astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "neighbourhood": "moore", "rules": [{"born": u[1][0], "survive": u[1][1]} for u in universes], "periods": [u[2] for u in universes],
        "records": [{"key": str(int(r["key"])), "symmetry": str(int(r["symmetry"])), "orientation": int(r["orientation"]), "phase": int(r["phase"]),
                     "population": int(r["population"]), "closed": bool(int(r["flags_shift"]) & host.CANON_CLOSED),
                     "shift": list(host.unpack_shift(r["flags_shift"]))} for r, _ in want],
        "keys": [[str(int(k)) for k in keys] for _, keys in want]}))
    r = subprocess.run([NODE, "tests/js/canon_period_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
