"""The envelope over a period from Node.js (N-API addon -> libca3d.so): two of tests/test_gpu_envelope.py's cases — SURVEY's Moore
B4/S4 oscillator at its period and one past it, and tests/test_gpu_moving.py's glider over its period — through Ensemble.envelope,
records and all three images into a second ensemble, against `host.envelope` of the same states: what the Python binding is held to."""
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
def test_js_envelope_on_gpu(tmp_path):
    from cellularautomatons3d_amd import host
    from test_gpu_envelope import IMAGES, OSCILLATOR, mask
    from test_gpu_moving import SHIP, ship

    G = 64
    seed = host.cells_to_words(G, OSCILLATOR)
    universes = [(seed, ("4", "4"), 2), (seed, ("4", "4"), 3), (ship("a")[0], SHIP, 4)]
    want = [host.envelope(state, "moore", (mask(b), mask(s)), p) for state, (b, s), p in universes]
    assert [int(w[0]["flags"]) for w in want] == [host.ENVELOPE_RETURNS, 0, 0]

    def plain(r):
        box = {name: [int(v) for v in r[field][:3]] for name, field in (("envelopeMin", "envelope_min"), ("envelopeMax", "envelope_max"),
                                                                          ("rotorMin", "rotor_min"), ("rotorMax", "rotor_max"))}
        return {"period": int(r["period"]), "returns": bool(int(r["flags"]) & host.ENVELOPE_RETURNS), "heat": int(r["heat"]),
                "populationSum": int(r["population_sum"]), "envelopePopulation": int(r["envelope_population"]),
                "statorPopulation": int(r["stator_population"]), "rotorPopulation": int(r["envelope_population"]) - int(r["stator_population"]), **box}

    np.stack([u[0] for u in universes]).astype("<u4").tofile(tmp_path / "states.bin")
    np.stack([np.stack(w[1:]) for w in want]).astype("<u4").tofile(tmp_path / "images.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "neighbourhood": "moore", "rules": [{"born": u[1][0], "survive": u[1][1]} for u in universes], "periods": [u[2] for u in universes],
        "images": list(IMAGES), "records": [plain(w[0]) for w in want]}))
    r = subprocess.run([NODE, "tests/js/envelope_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
