"""Damage spreading from Node.js (N-API addon -> libca3d.so): three of tests/test_gpu_damage.py's cases — the nine-cell row that heals
at 5 as a twin universe, three flips in a row that heal at 2, a soup with one flipped cell whose damage spreads — through
Ensemble.damage, records, curves and the image of the last difference into a second ensemble, against `host.damage` of the same
states: what the Python binding is held to."""
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
def test_js_damage_on_gpu(tmp_path):
    from cellularautomatons3d_amd import host
    from test_gpu_envelope import mask

    G, W = 64, 8192
    empty = np.zeros(W, dtype=np.uint32)
    row = host.cells_to_words(G, [(28 + i, 20, 26) for i in range(9)])
    soup = host.random_fill(W, seed=54)
    three = [(30 + i, 5, 7) for i in range(3)]
    # (state, (born, survive), steps, twin universe or None, flips); universe 3 is only a twin
    universes = [(empty, ("", "2"), 7, 3, []), (empty, ("", "2"), 4, None, three), (soup, ("4-6", "5-9"), 3, None, [(46, 0, 7)]),
                 (row, ("", "2"), None, None, None)]
    sources = universes[:3]
    want = [host.damage(state, "moore", (mask(b), mask(s)), p, twin=None if twin is None else universes[twin][0], flips=flips)
            for state, (b, s), p, twin, flips in sources]
    assert [int(w[1]["healed_at"]) for w in want] == [5, 2, host.DAMAGE_NEVER] and want[0][0].tolist() == [9, 7, 5, 3, 1, 0, 0, 0]
    assert int(want[2][1]["final_distance"]) > 1

    def plain(r):
        box = {name: [int(v) for v in r[field][:3]] for name, field in (("damageMin", "damage_min"), ("damageMax", "damage_max"),
                                                                          ("touchedMin", "touched_min"), ("touchedMax", "touched_max"))}
        healed = bool(int(r["flags"]) & host.DAMAGE_HEALED)
        return {"steps": int(r["steps"]), "healed": healed, "healedAt": int(r["healed_at"]) if healed else None,
                "finalDistance": int(r["final_distance"]), "initialDistance": int(r["initial_distance"]), "maxDistance": int(r["max_distance"]),
                "maxAt": int(r["max_at"]), "distanceSum": int(r["distance_sum"]), **box}

    np.stack([u[0] for u in universes]).astype("<u4").tofile(tmp_path / "states.bin")
    np.stack([w[2] for w in want]).astype("<u4").tofile(tmp_path / "images.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "neighbourhood": "moore", "rules": [{"born": u[1][0], "survive": u[1][1]} for u in universes], "steps": [u[2] for u in sources],
        "twins": [u[3] for u in sources], "flips": [u[4] for u in sources], "records": [plain(w[1]) for w in want],
        "curves": [w[0].tolist() for w in want]}))
    r = subprocess.run([NODE, "tests/js/damage_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
