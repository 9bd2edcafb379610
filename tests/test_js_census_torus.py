"""The torus census and isolate from Node.js (N-API addon -> libca3d.so): objects that cross a seam through `Ensemble.census` and
`Ensemble.isolate` with {connectivity}, against `host.census` and `host.isolate` of the same states."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import objects_torus_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

M = 16
#: the eight corners as they are (one object of the torus), and two states rolled by half a cube so that objects cross the faces
CASES = [("corners", (0, 0, 0)), ("shapes", (32, 32, 32)), ("shell_core", (32, 32, 32))]
PLACEMENTS = ["keep", "centre", "origin"]


def listed(ref):
    from cellularautomatons3d_amd import host

    comps, n, rest = ref
    assert rest == 0
    return [{"population": int(c["population"]), "firstCell": int(c["first_cell"]), "boxMin": list(host.unpack_box(c["box_min"])),
             "boxMax": list(host.unpack_box(c["box_max"])), "digest": str(int(c["digest"]))} for c in comps[:n]]


@pytest.mark.gpu
def test_js_torus_census_and_isolate_on_gpu(tmp_path):
    from cellularautomatons3d_amd import host

    states = np.stack([tc.state(n, d) for n, d in CASES])
    torus = [listed(tc.reference((n, d), tc.state(n, d), M)) for n, d in CASES]
    closed = [listed(tc.reference((n, d), tc.state(n, d), M, "closed")) for n, d in CASES]
    assert [len(v) for v in torus] == [1, 3, 2] and len(closed[0]) == 8 and len(closed[1]) > 3
    # the job: the shape that crosses the x face (its box runs past 63), by a cell in its middle
    across = [o for o in torus[1] if o["boxMax"][0] >= 64]
    assert len(across) == 1
    cells = tc.cells_list(host.isolate(states[1], across[0]["firstCell"], "keep", "torus")[0])
    job = {"universe": 1, "cell": int(cells[6]), "order": PLACEMENTS, "placements": {}}
    isolated = []
    for p in PLACEMENTS:
        words, pop, shift = host.isolate(states[1], job["cell"], p, "torus")
        job["placements"][p] = {"population": pop, "shift": list(shift)}
        isolated.append(words)
    assert job["placements"]["centre"]["population"] == 12
    states.astype("<u4").tofile(tmp_path / "states.bin")
    np.stack(isolated).astype("<u4").tofile(tmp_path / "isolated.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"universes": len(states), "maxComponents": M, "torus": torus, "closed": closed, "job": job}))
    r = subprocess.run([NODE, "tests/js/census_torus_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
