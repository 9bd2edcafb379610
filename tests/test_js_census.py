"""The census from Node.js (N-API addon -> libca3d.so): the closed faces, the translated shape and the glider beside a block of
tests/test_gpu_census.py through Ensemble.census, against `host.census` of the same states (the glider universe's from the oracle)."""
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

M = 16
NAMES = ["faces_x", "faces_y", "faces_z", "corners", "shape_0", "shape_1", "shape_2", "shapes"]


def listed(ref):
    from cellularautomatons3d_amd import host

    comps, n, rest = ref
    assert rest == 0
    return [{"population": int(c["population"]), "firstCell": int(c["first_cell"]), "boxMin": list(host.unpack_box(c["box_min"])),
             "boxMax": list(host.unpack_box(c["box_max"])), "digest": str(int(c["digest"]))} for c in comps[:n]]


@pytest.mark.gpu
def test_js_census_on_gpu(tmp_path):
    import oracle_lib as ol
    from cellularautomatons3d_amd import host
    from test_gpu_moving import SHIP, glider, moore_rules

    block = [(10 + i, 10 + j, 40 + k) for i, j, k in itertools.product((0, 1), repeat=3)]
    first = glider("xy", (28, 30, 30)) | host.cells_to_words(64, block)
    states = np.stack([cc.state(n) for n in NAMES] + [first])
    lists = [listed(cc.reference(n, M)) for n in NAMES] + [listed(cc.reference_of(("glider+block", 0), first, M))]
    assert [len(v) for v in lists] == [2, 2, 2, 8, 1, 1, 1, 3, 2]
    rules, state, ship = moore_rules(*SHIP), first, []
    for k in range(0, 13, 4):
        for _ in range(4 if k else 0):
            state = ol.packed_step(64, state, rules)
        ship.append(listed(cc.reference_of(("glider+block", k), state, M)))
    assert all(len(v) == 2 for v in ship) and len({v[0]["digest"] for v in ship}) == 1 and len({tuple(v[0]["boxMin"]) for v in ship}) == 4
    states.astype("<u4").tofile(tmp_path / "states.bin")
    (tmp_path / "expected.json").write_text(json.dumps({
        "universes": len(states), "maxComponents": M, "lists": lists, "corners": NAMES.index("corners"),
        "glider": {"born": SHIP[0], "survive": SHIP[1], "universe": len(NAMES), "every": 4, "lists": ship}}))
    r = subprocess.run([NODE, "tests/js/census_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
