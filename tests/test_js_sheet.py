"""The contact sheet from Node.js (N-API addon -> libca3d.so): three universes through Ensemble.renderSheet, 48 x 32 tiles in two
columns at 4 samples, against the presentation sheet assembled here from Engine.render frames ("render_skip" 0) of the same states,
byte for byte, as tests/test_gpu_sheet.py::test_empty_slot_and_sub_range does."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

W, H, COLUMNS, SPP = 48, 32, 2, 4


@pytest.mark.gpu
def test_js_sheet_on_gpu(tmp_path):
    from cellularautomatons3d_amd import Engine, host

    states = np.stack([host.seeded_state(64, seed, 4) for seed in (911, 912, 913)])
    u = host.uniform_block(W, H, host.orbit_camera()).astype(np.float32)
    sh, sw = host.sheet_shape(len(states), W, H, COLUMNS)
    sheet = np.zeros((sh, sw, 4), dtype=np.uint8)  # the fourth slot stays zero
    with Engine(0) as eng:
        eng.configure(64)
        eng.set_option("render_skip", 0)
        eng.set_option("render_indirect", 0)
        for k, s in enumerate(states):
            eng.upload_state(s)
            host.sheet_tile(sheet, k, W, H, COLUMNS)[...] = eng.render(u, W, H, SPP)[0]
    assert sheet[:H, :W, :3].max() > 12 and not np.array_equal(sheet[:H, :W], sheet[:H, W:])  # lit, and the tiles differ
    states.astype("<u4").tofile(tmp_path / "states.bin")
    u.astype("<f4").tofile(tmp_path / "uniforms.bin")
    sheet.tofile(tmp_path / "sheet.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"universes": len(states), "tileW": W, "tileH": H, "columns": COLUMNS, "spp": SPP,
                                                        "width": sw, "height": sh}))
    r = subprocess.run([NODE, "tests/js/sheet_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
