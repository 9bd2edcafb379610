"""Windows from Node.js (N-API addon -> libca3d.so): one cut of wrapping windows and one overlapping stamp per mode through
Engine.cutWindows / Engine.stampWindows, against `host.cut_window` / `host.stamp_windows` of the same words."""
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
def test_js_windows_on_gpu(tmp_path):
    from cellularautomatons3d_amd import host

    G = 96
    words = host.random_fill(host.words_per_buffer(G), seed=61, and_rounds=1)
    soups = np.stack([host.random_fill(8192, seed=70 + k, and_rounds=2) for k in range(3)])
    cut = [[2, [95, 33, 0]], [0, [0, 0, 0]], [1, [33, 95, 40]]]
    stamp = [[0, [90, 90, 90]], [1, [70, 80, 90]], [2, [0, 0, 0]], [0, [31, 0, 5]]]  # overlapping, wrapping, one universe twice
    words.astype("<u4").tofile(tmp_path / "grid.bin")
    soups.astype("<u4").tofile(tmp_path / "soups.bin")
    by_universe = {u: host.cut_window(G, words, at) for u, at in cut}
    np.stack([by_universe[u] for u in range(3)]).astype("<u4").tofile(tmp_path / "cut.bin")
    for mode in host.STAMP_MODES:
        host.stamp_windows(G, words, [(soups[u], at) for u, at in stamp], mode).astype("<u4").tofile(tmp_path / f"stamp_{mode}.bin")
    (tmp_path / "expected.json").write_text(json.dumps({"gridSize": G, "cut": cut, "stamp": stamp, "modes": list(host.STAMP_MODES)}))
    r = subprocess.run([NODE, "tests/js/windows_gpu_check.js", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
