"""Device seeding from Node.js (N-API addon -> libca3d.so): Engine.seedState, Ensemble.seedStates / setRuleTables, stepUntil, records
against Engine.summary() of lone engines and states against the JS definition seededState."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.mark.gpu
def test_js_seed_on_gpu():
    r = subprocess.run([NODE, "tests/js/seed_gpu_check.js"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
