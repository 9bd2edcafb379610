"""engine.summary() / engine.stepUntil() / EngineGroup.summary() from Node.js (N-API addon -> libca3d.so)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def _node(*args, timeout=300):
    return subprocess.run([NODE, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_js_wrapper_exposes_the_summary_surface():
    r = _node("-e", "const c=require('./cellularautomatons3d_amd/js/ca3d.js');"
                    "const ok=['summary','stepUntil'].every(m=>typeof c.Engine.prototype[m]==='function')&&typeof c.EngineGroup.prototype.summary==='function'"
                    "&&c.STOP_EXTINCT===1&&c.STOP_STILL===2;console.log(ok?'ok':'missing')")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.gpu
def test_js_summary_and_step_until_on_gpu():
    r = _node("tests/js/summary_gpu_check.js", timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
