"""CPU-side checks of the moving-pattern surface (CA3D_STOP_MOVING, ca3d_ensemble_step_until_moving): declared, bound, exported, a NULL
handle refused without touching a device or the outputs, wrapped for Python and JavaScript, and host.moved_by — the predicate on the CPU —
against a brute-force restatement on the oracle's glider states."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ca3d_ensemble_step_until_moving"
G = 64


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n: args for n, _, args in _capi.SYMBOLS}
    lib = _capi.load()
    assert re.search(r"^int " + NAME + r"\(", header, flags=re.M)
    assert NAME in bound and hasattr(lib, NAME)
    assert len(bound[NAME]) == len(bound["ca3d_ensemble_step_until_cycle"]) + 1  # + shift
    assert bound[NAME][-1] is C.POINTER(C.c_int32)
    assert re.search(r"\bCA3D_STOP_MOVING = 8\b", header)
    assert re.search(r"^#define CA3D_ABI_VERSION 7\b", header, flags=re.M) and lib.ca3d_abi_version() == 7  # an addition
    assert _capi.STOP_MOVING == 8


def test_a_null_handle_is_refused_with_the_outputs_untouched():
    lib = _capi.load()
    done, reason, period = (C.c_uint32 * 2)(77, 77), (C.c_uint32 * 2)(78, 78), (C.c_uint32 * 2)(79, 79)
    shift = (C.c_int32 * 6)(*[80] * 6)
    assert lib.ca3d_ensemble_step_until_moving(None, 4, 1, 15, done, reason, period, shift) == -1
    assert b"NULL" in lib.ca3d_last_error()
    assert list(done) == [77, 77] and list(reason) == [78, 78] and list(period) == [79, 79] and list(shift) == [80] * 6


def test_python_surface():
    from cellularautomatons3d_amd import Ensemble, engine

    assert engine.STOP_MOVING == 8 and (engine.STOP_EXTINCT, engine.STOP_STILL, engine.STOP_PERIODIC) == (1, 2, 4)
    p = inspect.signature(Ensemble.step_until_moving).parameters
    assert list(p) == ["self", "max_steps", "check_every", "stop_mask"]
    assert (p["check_every"].default, p["stop_mask"].default) == (8, 15)


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_js_wrapper_exposes_moving_detection():
    r = subprocess.run([shutil.which("node"), "-e",
                        "const c=require('./cellularautomatons3d_amd/js/ca3d.js');"
                        "const ok=typeof c.Ensemble.prototype.stepUntilMoving==='function'&&c.STOP_MOVING===8&&c.STOP_PERIODIC===4;"
                        "console.log(ok?'ok':'missing')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    assert NAME + "(" in napi and '{"ensembleStepUntilMoving",' in napi


def _cells(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def _brute(a_words, b_words):
    """The definition, cell by cell: both non-empty, both boxes strictly inside, d = box_min(b) - box_min(a) != 0, b == a rolled by d."""
    a, b = _cells(a_words), _cells(b_words)
    if not a.any() or not b.any():
        return None
    boxes = []
    for c in (a, b):
        z, y, x = np.nonzero(c)
        mn, mx = (x.min(), y.min(), z.min()), (x.max(), y.max(), z.max())
        if min(mn) < 1 or max(mx) > G - 2:
            return None
        boxes.append(mn)
    d = tuple(int(q - p) for p, q in zip(*boxes))
    if d == (0, 0, 0):
        return None
    return d if np.array_equal(b, np.roll(a, shift=d[::-1], axis=(0, 1, 2))) else None


def _glider(corner, flip):
    """Moore B6/S5-7's doubled glider in an xy plane, two layers along z; flip mirrors both plane axes."""
    cells = []
    for (p, q) in ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2)):
        for layer in (0, 1):
            cells.append((corner[0] + (2 - p if flip else p), corner[1] + (2 - q if flip else q), corner[2] + layer))
    return host.cells_to_words(G, cells)


def _states(first, steps=12):
    r = ol.Rules.from_strings(neighbourhood="moore", born="6", survive="5-7")
    t = [first]
    for _ in range(steps):
        t.append(ol.packed_step(G, t[-1], r))
    return t


def test_moved_by_is_the_definition():
    inner, plus, minus = _states(_glider((28, 30, 30), False)), _states(_glider((58, 58, 30), False)), _states(_glider((2, 20, 2), True))
    seen = {"moved": 0, "alike": 0, "face": 0}
    for t in (inner, plus, minus):
        for i in range(13):
            for j in range(13):
                want = _brute(t[i], t[j])
                assert host.moved_by(G, t[i], t[j]) == want, (i, j)
                seen["moved"] += want is not None
    # the ship, found at its period and at twice that, in both time directions
    assert host.moved_by(G, inner[0], inner[4]) == (1, 1, 0) and host.moved_by(G, inner[1], inner[9]) == (2, 2, 0)
    assert host.moved_by(G, inner[8], inner[4]) == (-1, -1, 0)
    # phases that only look alike (equal population and extents, displaced boxes, different cells): None
    for i in range(12):
        sa, sb = host.state_summary(G, inner[i]), host.state_summary(G, inner[i + 1])
        ext = lambda s: tuple(q - p for p, q in zip(s["box_min"], s["box_max"]))
        if sa["population"] == sb["population"] and ext(sa) == ext(sb) and sa["box_min"] != sb["box_min"]:
            seen["alike"] += 1
            assert host.moved_by(G, inner[i], inner[i + 1]) is None
    # equal states: None (the zero vector is excluded); the empty state: None
    assert host.moved_by(G, inner[3], inner[3]) is None
    assert host.moved_by(G, np.zeros(8192, dtype=np.uint32), np.zeros(8192, dtype=np.uint32)) is None
    assert host.moved_by(G, inner[0], np.zeros(8192, dtype=np.uint32)) is None
    # face-touching states: None, although the cells are a translate
    for t in (plus, minus):
        for i in range(9):
            s = host.state_summary(G, t[i + 4])
            if min(s["box_min"]) < 1 or max(s["box_max"]) > G - 2:
                seen["face"] += 1
                assert host.moved_by(G, t[i], t[i + 4]) is None
    on_face = _glider((0, 30, 30), False)  # a translate of inner[0] by (-28, 0, 0), on the - x face
    assert np.array_equal(np.roll(_cells(inner[0]), -28, axis=2), _cells(on_face)) and host.moved_by(G, inner[0], on_face) is None
    print(seen)
    assert seen["moved"] > 20 and seen["alike"] >= 1 and seen["face"] >= 2
