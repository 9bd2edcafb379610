"""Device seeding, the part that needs no GPU: host.seeded_state — the definition of ca3d_seed_state in executable form — against
host.random_fill and host.state_summary, its JavaScript twin, and the surface (symbols, NULL refusals, classes)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cellularautomatons3d_amd import _capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
NEW = ["ca3d_seed_state", "ca3d_group_seed_state", "ca3d_ensemble_seed_state", "ca3d_ensemble_set_rule_tables"]
BOX = ((5, 0, 60), (40, 63, 63))  # x edges inside words 0 and 1 of a 64^3 row


def unpack(words, G):
    """0 / 1 per cell, x fastest, of a packed state of whole planes."""
    cols = G // 32
    return ((words.reshape(-1, G, cols, 1) >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, G, G)


@pytest.mark.parametrize("G", [32, 64, 96])
@pytest.mark.parametrize("and_rounds", [0, 2, 5])
def test_whole_grid_equals_random_fill(G, and_rounds):
    for seed in (1, 0xCA3D0001):
        np.testing.assert_array_equal(host.seeded_state(G, seed, and_rounds), host.random_fill(host.words_per_buffer(G), seed, and_rounds))


def test_unaligned_box():
    G = 64
    full = host.seeded_state(G, 3, 1)
    got = host.seeded_state(G, 3, 1, box=BOX)
    s = host.state_summary(G, got)
    assert (s["box_min"], s["box_max"]) == BOX
    assert s["population"] == 2325
    a, b = unpack(full, G), unpack(got, G)
    inside = np.zeros((G, G, G), dtype=bool)
    inside[BOX[0][2]:BOX[1][2] + 1, BOX[0][1]:BOX[1][1] + 1, BOX[0][0]:BOX[1][0] + 1] = True
    np.testing.assert_array_equal(b[inside], a[inside])
    assert not b[~inside].any()
    # a single cell, and a box that touches the - and the + faces
    one = host.seeded_state(G, 3, 0, box=((33, 7, 9), (33, 7, 9)))
    assert ol_popcount(one) == host.get_cell(G, host.seeded_state(G, 3, 0), 33, 7, 9)
    faces = host.seeded_state(G, 3, 0, box=((0, 0, 0), (63, 63, 0)))
    np.testing.assert_array_equal(faces[:128], host.seeded_state(G, 3, 0)[:128])
    assert not faces[128:].any()


def ol_popcount(w):
    return int(sum(bin(int(v)).count("1") for v in w[w != 0]))


@pytest.mark.parametrize("G,z0,nz", [(64, 0, 64), (64, 58, 4), (96, 31, 33), (32, 31, 1)])
def test_planes_are_a_slice(G, z0, nz):
    pw = (G // 32) * G
    box = ((3, 1, 2), (G - 2, G - 1, G - 3))
    for b in (None, box):
        full = host.seeded_state(G, 9, 2, box=b)
        np.testing.assert_array_equal(host.seeded_state(G, 9, 2, box=b, z0=z0, nz=nz), full[z0 * pw:(z0 + nz) * pw])
        cells = host.seeded_state(G, 9, 2, box=b, layout=1)
        np.testing.assert_array_equal(host.seeded_state(G, 9, 2, box=b, layout=1, z0=z0, nz=nz), cells[z0 * G * G:(z0 + nz) * G * G])


def test_unpacked_form():
    for G, box in ((64, None), (64, BOX), (96, ((31, 2, 0), (64, 95, 95)))):
        packed = host.seeded_state(G, 3, 1, box=box)
        np.testing.assert_array_equal(host.seeded_state(G, 3, 1, box=box, layout=1), unpack(packed, G).reshape(-1))
    small = host.seeded_state(12, 3, 1, layout=1)
    assert small.size == 1728 and small.dtype == np.uint32 and set(small.tolist()) == {0, 1}
    # G = 12: one packed word per row, index y + 12 z
    rows = host.random_fill(144, 3, 1)
    np.testing.assert_array_equal(small.reshape(144, 12), (rows[:, None] >> np.arange(12, dtype=np.uint32)) & 1)
    boxed = host.seeded_state(12, 3, 0, box=((2, 3, 4), (9, 3, 11)), layout=1).reshape(12, 12, 12)
    whole = host.seeded_state(12, 3, 0, layout=1).reshape(12, 12, 12)
    np.testing.assert_array_equal(boxed[4:12, 3, 2:10], whole[4:12, 3, 2:10])
    assert boxed.sum() == whole[4:12, 3, 2:10].sum()


def test_refused_specs():
    for kw in (dict(and_rounds=32), dict(box=((5, 0, 0), (4, 0, 0))), dict(box=((0, 0, 0), (64, 0, 0))), dict(z0=60, nz=5)):
        with pytest.raises(ValueError):
            host.seeded_state(64, 1, **kw)
    with pytest.raises(ValueError):
        host.seeded_state(12, 1)  # packed needs a multiple of 32


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_js_twin_equals_the_python_definition():
    specs = [dict(G=64, seed=3, andRounds=1, box=BOX, layout=0, z0=0, nz=64), dict(G=96, seed=0xCA3D0001, andRounds=2, box=None, layout=0, z0=31, nz=33),
             dict(G=64, seed=7, andRounds=0, box=((33, 7, 9), (33, 7, 9)), layout=0, z0=0, nz=64), dict(G=12, seed=3, andRounds=1, box=None, layout=1, z0=0, nz=12),
             dict(G=64, seed=5, andRounds=5, box=BOX, layout=1, z0=58, nz=4), dict(G=32, seed=4000000000, andRounds=0, box=None, layout=0, z0=0, nz=32)]
    script = """
const c = require(process.argv[1]);
const specs = JSON.parse(process.argv[2]);
const crypto = require("crypto");
console.log(JSON.stringify(specs.map(s => { const w = c.seededState(s.G, s.seed, {andRounds: s.andRounds, box: s.box ? {min: s.box[0], max: s.box[1]} : undefined, layout: s.layout, z0: s.z0, nz: s.nz});
  return [w.length, crypto.createHash("sha256").update(Buffer.from(w.buffer)).digest("hex")]; })));
"""
    r = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js"), json.dumps(specs)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    import hashlib

    got = json.loads(r.stdout)
    for s, (n, digest) in zip(specs, got):
        w = host.seeded_state(s["G"], s["seed"], s["andRounds"], s["box"], s["layout"], s["z0"], s["nz"])
        assert n == w.size and digest == hashlib.sha256(w.astype("<u4").tobytes()).hexdigest(), s


def test_symbols_declared_bound_and_exported():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "ca3d.h")).read()
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in bound and hasattr(lib, name), name
    assert "typedef struct ca3d_seed" in header
    assert C.sizeof(_capi.SeedStruct) == 32
    assert lib.ca3d_abi_version() == 7


def test_null_refusals_touch_no_device():
    lib = _capi.load()
    spec = _capi.SeedStruct()
    masks = (C.c_uint32 * 1)(0)
    calls = [lambda: lib.ca3d_seed_state(None, C.byref(spec)), lambda: lib.ca3d_group_seed_state(None, C.byref(spec)),
             lambda: lib.ca3d_ensemble_seed_state(None, 0, 1, C.byref(spec), 1), lambda: lib.ca3d_ensemble_set_rule_tables(None, 0, 1, masks, masks, 1)]
    for call in calls:
        assert call() == -1
        assert b"NULL" in lib.ca3d_last_error()


def test_class_surfaces():
    from cellularautomatons3d_amd import Engine, EngineGroup, Ensemble

    assert callable(Engine.seed_state) and callable(EngineGroup.seed_state)
    assert callable(Ensemble.seed_states) and callable(Ensemble.set_rule_tables)
    js = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "ca3d.js")).read()
    for method in ("seedState(spec)", "seedStates(first, specs, count)", "setRuleTables(first, bornMasks, surviveMasks, count)", "function seededState("):
        assert method in js, method
    assert js.count("seedState(spec)") == 2  # Engine and EngineGroup
    assert re.search(r"module\.exports = \{[^}]*\bseededState\b", js, flags=re.S)
    napi = open(os.path.join(ROOT, "cellularautomatons3d_amd", "js", "addon", "ca3d_napi.c")).read()
    for fn, sym in (("seedState", "ca3d_seed_state"), ("groupSeedState", "ca3d_group_seed_state"), ("ensembleSeedState", "ca3d_ensemble_seed_state"),
                    ("ensembleSetRuleTables", "ca3d_ensemble_set_rule_tables")):
        assert '{"%s",' % fn in napi and sym + "(" in napi, fn
