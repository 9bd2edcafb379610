"""`host.state_summary`: the definition of ca3d_summarize in numpy, pinned on states whose answer is known by construction."""
import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import LAYOUT_UNPACKED, _capi, host

M64 = (1 << 64) - 1


def test_single_cell():
    G = 96
    s = host.state_summary(G, host.cells_to_words(G, [(37, 5, 90)]))
    assert s["population"] == 1 and s["box_min"] == (37, 5, 90) and s["box_max"] == (37, 5, 90)
    assert s["has_previous"] is False and s["births"] == 0 and s["deaths"] == 0
    want = np.zeros(G, dtype=np.uint32)
    want[90] = 1
    np.testing.assert_array_equal(s["plane_population"], want)
    assert s["digest"] != 0


def test_eight_corners_and_the_empty_state():
    G = 64
    corners = [(x, y, z) for x in (0, G - 1) for y in (0, G - 1) for z in (0, G - 1)]
    s = host.state_summary(G, host.cells_to_words(G, corners))
    assert s["population"] == 8 and s["box_min"] == (0, 0, 0) and s["box_max"] == (63, 63, 63)
    assert s["plane_population"][0] == 4 and s["plane_population"][63] == 4 and s["plane_population"].sum() == 8
    e = host.state_summary(G, np.zeros(host.words_per_buffer(G), dtype=np.uint32))
    assert e["population"] == 0 and e["digest"] == 0 and e["box_min"] == (G, G, G) and e["box_max"] == (0, 0, 0)
    assert not e["plane_population"].any()


def test_births_and_deaths_are_set_arithmetic():
    G = 64
    before = {(1, 2, 3), (31, 0, 0), (32, 0, 0), (63, 63, 63), (10, 20, 30), (40, 41, 42)}
    after = {(31, 0, 0), (63, 63, 63), (5, 5, 5), (33, 0, 0), (40, 41, 42), (0, 63, 7), (17, 17, 17)}
    s = host.state_summary(G, host.cells_to_words(G, after), host.cells_to_words(G, before))
    assert s["has_previous"] is True
    assert s["births"] == len(after - before) and s["deaths"] == len(before - after) and s["population"] == len(after)
    assert s["box_min"] == (0, 0, 0) and s["box_max"] == (63, 63, 63)


def test_unpacked_layout_counts_words_equal_to_one():
    G = 8
    w = np.zeros(G ** 3, dtype=np.uint32)
    q = np.zeros(G ** 3, dtype=np.uint32)
    w[1 + 2 * G + 3 * G * G] = 1
    w[7 + 7 * G + 7 * G * G] = 5  # not alive for the legacy kernel, but a stored word: part of the digest
    q[1 + 2 * G + 3 * G * G] = 1
    q[0] = 1
    s = host.state_summary(G, w, q, layout=LAYOUT_UNPACKED)
    assert s["population"] == 1 and s["births"] == 0 and s["deaths"] == 1 and s["box_min"] == s["box_max"] == (1, 2, 3)
    assert s["digest"] == (host.digest_mix(1 + 2 * G + 3 * G * G, 1) + host.digest_mix(G ** 3 - 1, 5)) & M64


@pytest.mark.parametrize("G", [64, 96])
@pytest.mark.parametrize("rounds", [0, 3, 12])
def test_population_equals_the_oracle_popcount(G, rounds):
    st = host.random_fill(host.words_per_buffer(G), seed=5 + G, and_rounds=rounds)
    s = host.state_summary(G, st)
    assert s["population"] == ol.popcount(st) == int(s["plane_population"].sum())


def test_digest_scalar_restatement():
    G = 32
    st = host.random_fill(host.words_per_buffer(G), seed=9, and_rounds=1)
    total = 0
    for i, w in enumerate(st.tolist()):
        if w == 0:
            continue
        z = (((i << 32) | w) + 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        total = (total + z) & M64
    assert host.state_summary(G, st)["digest"] == total


@pytest.mark.parametrize("P", [2, 4])
def test_slab_digests_add_up_and_slab_boxes_are_global(P):
    G = 64
    st = host.random_fill(host.words_per_buffer(G), seed=77, and_rounds=2)
    full = host.state_summary(G, st)
    pw = (G // 32) * G
    nz = G // P
    parts = [host.state_summary(G, st[k * nz * pw:(k + 1) * nz * pw], z0=k * nz) for k in range(P)]
    assert sum(p["digest"] for p in parts) & M64 == full["digest"]
    assert sum(p["population"] for p in parts) == full["population"]
    np.testing.assert_array_equal(np.concatenate([p["plane_population"] for p in parts]), full["plane_population"])
    assert min(p["box_min"][2] for p in parts) == full["box_min"][2] and max(p["box_max"][2] for p in parts) == full["box_max"][2]
    flipped = st.copy()
    flipped[4321] ^= np.uint32(1 << 7)
    assert host.state_summary(G, flipped)["digest"] != full["digest"]


def test_symbols_are_listed():
    names = {n for n, _, _ in _capi.SYMBOLS}
    assert {"ca3d_summarize", "ca3d_group_summarize", "ca3d_step_until"} <= names
    import ctypes as C

    assert C.sizeof(_capi.SummaryStruct) == 5 * 8 + 7 * 4 + 4  # 72: the C struct's size (u64 alignment pads the tail)


def test_symbols_are_exported_by_the_built_library():
    import ctypes as C

    lib = C.CDLL(_capi.LIB_PATH)
    for name in ("ca3d_summarize", "ca3d_group_summarize", "ca3d_step_until"):
        assert hasattr(lib, name)
    # the argument checks that need no device
    lib.ca3d_step_until.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.ca3d_step_until(None, 1, 1, 3, None, None, None) == -1
    lib.ca3d_summarize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.ca3d_summarize(None, None, None) == -1
