"""ca3d_seed_state / ca3d_group_seed_state / ca3d_ensemble_seed_state / ca3d_ensemble_set_rule_tables on the GPU. Expected values come
from host.seeded_state (the definition), host.state_summary and CPU-oracle trajectories — never from the engine. Every comparison is exact."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import LAYOUT_PACKED32, LAYOUT_UNPACKED, Ca3dError, _capi, host, slab
from gpu_common import rules, set_rules

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture()
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def boxes(G):
    """The whole grid, a single cell, a box touching the - and the + faces, a box whose x edges are not word-aligned."""
    return [None, ((G // 2 + 1, 7, G - 3), (G // 2 + 1, 7, G - 3)), ((0, 0, 0), (G - 1, G - 1, 1)), ((0, G - 2, 3), (G - 1, G - 1, G - 1)),
            ((5, 0, G - 4), (min(40, G - 2), G - 1, G - 1))]


def check(s, want, step, where):
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


# ------------------------------------------------------------------------------------------------------------------ 1. engine, packed
@pytest.mark.parametrize("G", [32, 64, 96, 256, 512])
def test_packed_engine_equals_the_definition(eng, G):
    eng.configure(G)
    for and_rounds in (0, 2, 5):
        for box in boxes(G):
            where = f"G={G} and_rounds={and_rounds} box={box}"
            eng.seed_state(1000 + G, and_rounds, box)  # rules need not be set
            want = host.seeded_state(G, 1000 + G, and_rounds, box)
            assert np.array_equal(eng.read_state(), want), where
            assert eng.info().step == 0
            s = eng.summary()
            check(s, host.state_summary(G, want), 0, where)
            assert not s.has_previous


# -------------------------------------------------------------------------------------------------------- 2. seeded equals uploaded
@pytest.mark.parametrize("G", [64, 256, 512])
@pytest.mark.parametrize("name", ["vn_b24_s135", "default"])
def test_seeded_equals_uploaded(eng, G, name):
    from cellularautomatons3d_amd import Engine

    r = rules(name)
    box = ((3, 0, 1), (G - 6, G - 1, G - 2))
    words = host.seeded_state(G, 77, 1, box)
    with Engine(0) as twin:
        for e in (eng, twin):
            e.configure(G)
            set_rules(e, r)
        eng.seed_state(77, 1, box)
        twin.upload_state(words)
        want, done = words, 0
        for n in (1, 24):
            eng.step(n)
            twin.step(n)
            if n == 24:  # 64^3: the one-workgroup form; 256^3 / 512^3: the tiled forms
                assert eng.info().kernel_name.startswith(b"ca_resident"), eng.info().kernel_name
            prev = ol.packed_run(G, want, r, n - 1)
            want = ol.packed_step(G, prev, r)
            done += n
            got = eng.read_state()
            assert np.array_equal(got, want), f"after {done} steps: seeded engine against the oracle"
            assert np.array_equal(twin.read_state(), got), f"after {done} steps: twin"
            a, b = eng.summary(planes=True), twin.summary(planes=True)
            np.testing.assert_array_equal(a.plane_population, b.plane_population)
            a.plane_population = b.plane_population = None
            assert a == b
            check(a, host.state_summary(G, want, prev), done, f"after {done} steps")
            assert eng.recovered_launches() == 0 and twin.recovered_launches() == 0


# --------------------------------------------------------------------------------------------------- 3. a seed in the middle of things
@pytest.mark.parametrize("G", [64, 256])
def test_seed_in_the_middle_of_things(eng, G):
    r = rules("vn_b24_s135")
    eng.configure(G)
    set_rules(eng, r)
    want = host.seeded_state(G, 5, 2)

    def seeded(where):
        assert np.array_equal(eng.read_state(), want), where
        assert eng.info().step == 0, where
        assert eng.recovered_launches() == 0, where
        s = eng.summary()
        check(s, host.state_summary(G, want), 0, where)
        eng.step(9)  # and the engine goes on from there
        assert np.array_equal(eng.read_state(), ol.packed_run(G, want, r, 9)), where
        assert eng.info().step == 9 and eng.recovered_launches() == 0, where

    # steps queued, not yet submitted
    eng.upload_state(host.random_fill(host.words_per_buffer(G), seed=3))
    eng.set_option("queue", 64)
    eng.step(5)
    eng.step(2)
    eng.seed_state(5, 2)
    seeded("queued steps")
    eng.set_option("queue", 0)
    # right behind a long batch nobody has looked at yet (G = 64 / 256: one resident launch)
    eng.upload_state(host.random_fill(host.words_per_buffer(G), seed=4))
    eng.step(24)
    eng.seed_state(5, 2)
    seeded("behind an unverified step(24)")
    # after the buffers were handed out
    eng.device_buffer(0)
    eng.seed_state(5, 2)
    seeded("after ca3d_device_buffer")
    eng.step(1)
    assert eng.summary().has_previous  # (the hand-out's "no previous state" ended with the seed and the step)


# ---------------------------------------------------------------------------------------------------------------------- 4. render
@pytest.mark.parametrize("literal", [False, True])
def test_frames_after_a_seed(eng, literal):
    from cellularautomatons3d_amd import Engine

    G, W, H = 64, 320, 180
    r = rules("default")
    a_words = host.random_fill(host.words_per_buffer(G), seed=11, and_rounds=3)
    box = ((9, 4, 2), (50, 60, 61))
    b_words = host.seeded_state(G, 12, 2, box)
    u = host.uniform_block(W, H, host.orbit_camera(), elapsed_time=0.3)
    with Engine(0) as twin:
        for e in (eng, twin):
            e.configure(G)
            set_rules(e, r)
            e.set_render_mode(literal)
        eng.upload_state(a_words)
        if literal:
            # the history surfaces are what an upload leaves them: the twin draws the same two frames with uploads
            eng.render(u, W, H, 1)
            twin.upload_state(a_words)
            twin.render(u, W, H, 1)
        else:
            for _ in range(3):  # frames that stay on the device: the pipeline is on (the default), later ones are in flight
                eng.render(u, W, H, 4, readback=False)
        eng.seed_state(12, 2, box)
        twin.upload_state(b_words)
        spp = 1 if literal else 4
        if not literal:
            eng.render(u, W, H, spp, readback=False)  # derived data (occupancy, bricks) of state A must not be reused
        got = eng.render(u, W, H, spp)
        want = twin.render(u, W, H, spp)
        for x, y, what in zip(got, want, ("presentation", "light", "depth")):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)
        assert got[0][..., :3].any()
        assert np.array_equal(eng.read_state(), b_words)


# -------------------------------------------------------------------------------------------------------------------- 5. unpacked
@pytest.mark.parametrize("G", [12, 64, 128])
def test_unpacked_engine(eng, G):
    r = ol.Rules.from_strings()
    eng.configure(G, LAYOUT_UNPACKED)
    set_rules(eng, r)
    hi = G - 2
    for and_rounds, box in ((0, None), (1, ((1, 0, 2), (hi, G - 1, hi))), (2, ((G // 2, 3, 3), (G // 2, 3, 3)))):
        where = f"G={G} and_rounds={and_rounds} box={box}"
        eng.seed_state(40 + G, and_rounds, box)
        want = host.seeded_state(G, 40 + G, and_rounds, box, layout=1)
        assert np.array_equal(eng.read_state(), want), where
        assert eng.info().step == 0
        check(eng.summary(), host.state_summary(G, want, layout=1), 0, where)
        eng.step(3)
        if G == 128:
            assert eng.info().kernel_name == b"ca_unpacked_ballot"  # binary_state is true after a seed
        cur = want
        for _ in range(3):
            cur = ol.unpacked_step(G, cur, r.main, r.survive, r.born)
        assert np.array_equal(eng.read_state(), cur), where


# ------------------------------------------------------------------------------------------------------------- 6. slabs and the group
@pytest.mark.parametrize("layout", [LAYOUT_PACKED32, LAYOUT_UNPACKED])
def test_slab_engines_fill_their_own_planes(layout):
    from cellularautomatons3d_amd import Engine

    G, P, K = 128, 4, 3
    box = ((5, 2, 30), (100, 127, 97))  # cuts through slabs 0 and 3, covers 1 and 2
    full = host.seeded_state(G, 21, 1, box, layout=layout)
    pw = full.size // G
    total = 0
    for k in range(P):
        z0, nz = slab.slab_bounds(G, P, k)
        with Engine(0) as e:
            e.configure_slab(G, z0, nz, K, layout)
            # dirty buffers first: the ghosts must come out zeroed
            e.upload_state(np.full(nz * pw, 1 if layout else 0xFFFFFFFF, dtype=np.uint32))
            e.seed_state(21, 1, box)
            assert np.array_equal(e.read_state(), full[z0 * pw:(z0 + nz) * pw]), f"slab {k}"
            s = e.summary()
            check(s, host.state_summary(G, full[z0 * pw:(z0 + nz) * pw], layout=layout, z0=z0), 0, f"slab {k}")
            total = (total + s.digest) & M64
            for which in (0, 1):
                ptr, nbytes = e.device_buffer(which)
                whole = slab.device_tensor(ptr, nbytes, 0).cpu().numpy().view(np.uint32)
                assert whole.size == (nz + 2 * K) * pw
                assert not whole[:K * pw].any() and not whole[(K + nz) * pw:].any(), f"slab {k}: ghosts of buffer {which}"
                assert np.array_equal(whole[K * pw:(K + nz) * pw], full[z0 * pw:(z0 + nz) * pw]), f"slab {k}: buffer {which}"
    assert total == host.state_summary(G, full, layout=layout)["digest"]


def _group_case(devices, layout, G, K):
    from cellularautomatons3d_amd import EngineGroup

    r = rules("default")
    box = ((2, 0, 1), (G - 3, G - 1, G - 1))
    want = host.seeded_state(G, 31, 1, box, layout=layout)
    with EngineGroup(devices) as g:
        g.configure(G, K, layout)
        g.set_rules(r.main, r.edges, r.corners, r.survive, r.born)
        g.seed_state(31, 1, box)
        assert np.array_equal(g.read_state(), want)
        check(g.summary(), host.state_summary(G, want, layout=layout), 0, "group after the seed")
        g.step(11)
        if layout == LAYOUT_PACKED32:
            after = ol.packed_run(G, want, r, 11)
        else:
            after = want
            for _ in range(11):
                after = ol.unpacked_step(G, after, r.main, r.survive, r.born)
        assert np.array_equal(g.read_state(), after)
        # a second seed on a stepped group: ghosts are refreshed again before the next batch
        g.seed_state(32, 0, None)
        g.step(2)
        again = host.seeded_state(G, 32, 0, None, layout=layout)
        if layout == LAYOUT_PACKED32:
            again = ol.packed_run(G, again, r, 2)
        else:
            for _ in range(2):
                again = ol.unpacked_step(G, again, r.main, r.survive, r.born)
        assert np.array_equal(g.read_state(), again)
        assert g.summary().step == 2


@pytest.mark.parametrize("layout,G,K", [(LAYOUT_PACKED32, 256, 4), (LAYOUT_UNPACKED, 64, 3)])
def test_group_of_four_ranks_on_one_device(layout, G, K):
    _group_case([0, 0, 0, 0], layout, G, K)


def test_group_across_two_devices():
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    _group_case([0, 1, 0, 1], LAYOUT_PACKED32, 256, 4)


# ----------------------------------------------------------------------------------------------------------------- 7. large grids
def test_1024_cubed(eng):
    G = 1024
    eng.configure(G)
    box = ((33, 0, 0), (1000, 1023, 1022))
    eng.seed_state(9, 0, box)
    want = host.seeded_state(G, 9, 0, box)
    assert np.array_equal(eng.read_state(), want)
    check(eng.summary(), host.state_summary(G, want), 0, "1024^3")
    eng.configure(32)


def test_2048_cubed_population_and_digest(eng):
    """1 GiB per buffer, word indices past 2^28: population, digest and per-plane counts of the whole grid against the definition, which
    the host evaluates 64 planes at a time (host.seeded_state with z0 / nz: no grid-sized temporaries)."""
    G, chunk = 2048, 64
    box = ((1, 0, 3), (2046, 2047, 2047))
    t0 = time.time()
    eng.configure(G)
    eng.seed_state(7, 1, box)
    s = eng.summary(planes=True)
    pop, dig, planes = 0, 0, []
    for z0 in range(0, G, chunk):
        w = host.state_summary(G, host.seeded_state(G, 7, 1, box, z0=z0, nz=chunk), z0=z0)
        pop += w["population"]
        dig = (dig + w["digest"]) & M64
        planes.append(w["plane_population"])
    print(f"2048^3 seed check: {time.time() - t0:.1f} s")
    assert s.population == pop and s.digest == dig and s.step == 0 and not s.has_previous
    np.testing.assert_array_equal(s.plane_population, np.concatenate(planes))
    assert s.box_min == (1, 0, 3) and s.box_max == (2046, 2047, 2047)
    eng.configure(32)  # release the 2 GiB before the next test


# -------------------------------------------------------------------------------------------------------------------- 8. ensemble
G64, W = 64, 8192
STOP_EXTINCT, STOP_STILL = 1, 2
# test_gpu_ensemble.py's rules and fills: universe u runs rule u % 10 from fill_of(u) = random_fill(8192, 1 + u, (0, 2, 5)[u % 3])
RULES = [("1,3", "0-6"), ("2,4", "1,3,5"), ("", ""), ("", "0-6"), ("3", "2,3"), ("1", ""), ("4-6", "3-6"), ("5,6", "4-6"), ("0", "0-6"), ("2", "1-3")]


def fill_of(u):
    return host.random_fill(W, seed=1 + u, and_rounds=(0, 2, 5)[u % 3])


def mask_of(text):
    m = 0
    for v in host.rules_components_to_values(text):
        m |= 1 << v
    return m


def set_rules_one_by_one(e, B):
    for u in range(B):
        e.set_rule_strings(u, born=RULES[u % 10][0], survive=RULES[u % 10][1])


def test_ensemble_seeds(ens):
    from cellularautomatons3d_amd import Ensemble

    B = 300
    ens.configure(B)
    set_rules_one_by_one(ens, B)
    seeds, rounds = 1 + np.arange(B), np.array([(0, 2, 5)[u % 3] for u in range(B)])
    ens.seed_states(0, seeds, rounds)
    first = [fill_of(u) for u in range(B)]
    got = ens.read_state()
    for u, s in enumerate(ens.summaries()):
        assert np.array_equal(got[u], first[u]), f"universe {u}"
        check(s, host.state_summary(G64, first[u]), 0, f"universe {u} after the seed")
        assert not s.has_previous
    ens.step(8)
    got = ens.read_state()
    recs = ens.summaries()
    for u in range(B):
        r = ol.Rules.from_strings(born=RULES[u % 10][0], survive=RULES[u % 10][1])
        prev = ol.packed_run(G64, first[u], r, 7)
        want = ol.packed_step(G64, prev, r)
        assert np.array_equal(got[u], want), f"universe {u} after 8 steps"
        check(recs[u], host.state_summary(G64, want, prev), 8, f"universe {u} after 8 steps")
    # step_until from a seed and from an upload of the same words
    with Ensemble(0) as twin:
        twin.configure(B)
        set_rules_one_by_one(twin, B)
        twin.upload_state(0, np.stack(first))
        ens.seed_states(0, seeds, rounds)
        d0, r0 = ens.step_until(64, check_every=8)
        d1, r1 = twin.step_until(64, check_every=8)
        np.testing.assert_array_equal(d0, d1)
        np.testing.assert_array_equal(r0, r1)
        assert len(set(r0.tolist())) > 1 and len(set(d0.tolist())) > 1  # the universes did end at different moments
        assert np.array_equal(ens.read_state(), twin.read_state())
        assert ens.summaries() == twin.summaries()

    # seeding [100, 120) of a stepped ensemble leaves every other universe alone
    before_state, before_recs = ens.read_state(), ens.summaries()
    box = ((5, 0, 60), (40, 63, 63))
    ens.seed_states(100, 500 + np.arange(20), 1, box)
    after_state, after_recs = ens.read_state(), ens.summaries()
    for u in range(B):
        if 100 <= u < 120:
            want = host.seeded_state(G64, 500 + u - 100, 1, box)
            assert np.array_equal(after_state[u], want), f"universe {u}"
            check(after_recs[u], host.state_summary(G64, want), 0, f"universe {u}")
        else:
            assert np.array_equal(after_state[u], before_state[u]) and after_recs[u] == before_recs[u], f"universe {u}"
    ens.step(3)
    recs = ens.summaries()
    assert recs[100].step == 3 and recs[119].step == 3 and recs[99].step == before_recs[99].step + 3


def test_one_spec_for_every_universe(ens):
    B = 37
    ens.configure(B)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, born="2,4", survive="1,3,5")
    box = ((0, 3, 0), (63, 63, 33))
    ens.seed_states(0, 99, 2, box)  # scalars: n_specs == 1
    want = host.seeded_state(G64, 99, 2, box)
    got = ens.read_state()
    for u in range(B):
        assert np.array_equal(got[u], want), f"universe {u}"
    assert all(s == ens.summaries()[0] for s in ens.summaries())
    check(ens.summaries()[5], host.state_summary(G64, want), 0, "universe 5")
    ens.seed_states(30, 98, 0, None, count=2)  # one spec, a sub-range
    got = ens.read_state()
    assert np.array_equal(got[30], host.seeded_state(G64, 98)) and np.array_equal(got[31], got[30])
    assert np.array_equal(got[29], want) and np.array_equal(got[32], want)


# ------------------------------------------------------------------------------------------------------------- 9. set_rule_tables
def test_rule_tables_in_one_call(ens):
    from cellularautomatons3d_amd import Ensemble

    assert (mask_of("2,4"), mask_of("1,3,5")) == (0x14, 0x2A)
    B = 50
    born = [mask_of(RULES[u % 10][0]) for u in range(B)]
    survive = [mask_of(RULES[u % 10][1]) for u in range(B)]
    seeds, rounds = 1 + np.arange(B), np.array([(0, 2, 5)[u % 3] for u in range(B)])
    ens.configure(B)
    ens.set_rule_tables(0, born, survive)  # ONE call
    ens.seed_states(0, seeds, rounds)
    ens.step(8)
    with Ensemble(0) as twin:
        twin.configure(B)
        set_rules_one_by_one(twin, B)
        twin.upload_state(0, np.stack([fill_of(u) for u in range(B)]))
        twin.step(8)
        assert np.array_equal(ens.read_state(), twin.read_state())
        assert ens.summaries() == twin.summaries()
    got = ens.read_state()
    for u in (0, 1, 4, 9, 11, 49):  # ... and the oracle
        r = ol.Rules.from_strings(born=RULES[u % 10][0], survive=RULES[u % 10][1])
        assert np.array_equal(got[u], ol.packed_run(G64, fill_of(u), r, 8)), f"universe {u}"
    # one pair for a range
    ens.set_rule_tables(10, 0x14, 0x2A, count=5)
    ens.seed_states(0, seeds, rounds)
    ens.step(4)
    got = ens.read_state()
    r = ol.Rules.from_strings(born="2,4", survive="1,3,5")
    for u in (10, 14):
        assert np.array_equal(got[u], ol.packed_run(G64, fill_of(u), r, 4)), f"universe {u}"
    r = ol.Rules.from_strings(born=RULES[5][0], survive=RULES[5][1])
    assert np.array_equal(got[15], ol.packed_run(G64, fill_of(15), r, 4))
    # a bit at position 7 or above is refused, and the universe is named
    bad = list(born)
    bad[23] |= 0x80
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_tables(0, bad, survive)
    assert e.value.code == -1 and "universe 23" in e.value.message
    with pytest.raises(Ca3dError) as e:
        ens.set_rule_tables(7, [1, 2, 3], [1, 2, 0x100])
    assert e.value.code == -1 and "universe 9" in e.value.message


# ------------------------------------------------------------------------------------------------------------------- 10. refusals
def spec_of(G, **kw):
    from cellularautomatons3d_amd.engine import _seed_spec

    s = _seed_spec(G, kw.get("seed", 1), kw.get("and_rounds", 0), kw.get("box"))
    return s


def test_refusals(eng, ens):
    from cellularautomatons3d_amd import EngineGroup

    lib = _capi.load()
    G = 64
    good = spec_of(G)
    bad = [spec_of(G, and_rounds=32), spec_of(G, box=((5, 0, 0), (4, 63, 63))), spec_of(G, box=((0, 9, 0), (63, 8, 63))), spec_of(G, box=((0, 0, 2), (63, 63, 1))),
           spec_of(G, box=((0, 0, 0), (64, 63, 63))), spec_of(G, box=((0, 0, 0), (63, 64, 63))), spec_of(G, box=((0, 0, 0), (63, 63, 64)))]

    def refused(rc, code, text=None):
        assert rc == code, lib.ca3d_last_error()
        if text:
            assert text in lib.ca3d_last_error()

    # engine
    refused(lib.ca3d_seed_state(None, C.byref(good)), -1, b"NULL")
    refused(lib.ca3d_seed_state(eng._h, None), -1, b"NULL")
    refused(lib.ca3d_seed_state(eng._h, C.byref(good)), -2)  # not configured
    eng.configure(G)
    for s in bad:
        refused(lib.ca3d_seed_state(eng._h, C.byref(s)), -1)
    eng.seed_state(1)  # no rules set: fine
    assert np.array_equal(eng.read_state(), host.seeded_state(G, 1))
    eng.configure(G, LAYOUT_UNPACKED)
    refused(lib.ca3d_seed_state(eng._h, C.byref(bad[4])), -1)
    # group
    refused(lib.ca3d_group_seed_state(None, C.byref(good)), -1, b"NULL")
    with EngineGroup([0, 0]) as g:
        refused(lib.ca3d_group_seed_state(g._h, None), -1, b"NULL")
        refused(lib.ca3d_group_seed_state(g._h, C.byref(good)), -2)
        g.configure(G, 2)
        for s in bad:
            refused(lib.ca3d_group_seed_state(g._h, C.byref(s)), -1)
        g.seed_state(1)
        assert np.array_equal(g.read_state(), host.seeded_state(G, 1))
    # ensemble
    one = (C.c_uint32 * 1)(0x14)
    three = (_capi.SeedStruct * 3)(good, good, good)
    refused(lib.ca3d_ensemble_seed_state(None, 0, 1, C.byref(good), 1), -1, b"NULL")
    refused(lib.ca3d_ensemble_set_rule_tables(None, 0, 1, one, one, 1), -1, b"NULL")
    refused(lib.ca3d_ensemble_seed_state(ens._h, 0, 1, C.byref(good), 1), -2)
    refused(lib.ca3d_ensemble_set_rule_tables(ens._h, 0, 1, one, one, 1), -2)
    ens.configure(4)
    refused(lib.ca3d_ensemble_seed_state(ens._h, 0, 4, None, 1), -1, b"NULL")
    refused(lib.ca3d_ensemble_set_rule_tables(ens._h, 0, 4, None, one, 1), -1, b"NULL")
    refused(lib.ca3d_ensemble_seed_state(ens._h, 0, 4, three, 3), -1)  # neither 1 nor count
    refused(lib.ca3d_ensemble_seed_state(ens._h, 0, 4, three, 0), -1)
    refused(lib.ca3d_ensemble_seed_state(ens._h, 2, 3, three, 3), -1)  # past the end
    refused(lib.ca3d_ensemble_seed_state(ens._h, 0, 0, three, 1), -1)
    refused(lib.ca3d_ensemble_set_rule_tables(ens._h, 0, 4, (C.c_uint32 * 3)(1, 2, 3), (C.c_uint32 * 3)(1, 2, 3), 3), -1)
    refused(lib.ca3d_ensemble_set_rule_tables(ens._h, 3, 2, one, one, 1), -1)
    for s in bad:
        refused(lib.ca3d_ensemble_seed_state(ens._h, 1, 1, C.byref(s), 1), -1, b"universe 1")
    mixed = (_capi.SeedStruct * 3)(good, good, bad[0])
    refused(lib.ca3d_ensemble_seed_state(ens._h, 1, 3, mixed, 3), -1, b"universe 3")
    # nothing above marked anything: stepping still wants rules and states
    with pytest.raises(Ca3dError) as e:
        ens.step(1)
    assert e.value.code == -2
    ens.seed_states(0, 5)  # rules need not be set first
    with pytest.raises(Ca3dError) as e:
        ens.step(1)
    assert e.value.code == -2 and "set_rules" in e.value.message
    ens.set_rule_tables(0, 0x0A, 0x7F)
    ens.step(1)
    r = ol.Rules.from_strings()
    assert np.array_equal(ens.read_state()[3], ol.packed_step(G, host.seeded_state(G, 5), r))
