"""ca3d_summarize / ca3d_group_summarize / ca3d_step_until on the GPU against the numpy definition (host.state_summary) of
states computed by the CPU oracle — never read back from the engine. Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import LAYOUT_PACKED32, LAYOUT_UNPACKED, Ca3dError, _capi, host, slab
from gpu_common import rules, set_rules

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
STOP_EXTINCT, STOP_STILL = 1, 2


@pytest.fixture(scope=lambda fixture_name, config: os.environ.get("CA3D_TEST_ENGINE_SCOPE", "module"))
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


_TRAJ = {}


def trajectory(G, name, seed, rounds, steps):
    """Oracle states 0 .. steps of a random fill, computed once per module and extended on demand."""
    key = (G, name, seed, rounds)
    r = rules(name) if isinstance(name, str) else name
    if key not in _TRAJ:
        _TRAJ[key] = [host.random_fill(host.words_per_buffer(G), seed=seed, and_rounds=rounds)]
    t = _TRAJ[key]
    while len(t) <= steps:
        t.append(ol.packed_step(G, t[-1], r))
    return t


def check(s, want, step, where=""):
    """Every field of an engine Summary against a host.state_summary dict."""
    print(f"{where} step {step}: population {s.population} births {s.births} deaths {s.deaths} digest {s.digest:#018x} "
          f"box {s.box_min}-{s.box_max} has_previous {s.has_previous}")
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where
    if s.plane_population is not None:
        np.testing.assert_array_equal(s.plane_population, want["plane_population"], err_msg=where)


def summarize_unchanged(eng, planes=True):
    """summary() with the state and the step counter looked at before and after."""
    before, step = eng.read_state(), eng.info().step
    s = eng.summary(planes=planes)
    np.testing.assert_array_equal(eng.read_state(), before)
    assert eng.info().step == step
    return s


@pytest.mark.parametrize("G", [32, 64, 96, 128, 160, 256, 512])
@pytest.mark.parametrize("name", ["default", "clustered", "vn_b24_s135"])
@pytest.mark.parametrize("rounds", [0, 12])
def test_summary_equals_definition_and_oracle(eng, G, name, rounds):
    """After upload (no previous state), one step, three more (per-step kernels) and 24 more (resident kernels where the grid
    has them)."""
    t = trajectory(G, name, 0xCA3D0001 + G, rounds, 28)
    eng.configure(G)
    set_rules(eng, rules(name))
    eng.upload_state(t[0])
    done = 0
    for n in (0, 1, 3, 24):
        if n:
            eng.step(n)
        done += n
        cur, prev = t[done], (t[done - 1] if done else None)
        s = summarize_unchanged(eng)
        assert s.population == ol.popcount(cur)
        check(s, host.state_summary(G, cur, prev), done, f"{G} {name} and_rounds={rounds}")
        np.testing.assert_array_equal(eng.read_state(), cur)


def test_summary_1024(eng):
    G = 1024
    r = rules("default")
    st = host.random_fill(host.words_per_buffer(G), seed=1024)
    eng.configure(G)
    set_rules(eng, r)
    eng.upload_state(st)
    eng.step(2)
    cur = ol.packed_run(G, st, r, 2)
    s = eng.summary()
    print(f"1024: population {s.population} digest {s.digest:#018x}")
    assert s.step == 2 and s.has_previous
    assert s.population == ol.popcount(cur)
    assert s.digest == host.state_summary(G, cur)["digest"]
    eng.configure(32)  # give the memory back


def test_box_edges(eng):
    """Single cells at the 8 grid corners and at the word boundaries x = 31 / 32 / G - 1 of a 96^3 grid (rows of 3 words: not whole
    uint4)."""
    G = 96
    eng.configure(G)
    cells = [(x, y, z) for x in (0, G - 1) for y in (0, G - 1) for z in (0, G - 1)] + [(31, 40, 7), (32, 1, 95), (G - 1, 94, 50), (63, 0, 1), (64, 95, 94)]
    for c in cells:
        w = host.cells_to_words(G, [c])
        eng.upload_state(w)
        s = eng.summary(planes=True)
        check(s, host.state_summary(G, w), 0, f"cell {c}")
        assert s.population == 1 and s.box_min == c and s.box_max == c and s.plane_population[c[2]] == 1
    w = host.cells_to_words(G, cells)
    eng.upload_state(w)
    check(eng.summary(planes=True), host.state_summary(G, w), 0, "all edge cells")
    w = np.zeros(host.words_per_buffer(G), dtype=np.uint32)
    eng.upload_state(w)
    s = eng.summary(planes=True)
    check(s, host.state_summary(G, w), 0, "empty")
    assert s.box_min == (G, G, G) and s.box_max == (0, 0, 0) and s.digest == 0


@pytest.mark.parametrize("G", [64, 128])
def test_unpacked_layout(eng, G):
    r = rules("default")
    st = (host.random_fill(G ** 3, seed=3 + G) & 1).astype(np.uint32)
    eng.configure(G, LAYOUT_UNPACKED)
    set_rules(eng, r)
    eng.upload_state(st)
    states = [st]
    done = 0
    for n in (0, 1, 3):
        for _ in range(n):
            states.append(ol.unpacked_step(G, states[-1], r.main, r.survive, r.born))
        if n:
            eng.step(n)
        done += n
        s = summarize_unchanged(eng)
        want = host.state_summary(G, states[done], states[done - 1] if done else None, layout=LAYOUT_UNPACKED)
        assert want["population"] == int(np.count_nonzero(states[done]))
        check(s, want, done, f"unpacked {G}")
    # words other than 0 / 1: stored, digested, not alive (the legacy kernel's `st == 1u`)
    odd = st.copy()
    odd[::7] *= 3
    eng.upload_state(odd)
    check(eng.summary(planes=True), host.state_summary(G, odd, layout=LAYOUT_UNPACKED), 0, "unpacked words > 1")
    eng.configure(32)


def test_queue_mode(eng):
    G = 128
    t = trajectory(G, "vn_b24_s135", 55, 0, 12)
    eng.configure(G)
    set_rules(eng, rules("vn_b24_s135"))
    for queue, n in ((1, 5), (64, 5), (64, 12)):
        eng.upload_state(t[0])
        eng.set_option("queue", queue)
        eng.step(n)  # (queue 64: only encoded — the summary submits it)
        s = eng.summary(planes=True)
        eng.set_option("queue", 0)
        check(s, host.state_summary(G, t[n], t[n - 1]), n, f"queue {queue}")


def test_summary_between_pipelined_frames_changes_no_pixel(eng):
    G, W, H = 128, 320, 176
    t = trajectory(G, "default", 808, 0, 3)
    u = host.uniform_block(W, H, host.orbit_camera())
    eng.configure(G)
    set_rules(eng, rules("default"))
    eng.set_option("render_pipeline", 1)
    frames = []
    for with_summary in (False, True):
        eng.upload_state(t[0])
        eng.step(3)
        for _ in range(4):
            eng.render(u, W, H, 1, readback=False)
        if with_summary:
            check(eng.summary(planes=True), host.state_summary(G, t[3], t[2]), 3, "between frames")
        frames.append(eng.render(u, W, H, 1))
    for a, b in zip(*frames):
        np.testing.assert_array_equal(a, b)
    assert eng.recovered_launches() == 0


def _exchange(engs, layout):
    import torch

    names = {"send_low": 0, "send_high": 1, "recv_low": 2, "recv_high": 3}
    for e in engs:
        e.synchronize()
    regs = [{n: slab.device_tensor(*e.slab_region(i), 0) for n, i in names.items()} for e in engs]
    for rk in range(len(engs)):
        plan = slab.halo_plan(rk, len(engs), layout)
        if plan.send_low_to is not None:
            regs[plan.send_low_to]["recv_high"].copy_(regs[rk]["send_low"])
        if plan.send_high_to is not None:
            regs[plan.send_high_to]["recv_low"].copy_(regs[rk]["send_high"])
    torch.cuda.synchronize()


def test_slabs_and_group(eng):
    """256^3 as 8 slab engines on one GPU: per-slab numbers of the oracle state's planes, digests that add up to the full grid's,
    births / deaths after whole batches and after an EDGES + INTERIOR batch (per-step kernels: has_previous is 1, include/ca3d.h);
    EngineGroup.summary equals the single engine's."""
    from cellularautomatons3d_amd import SLAB_PHASE_EDGES, SLAB_PHASE_INTERIOR, Engine, EngineGroup

    G, P, K = 256, 8, 4
    name = "vn_b24_s135"
    r = rules(name)
    t = trajectory(G, name, 31, 0, 20)
    pw = (G // 32) * G
    engs = []
    for k in range(P):
        e = Engine(0)
        z0, nz = slab.slab_bounds(G, P, k)
        e.configure_slab(G, z0, nz, K, LAYOUT_PACKED32)
        set_rules(e, r)
        e.upload_state(t[0][z0 * pw:(z0 + nz) * pw])
        engs.append(e)
    eng.configure(G)
    set_rules(eng, r)
    eng.upload_state(t[0])

    def compare(step):
        total = 0
        for k, e in enumerate(engs):
            z0, nz = slab.slab_bounds(G, P, k)
            s = e.summary(planes=True)
            want = host.state_summary(G, t[step][z0 * pw:(z0 + nz) * pw], t[step - 1][z0 * pw:(z0 + nz) * pw] if step else None, z0=z0)
            if not s.has_previous:  # allowed by the contract where the previous state cannot be guaranteed: then both counts are 0
                want.update(has_previous=False, births=0, deaths=0)
            check(s, want, step, f"slab {k}")
            assert s.has_previous == (step > 0), "per-step slab batches keep the previous state (include/ca3d.h)"
            total = (total + s.digest) & M64
        full = eng.summary(planes=True)
        check(full, host.state_summary(G, t[step], t[step - 1] if step else None), step, "full grid")
        assert total == full.digest

    compare(0)
    for _ in range(4):
        _exchange(engs, LAYOUT_PACKED32)
        for e in engs:
            e.slab_step(K)
    eng.step(16)
    compare(16)
    _exchange(engs, LAYOUT_PACKED32)
    for e in engs:
        e.slab_step_phase(K, SLAB_PHASE_EDGES)
    with pytest.raises(Ca3dError) as ei:  # between the phases both buffers are mid-batch: there is no state to describe
        engs[3].summary()
    assert ei.value.code == -1
    for e in engs:
        e.slab_step_phase(K, SLAB_PHASE_INTERIOR)
    eng.step(4)
    compare(20)
    for e in engs:
        e.close()

    single = eng.summary(planes=True)
    with EngineGroup([0, 0, 0, 0]) as g:
        g.configure(G, K)
        g.set_rules(r.main, r.edges, r.corners, r.survive, r.born)
        g.upload_state(t[0])
        s0 = g.summary(planes=True)
        check(s0, host.state_summary(G, t[0]), 0, "group, after upload")
        g.step(20)
        gs = g.summary(planes=True)
        check(gs, host.state_summary(G, t[20], t[19]), 20, "group")
        np.testing.assert_array_equal(gs.plane_population, single.plane_population)
        for f in ("step", "population", "births", "deaths", "digest", "has_previous", "box_min", "box_max"):
            assert getattr(gs, f) == getattr(single, f), f


def first_still_step(G, name, seed):
    """Smallest s >= 1 with state_s == state_(s-1) on the oracle."""
    s = 1
    while True:
        t = trajectory(G, name, seed, 0, s)
        if np.array_equal(t[s], t[s - 1]):
            return s
        s += 1
        assert s < 64


@pytest.mark.parametrize("G,every", [(64, 1), (64, 8), (128, 1), (128, 8), (256, 8), (512, 8)])
def test_step_until_still(eng, G, every):
    r = rules("default")
    s = first_still_step(G, "default", 21)
    t = trajectory(G, "default", 21, 0, 16)
    print(f"{G}^3: first unchanged step {s}, population {ol.popcount(t[s])}")
    eng.configure(G)
    set_rules(eng, r)
    eng.upload_state(t[0])
    if G >= 256:
        assert eng.info().kernel_name.startswith(b"ca_resident"), eng.info().kernel_name
    done, reason, sm = eng.step_until(1000, check_every=every)
    want = s if every == 1 else -(-s // every) * every
    assert (done, reason) == (want, STOP_STILL)
    assert eng.info().step == done and sm.step == done
    t = trajectory(G, "default", 21, 0, done)
    np.testing.assert_array_equal(eng.read_state(), t[done])
    check(sm, host.state_summary(G, t[done], t[done - 1]), done, "step_until still")
    assert sm.births == 0 and sm.deaths == 0 and sm.population == ol.popcount(t[s])
    assert eng.recovered_launches() == 0
    # on entry the condition already holds: nothing is stepped
    assert eng.step_until(1000, check_every=every)[:2] == (0, STOP_STILL)


def test_step_until_extinct(eng):
    G = 64
    r = ol.Rules.from_strings(neighbourhood="moore", born="", survive="14-26")
    st = host.random_fill(host.words_per_buffer(G), seed=21)
    pops, cur, k = [ol.popcount(st)], st, 0
    while pops[-1]:
        cur = ol.packed_step(G, cur, r)
        pops.append(ol.popcount(cur))
        k += 1
        assert k < 64
    print("populations", pops)
    eng.configure(G)
    set_rules(eng, r)
    eng.upload_state(st)
    done, reason, sm = eng.step_until(100, check_every=1)
    assert done == k and reason & STOP_EXTINCT and sm.population == 0 and sm.step == k
    # at step k the state (empty) differs from step k - 1 (pops[k - 1] cells died): not STILL yet
    assert reason == STOP_EXTINCT and sm.has_previous and sm.deaths == pops[k - 1] and sm.births == 0
    assert sm.box_min == (G, G, G) and sm.box_max == (0, 0, 0) and sm.digest == 0
    assert not eng.read_state().any() and eng.info().step == k
    eng.upload_state(st)
    done, reason, _ = eng.step_until(100, check_every=1, extinct=False)  # only STILL is watched: one step later
    assert (done, reason) == (k + 1, STOP_STILL)


def test_step_until_neither(eng):
    G = 128
    t = trajectory(G, "vn_b24_s135", 21, 0, 20)
    eng.configure(G)
    set_rules(eng, rules("vn_b24_s135"))
    eng.upload_state(t[0])
    done, reason, sm = eng.step_until(20, check_every=8)
    assert (done, reason) == (20, 0) and eng.info().step == 20
    np.testing.assert_array_equal(eng.read_state(), t[20])
    check(sm, host.state_summary(G, t[20], t[19]), 20, "max_steps")
    assert sm.births > 10000 and sm.deaths > 10000
    assert eng.step_until(0, check_every=8)[:2] == (0, 0)


def test_argument_errors(eng):
    from cellularautomatons3d_amd import Engine

    G = 64
    t = trajectory(G, "default", 21, 0, 3)
    eng.configure(G)
    set_rules(eng, rules("default"))
    eng.upload_state(t[0])
    lib = _capi.load()
    st = _capi.SummaryStruct()
    done, reason = C.c_uint32(), C.c_uint32()
    with pytest.raises(Ca3dError) as ei:
        eng.step_until(10, check_every=0)
    assert ei.value.code == -1
    assert lib.ca3d_step_until(eng._h, 10, 1, 3, None, C.byref(done), C.byref(reason)) == -1
    assert lib.ca3d_step_until(eng._h, 10, 1, 4, C.byref(st), C.byref(done), C.byref(reason)) == -1
    assert lib.ca3d_summarize(eng._h, None, None) == -1
    with Engine(0) as fresh:
        with pytest.raises(Ca3dError) as ei:
            fresh.step_until(10)
        assert ei.value.code == -2
        assert lib.ca3d_summarize(fresh._h, C.byref(st), None) == -2
        fresh.configure(G)
        assert lib.ca3d_summarize(fresh._h, C.byref(st), None) == -2  # nothing uploaded
    with Engine(0) as sl:
        sl.configure_slab(G, 0, 32, 2)
        set_rules(sl, rules("default"))
        sl.upload_state(t[0][:32 * 2 * G])
        with pytest.raises(Ca3dError) as ei:
            sl.step_until(10)
        assert ei.value.code == -5
        assert sl.summary().population == ol.popcount(t[0][:32 * 2 * G])
    eng.step(3)
    np.testing.assert_array_equal(eng.read_state(), t[3])
    assert lib.ca3d_step_until(eng._h, 0, 1, 3, C.byref(st), None, None) == 0 and st.step == 3  # steps_done / reason are nullable
