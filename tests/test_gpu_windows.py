"""`ca3d_cut_windows` / `ca3d_stamp_windows` on the GPU (csrc/ca_window.hip) against `host.cut_window` / `host.stamp_windows`, the numpy
restatement of the definition in include/ca3d.h, on states of the CPU oracle — never of the engine. Every comparison is exact, word for
word. The grids are the smallest at which the kernels can go wrong: 64 (two words a row: the first and the third word of a window row
coincide), 96 (three words, no power of two) and 128. tests/test_windows_cpu.py checks the host functions themselves."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_moving import MOVING, SHIP, glider, moore_rules

pytestmark = pytest.mark.gpu

GRIDS = (64, 96, 128)
MODES = ("or", "replace", "erase")
VN = ol.Rules.from_strings()
INVALID, NOT_CONFIGURED, UNSUPPORTED = -1, -2, -5

_KEPT = {}


def kept(key, make):
    """`make()`, computed once for the run under `key` and never changed."""
    if key not in _KEPT:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _KEPT[key] = v
    return _KEPT[key]


def dense(G, seed=None, and_rounds=0):
    return kept(("fill", G, seed, and_rounds), lambda: host.random_fill(host.words_per_buffer(G), seed=G if seed is None else seed, and_rounds=and_rounds))


def soup(k, and_rounds=1):
    return kept(("soup", k, and_rounds), lambda: host.random_fill(8192, seed=1000 + k, and_rounds=and_rounds))


def run(G, words, rules, steps, key):
    return kept(("run", key, G, steps), lambda: ol.packed_run(G, np.array(words), rules, steps))


def origins(G):
    """Every x of {0, 1, 31, 32, 33, G - 1, G - 32, G - 63} with a wrapping y and z, and every y, z of {0, 1, G - 1, G - 63} at x = 0."""
    xs = (0, 1, 31, 32, 33, G - 1, G - 32, G - 63)
    yz = (0, 1, G - 1, G - 63)
    return sorted({(x, yz[(i + 2) % 4], yz[(i + 3) % 4]) for i, x in enumerate(xs)} | {(x, G - 1, G - 63) for x in xs}
                  | {(0, y, z) for y in yz for z in yz})


@pytest.fixture()
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def twin():
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


def world(e, G, words=None, rules=VN):
    e.configure(G)
    e.set_rules(rules.main, rules.edges, rules.corners, rules.survive, rules.born)
    if words is not None:
        e.upload_state(words)


def hold(e, states, nb="von neumann"):
    e.configure(len(states), neighbourhood=nb)
    e.upload_state(0, np.stack(states))


def check_record(s, words, where):
    want = host.state_summary(64, words)
    assert s.step == 0 and not s.has_previous and (s.births, s.deaths) == (0, 0), where
    assert s.population == want["population"] and s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


def check_cut(ens, G, words, windows):
    got = {u: ens.read_state(u, 1)[0] for u, _ in windows}
    for u, at in windows:
        np.testing.assert_array_equal(got[u], host.cut_window(G, words, at), err_msg=f"universe {u}, origin {at}, grid {G}")


# ---------------------------------------------------------------------------------------------------------------- cut
@pytest.mark.parametrize("G", GRIDS)
def test_cut_origins_and_records(eng, ens, G):
    words = dense(G)
    world(eng, G, words)
    windows = list(enumerate(origins(G)))
    ens.configure(len(windows))
    eng.cut_windows(ens, windows)
    assert eng.windows_gpu_ms() > 0
    check_cut(ens, G, words, windows)
    for (u, at), s in zip(windows, ens.summaries()):
        check_record(s, host.cut_window(G, words, at), f"origin {at}")
    np.testing.assert_array_equal(eng.read_state(), words)
    assert eng.info().step == 0


def test_cut_300_windows_into_scattered_universes(eng, ens):
    G = 96
    words = dense(G)
    world(eng, G, words)
    rng = np.random.default_rng(5)
    universes = rng.permutation(330)[:300]
    windows = [(int(u), tuple(int(v) for v in rng.integers(0, G, 3))) for u in universes]
    ens.configure(330)
    eng.cut_windows(ens, windows)
    check_cut(ens, G, words, windows)
    for u, at in windows[::17]:
        check_record(ens.summaries(u, 1)[0], host.cut_window(G, words, at), f"universe {u}")
    left = sorted(set(range(330)) - set(int(u) for u in universes))
    assert len(left) == 30
    for u in left[::7]:  # a universe no window named has no state yet
        with pytest.raises(Ca3dError) as err:
            ens.read_state(u, 1)
        assert err.value.code == NOT_CONFIGURED


def test_cut_leaves_the_engine_alone(eng, ens):
    G = 64
    words = dense(G, 21, 1)
    world(eng, G, words)
    eng.step(2)
    ens.configure(2)
    before = eng.summary()
    eng.cut_windows(ens, [(1, (33, 63, 1)), (0, (0, 0, 0))])
    check_cut(ens, G, run(G, words, VN, 2, "alone"), [(1, (33, 63, 1)), (0, (0, 0, 0))])
    assert eng.info().step == 2 and eng.summary() == before and before.has_previous
    np.testing.assert_array_equal(eng.read_state(), run(G, words, VN, 2, "alone"))
    eng.step(1)
    np.testing.assert_array_equal(eng.read_state(), run(G, words, VN, 3, "alone"))


@pytest.mark.parametrize("G,steps", [(64, 1), (64, 3), (128, 1), (128, 3), (64, 9)])
def test_cut_sees_the_current_state(eng, ens, G, steps):
    """After 1 and 3 steps the current buffer is buffer 1; 9 steps at 64^3 are one resident launch."""
    words = dense(G, 22, 1)
    world(eng, G, words)
    eng.step(steps)
    assert eng.info().current_buffer == 1
    windows = [(0, (G - 1, G - 63, 31)), (1, (32, 0, G - 1))]
    ens.configure(2)
    eng.cut_windows(ens, windows)
    check_cut(ens, G, run(G, words, VN, steps, "current"), windows)
    assert eng.recovered_launches() == 0


def test_cut_behind_queued_steps(eng, ens):
    G = 64
    words = dense(G, 22, 1)
    world(eng, G, words)
    eng.set_option("queue", 64)
    eng.step(2)
    eng.step(3)  # encoded, never submitted or waited for
    windows = [(0, (1, 2, 3)), (1, (63, 63, 63))]
    ens.configure(2)
    eng.cut_windows(ens, windows)
    check_cut(ens, G, run(G, words, VN, 5, "current"), windows)
    assert eng.info().step == 5


def test_tiling_read_back_is_the_state(eng, ens):
    G = 128
    words = dense(G)
    world(eng, G, words)
    at = [tuple(int(v) for v in o) for o in host.window_tiling(G)]
    ens.configure(len(at))
    eng.cut_windows(ens, list(enumerate(at)))
    got = ens.read_state()
    back = host.stamp_windows(G, np.zeros_like(words), [(got[k], o) for k, o in enumerate(at)], "or")
    np.testing.assert_array_equal(back, words)


def test_tiling_of_a_seeded_512_grid(eng, ens):
    G = 512
    eng.configure(G)
    eng.seed_state(3, 1)
    words = kept("seeded512", lambda: host.seeded_state(G, 3, 1))
    at = [tuple(int(v) for v in o) for o in host.window_tiling(G)]
    assert len(at) == 512
    ens.configure(len(at))
    eng.cut_windows(ens, list(enumerate(at)))
    got = ens.read_state()
    grid = words.reshape(G, G, G // 32)
    for k, (x, y, z) in enumerate(at):  # 64 divides 512: a window is a block of whole words
        np.testing.assert_array_equal(got[k].reshape(64, 64, 2), grid[z:z + 64, y:y + 64, x // 32:x // 32 + 2], err_msg=str((x, y, z)))
    np.testing.assert_array_equal(got[77], host.cut_window(G, words, at[77]))


# -------------------------------------------------------------------------------------------------------------- stamp
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", GRIDS)
def test_stamp_origins(eng, ens, G, mode):
    """One call an origin, each on top of the last: the state is compared after every call."""
    words = np.array(dense(G, 31, 1))
    world(eng, G, words)
    hold(ens, [soup(0), soup(1, 3)])
    for k, at in enumerate(origins(G)):
        u = k & 1
        eng.stamp_windows(ens, [(u, at)], mode)
        words = host.stamp_windows(G, words, [(soup(0) if u == 0 else soup(1, 3), at)], mode)
        np.testing.assert_array_equal(eng.read_state(), words, err_msg=f"{mode} at {at}, grid {G}")
    assert eng.windows_gpu_ms() > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G,places", [(128, ((5, 0, 0), (40, 0, 0))), (64, ((33, 7, 9), (1, 7, 9))), (96, ((95, 95, 95), (64, 31, 80)))])
def test_stamp_two_windows_sharing_grid_words(eng, ens, G, places, mode):
    words = dense(G, 32, 1)
    world(eng, G, words)
    hold(ens, [soup(2), soup(3)])
    eng.stamp_windows(ens, list(enumerate(places)), mode)
    np.testing.assert_array_equal(eng.read_state(), host.stamp_windows(G, words, [(soup(2), places[0]), (soup(3), places[1])], mode))


@pytest.mark.parametrize("mode", MODES)
def test_stamp_300_overlapping_soups_in_either_order(eng, ens, mode):
    G, n, kinds = 128, 300, 12
    words = dense(G, 33, 1)
    rng = np.random.default_rng(8)
    windows = [(int(rng.integers(0, kinds)), tuple(int(v) for v in rng.integers(0, G, 3))) for _ in range(n)]
    hold(ens, [soup(10 + k) for k in range(kinds)])
    want = kept(("overlap", mode), lambda: host.stamp_windows(G, words, [(soup(10 + u), at) for u, at in windows], mode))
    got = []
    for order in (windows, windows[::-1]):
        world(eng, G, words)
        eng.stamp_windows(ens, order, mode)
        got.append(eng.read_state())
    np.testing.assert_array_equal(got[0], want)
    assert got[0].tobytes() == got[1].tobytes()
    np.testing.assert_array_equal(ens.read_state(), np.stack([soup(10 + k) for k in range(kinds)]))  # the ensemble is only read


def test_stamp_into_an_engine_without_a_state(eng, ens):
    G = 96
    world(eng, G)
    hold(ens, [soup(4, 3)])
    windows = [(0, (90, 1, 70)), (0, (10, 60, 5))]
    eng.stamp_windows(ens, windows, "or")
    want = host.stamp_windows(G, np.zeros(host.words_per_buffer(G), dtype=np.uint32), [(soup(4, 3), at) for _, at in windows], "or")
    np.testing.assert_array_equal(eng.read_state(), want)
    s = eng.summary()
    assert s.step == 0 and not s.has_previous and s.population == host.state_summary(G, want)["population"]
    eng.step(2)
    np.testing.assert_array_equal(eng.read_state(), ol.packed_run(G, want, VN, 2))


@pytest.mark.parametrize("G,before,queue", [(64, 3, 0), (64, 9, 0), (128, 3, 0), (64, 5, 64)])
def test_stamp_then_read_summarise_and_step(eng, ens, G, before, queue):
    """Behind plain steps, behind a resident launch (9 steps at 64^3) and behind steps that were only queued."""
    words = dense(G, 34, 2)
    world(eng, G, words)
    hold(ens, [soup(5, 2), soup(6, 2)])
    if queue:
        eng.set_option("queue", queue)
    eng.step(before)
    windows = [(0, (G - 1, 3, G - 40)), (1, (20, G - 10, 2))]
    eng.stamp_windows(ens, windows, "replace")
    want = host.stamp_windows(G, run(G, words, VN, before, "then"), [(soup(5, 2), windows[0][1]), (soup(6, 2), windows[1][1])], "replace")
    np.testing.assert_array_equal(eng.read_state(), want)
    s, ref = eng.summary(), host.state_summary(G, want)
    assert s.step == before == eng.info().step and not s.has_previous and (s.births, s.deaths) == (0, 0)
    assert s.population == ref["population"] and s.digest == ref["digest"]
    eng.step(5)
    after = ol.packed_run(G, want, VN, 5)
    np.testing.assert_array_equal(eng.read_state(), after)
    s = eng.summary()
    assert s.step == before + 5 and s.has_previous and s.digest == host.state_summary(G, after)["digest"]
    assert eng.recovered_launches() == 0


def test_stamp_and_the_renderer(eng, twin, ens):
    """The frame after a stamp is the frame of a fresh engine given the same words, bit for bit: frames drawn before the stamp (in flight
    when it comes) and two pipelined frames after it."""
    G, W, H = 64, 160, 90
    words = dense(G, 5, 3)
    world(eng, G, words)
    world(twin, G)
    hold(ens, [soup(7, 3)])
    u = host.uniform_block(W, H, host.orbit_camera())
    for _ in range(3):
        eng.render(u, W, H, 4, readback=False)
    eng.stamp_windows(ens, [(0, (40, 50, 60))], "replace")
    want_words = host.stamp_windows(G, words, [(soup(7, 3), (40, 50, 60))], "replace")
    assert not np.array_equal(want_words, words)
    for _ in range(2):
        eng.render(u, W, H, 4, readback=False)
    got = eng.render(u, W, H, 4)
    twin.upload_state(want_words)
    want = twin.render(u, W, H, 4)
    for x, y, what in zip(got, want, ("presentation", "light", "depth")):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=what)
    assert got[0][..., :3].any()
    np.testing.assert_array_equal(eng.read_state(), want_words)


@pytest.mark.parametrize("G", (96, 128))
def test_round_trip_through_a_tiling(eng, twin, ens, G):
    words = dense(G)
    world(eng, G, words)
    world(twin, G, dense(G, 35))
    at = [tuple(int(v) for v in o) for o in host.window_tiling(G)]
    ens.configure(len(at))
    eng.cut_windows(ens, list(enumerate(at)))
    twin.stamp_windows(ens, list(enumerate(at)), "replace")
    np.testing.assert_array_equal(twin.read_state(), words)
    np.testing.assert_array_equal(eng.read_state(), words)


def test_a_composed_ship_sails_in_a_big_world(eng, ens):
    """What it is for: the doubled glider, turned on the device by compose, stamped into a 128^3 world under Moore B6/S5-7, moves as
    its orientation says; a cut around it is found MOVING."""
    from cellularautomatons3d_amd import Ensemble

    G, k = 128, 3
    orientations = (0, 7, 21, 40)
    rules = moore_rules(*SHIP)
    with Ensemble(0) as objects, Ensemble(0) as probe:
        objects.configure(1, neighbourhood="moore")
        objects.set_rule_strings(0, born=SHIP[0], survive=SHIP[1], neighbourhood="moore")
        objects.upload_state(0, glider("xy", (28, 30, 30)))
        ens.configure(len(orientations), neighbourhood="moore")
        ens.compose([[(0, o, (30, 30, 30))] for o in orientations], src=objects)
        turned = ens.read_state()
        probe.configure(len(orientations), neighbourhood="moore")
        probe.set_rule_strings(_capi.ENSEMBLE_ALL, born=SHIP[0], survive=SHIP[1], neighbourhood="moore")
        at = (30, 40, 50)
        for j, o in enumerate(orientations):
            world(eng, G, None, rules)
            eng.stamp_windows(ens, [(j, at)], "or")
            stamped = eng.read_state()
            np.testing.assert_array_equal(stamped, host.stamp_windows(G, np.zeros_like(stamped), [(turned[j], at)], "or"))
            eng.step(4 * k)
            vector = host.orient_vector(o, (1, 1, 0))
            assert host.moved_by(G, stamped, eng.read_state()) == tuple(k * v for v in vector), o
            eng.cut_windows(probe, [(j, at)])
        done, reason, period, shift = probe.step_until_moving(64, 4)
        for j, o in enumerate(orientations):
            assert reason[j] == MOVING and period[j] == 4 and tuple(int(v) for v in shift[j]) == host.orient_vector(o, (1, 1, 0)), o


# ----------------------------------------------------------------------------------------------------------- refusals
def snapshot(engine, ensemble):
    out = []
    try:
        out += [engine.read_state().tobytes(), engine.info().step, engine.info().current_buffer]
    except Ca3dError as e:
        out.append(e.code)
    try:
        out += [ensemble.read_state().tobytes(), ensemble.summaries()]
    except Ca3dError as e:
        out.append(e.code)
    return out


def refused(engine, ensemble, code, pattern, call):
    before = snapshot(engine, ensemble)
    with pytest.raises(Ca3dError, match=pattern) as err:
        call()
    assert err.value.code == code, err.value
    assert snapshot(engine, ensemble) == before


def test_refusals(eng, twin, ens):
    from cellularautomatons3d_amd import Engine, Ensemble

    G = 96
    lib = _capi.load()
    one = host.window_records([(0, (0, 0, 0))])
    wp = one.ctypes.data_as(C.POINTER(_capi.WindowStruct))

    def raw(fn, *args):
        _capi.check(fn(*args))

    # not configured, either handle
    refused(eng, ens, NOT_CONFIGURED, "engine", lambda: eng.cut_windows(ens, [(0, (0, 0, 0))]))
    refused(eng, ens, NOT_CONFIGURED, "engine", lambda: eng.stamp_windows(ens, [(0, (0, 0, 0))]))
    world(eng, G)
    refused(eng, ens, NOT_CONFIGURED, "ensemble", lambda: eng.cut_windows(ens, [(0, (0, 0, 0))]))
    refused(eng, ens, NOT_CONFIGURED, "ensemble", lambda: eng.stamp_windows(ens, [(0, (0, 0, 0))]))
    ens.configure(3)
    # an engine without a state, a universe without a state
    refused(eng, ens, NOT_CONFIGURED, "no state to cut", lambda: eng.cut_windows(ens, [(0, (0, 0, 0))]))
    ens.upload_state(0, np.stack([soup(0), soup(1)]))
    refused(eng, ens, NOT_CONFIGURED, "window 1.*universe 2", lambda: eng.stamp_windows(ens, [(0, (0, 0, 0)), (2, (0, 0, 0))]))
    eng.upload_state(dense(G))
    ens.upload_state(2, soup(2))
    for mode in (None,) + MODES:
        call = (lambda w: eng.cut_windows(ens, w)) if mode is None else (lambda w, m=mode: eng.stamp_windows(ens, w, m))
        fn = lib.ca3d_cut_windows if mode is None else lib.ca3d_stamp_windows
        tail = (None,) if mode is None else (_capi.STAMP_MODES[mode], None)
        refused(eng, ens, INVALID, "NULL", lambda: raw(fn, None, ens._h, 1, wp, *tail))
        refused(eng, ens, INVALID, "NULL", lambda: raw(fn, eng._h, None, 1, wp, *tail))
        refused(eng, ens, INVALID, "NULL", lambda: raw(fn, eng._h, ens._h, 1, None, *tail))
        refused(eng, ens, INVALID, "1 to", lambda: call([]))
        refused(eng, ens, INVALID, "window 1: universe 3 of 3", lambda: call([(0, (0, 0, 0)), (3, (0, 0, 0))]))
        for axis in range(3):
            at = [5, 5, 5]
            at[axis] = G
            refused(eng, ens, INVALID, r"window 2: origin\[%d\] = %d" % (axis, G), lambda: call([(0, (0, 0, 0)), (1, (95, 95, 95)), (2, tuple(at))]))
    refused(eng, ens, INVALID, "window 2: universe 1", lambda: eng.cut_windows(ens, [(1, (0, 0, 0)), (0, (0, 0, 0)), (1, (5, 5, 5))]))
    refused(eng, ens, INVALID, "unknown mode 3", lambda: raw(lib.ca3d_stamp_windows, eng._h, ens._h, 1, wp, 3, None))
    with pytest.raises(ValueError):
        eng.stamp_windows(ens, [(0, (0, 0, 0))], "xor")
    n = C.c_int(0)
    _capi.check(lib.ca3d_device_count(C.byref(n)))
    if n.value > 1:
        with Ensemble(1) as far:
            hold(far, [soup(0)])
            refused(eng, far, INVALID, "device", lambda: eng.cut_windows(far, [(0, (0, 0, 0))]))
            refused(eng, far, INVALID, "device", lambda: eng.stamp_windows(far, [(0, (0, 0, 0))]))
    # unsupported engines: the unpacked layout, a slab, a grid below 64
    for configure, why in ((lambda e: e.configure(64, _capi.LAYOUT_UNPACKED), "packed"), (lambda e: e.configure_slab(128, 32, 64, 1), "slab"),
                           (lambda e: e.configure(32), "64")):
        configure(twin)
        refused(twin, ens, UNSUPPORTED, why, lambda: twin.cut_windows(ens, [(0, (0, 0, 0))]))
        refused(twin, ens, UNSUPPORTED, why, lambda: twin.stamp_windows(ens, [(0, (0, 0, 0))]))
    # and the handles still work
    eng.stamp_windows(ens, [(2, (95, 0, 95))], "erase")
    np.testing.assert_array_equal(eng.read_state(), host.stamp_windows(G, dense(G), [(soup(2), (95, 0, 95))], "erase"))
