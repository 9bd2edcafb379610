"""Ensemble boundaries on the GPU: the *_torus and *_closed kernels (ca_ensemble_boundary.hip) behind ca3d_ensemble_set_boundary, for all
three kinds, through step, step_until, step_until_cycle, step_until_moving and step_until_trace. Every expected state comes from
host.ensemble_step — the numpy definition, which tests/test_ensemble_boundary_cpu.py pins to the CPU oracle — chained from the uploaded
state; every comparison is exact. Where the reference boundary is looked at, the expectation is the oracle's own (oracle_lib.packed_step):
what an ensemble computed before it had a boundary to choose."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_cycle import MOORE as CYCLE_MOORE, expected as expected_cycle
from test_gpu_moving import SHIP, Trajectory, expected as expected_moving, glider

pytestmark = pytest.mark.gpu

G, W = 64, 8192
EXTINCT, STILL, PERIODIC, MOVING = 1, 2, 4, 8
KINDS = ("von neumann", "moore", "clustered")
NEW = ("torus", "closed")


def mask(s, bits=27):
    m = 0
    for v in host.rules_components_to_values(s):
        m |= 1 << v
    return m & ((1 << bits) - 1)


class Chain:
    """The states of one universe under host.ensemble_step, computed on demand and kept for the module."""

    def __init__(self, first, kind, tables, boundary):
        self.t, self.kind, self.tables, self.boundary = [np.ascontiguousarray(first, dtype=np.uint32)], kind, tables, boundary

    def __getitem__(self, k):
        while len(self.t) <= k:
            self.t.append(host.ensemble_step(self.t[-1], self.kind, self.tables, self.boundary))
        return self.t[k]


_CHAINS = {}


def chain(key, first, kind, tables, boundary):
    """`key` names the first state and the rule; the rest of the cache key is given."""
    full = (key, kind, boundary)
    if full not in _CHAINS:
        _CHAINS[full] = Chain(first() if callable(first) else first, kind, tables, boundary)
    return _CHAINS[full]


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def configure(ens, n, kind, boundary="reference"):
    ens.configure(n, neighbourhood="von neumann" if kind == "von neumann" else "moore", clustered=kind == "clustered")
    assert ens.boundary == "reference"  # every configure goes back to the reference
    ens.set_boundary(boundary)


def set_tables(ens, kind, tables):
    """`tables`: one (born, survive) per universe, from universe 0."""
    born, survive = [t[0] for t in tables], [t[1] for t in tables]
    if kind == "clustered":
        ens.set_clustered_tables(0, np.array(born, dtype=np.uint32).reshape(-1, 3), np.array(survive, dtype=np.uint32).reshape(-1, 3))
    else:
        ens.set_rule_tables(0, np.array(born, dtype=np.uint32), np.array(survive, dtype=np.uint32))


def cells(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]


def pack(c):
    return np.packbits(np.ascontiguousarray(c, dtype=np.uint8).ravel(), bitorder="little").view("<u4").astype(np.uint32)


def rolled(words, shift):
    """The state translated by shift = (dx, dy, dz) on the torus."""
    return pack(np.roll(cells(words), shift=(shift[2], shift[1], shift[0]), axis=(0, 1, 2)))


def check_record(s, want, step, where):
    assert s.step == step, where
    assert s.population == want["population"], where
    assert s.has_previous == want["has_previous"], where
    assert (s.births, s.deaths) == (want["births"], want["deaths"]), where
    assert s.digest == want["digest"], where
    assert s.box_min == tuple(want["box_min"]) and s.box_max == tuple(want["box_max"]), where


# ---------------------------------------------------------------------------------------------- face, edge and corner cells

MID = (21, 30, 42)  # a face or edge cell's free coordinates: different on every axis


def face_cells():
    """The 26 cells on the 6 faces, 12 edges and 8 corners of the cube."""
    out = [tuple((0, MID[i], G - 1)[p] for i, p in enumerate(pick)) for pick in itertools.product((0, 1, 2), repeat=3) if pick != (1, 1, 1)]
    assert len(out) == 26
    return out


def grow_tables(kind):
    """Born at count 1 (clustered: edges born at 1 and corners born at 1 as well), survive at 0 and 2."""
    return ([1 << 1] * 3, [0b101] * 3) if kind == "clustered" else (1 << 1, 0b101)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("boundary", NEW)
@pytest.mark.parametrize("kind", KINDS)
def test_face_edge_and_corner_cells(ens, kind, boundary, steps):
    """One live cell per universe; after 1 step, and after 3 — an odd number: the kernel's two register sets have changed roles."""
    tables = grow_tables(kind)
    chains = [chain(("cell", c), host.cells_to_words(G, [c]), kind, tables, boundary) for c in face_cells()]
    configure(ens, len(chains), kind, boundary)
    set_tables(ens, kind, [tables] * len(chains))
    ens.upload_state(0, np.stack([t[0] for t in chains]))
    ens.step(steps)
    got = ens.read_state()
    recs = ens.summaries()
    for u, (c, t) in enumerate(zip(face_cells(), chains)):
        np.testing.assert_array_equal(got[u], t[steps], err_msg=f"{kind}, {boundary}: cell {c} after {steps} steps")
        check_record(recs[u], host.state_summary(G, t[steps], prev_words=t[steps - 1]), steps, f"cell {c}")
    # the boundary shows: a corner cell's successors differ between the two modes
    if steps == 1:
        other = chain(("cell", (0, 0, 0)), None, kind, tables, boundary)[1]
        assert int(cells(other).sum()) == {"von neumann": (7, 4), "moore": (27, 8), "clustered": (27, 8)}[kind][NEW.index(boundary)]


# ---------------------------------------------------------------------------------------------- seams

SHIP_TABLES = (mask(SHIP[0]), mask(SHIP[1]))
# name: (plane, flip, the axis it heads out along, the sign) — 3 cells from that face, heading out; the other coordinates mid-cube
HEADINGS = {"+x": ("xy", (False, False), 0, +1), "-x": ("xy", (True, False), 0, -1), "+y": ("yz", (False, False), 1, +1),
            "-y": ("yz", (True, False), 1, -1), "+z": ("xz", (False, False), 2, +1), "-z": ("xz", (False, True), 2, -1)}
CROSS = 40  # steps: ten cells along both axes of the ship's plane — the face lies 3 cells ahead and the ship is 3 long


def heading_corner(name):
    _, _, axis, sign = HEADINGS[name]
    corner = [30, 30, 30]
    corner[axis] = G - 3 - 3 if sign > 0 else 3  # its 3-cell box ends 3 cells before the face
    return tuple(corner)


def seam_universes():
    """[(name, first state, free-space chain, the translation that takes the free-space ship to the first state)]: the six headings, and
    a ship inside that crosses the word seam x = 31 / 32 and the wave seam z = 15 / 16 and meets no face."""
    out = []
    for name, (plane, flip, axis, sign) in HEADINGS.items():
        corner = heading_corner(name)
        far = list(corner)
        far[axis] = (corner[axis] + G // 2) % G  # the same ship half a cube away, where it meets no face in CROSS steps
        shift = [0, 0, 0]
        shift[axis] = G // 2
        free = chain(("free", name), glider(plane, tuple(far), flip), "moore", SHIP_TABLES, "closed")
        out.append((name, glider(plane, corner, flip), free, tuple(shift)))
    inside = glider("xz", (28, 30, 13), (False, False))
    out.append(("inside", inside, chain(("free", "inside"), inside, "moore", SHIP_TABLES, "closed"), (0, 0, 0)))
    return out


def test_a_ship_crosses_every_seam(ens):
    """Moore B6/S5-7's doubled glider. Torus: the state is the free-space state rolled. Closed: the definition's, and nothing ever shows
    on the far side. Reference, on the same handle after set_boundary: the oracle's, as ever."""
    unis = seam_universes()
    for name, first, free, shift in unis:
        c = cells(free[CROSS])
        assert c.sum() == 10 and not (c[0].any() or c[-1].any() or c[:, 0].any() or c[:, -1].any() or c[:, :, 0].any() or c[:, :, -1].any()), name
    assert np.array_equal(unis[0][1], rolled(unis[0][2][0], unis[0][3]))
    configure(ens, len(unis), "moore", "torus")
    ens.set_rule_tables(0, SHIP_TABLES[0], SHIP_TABLES[1])
    first = np.stack([u[1] for u in unis])

    ens.upload_state(0, first)
    ens.step(CROSS)
    got = ens.read_state()
    for k, (name, _, free, shift) in enumerate(unis):
        np.testing.assert_array_equal(got[k], rolled(free[CROSS], shift), err_msg=f"torus, heading {name}")
        np.testing.assert_array_equal(got[k], chain(("seam", name), first[k], "moore", SHIP_TABLES, "torus")[CROSS], err_msg=f"torus, heading {name}")

    ens.set_boundary("closed")
    assert ens.boundary == "closed"
    ens.upload_state(0, first)
    for done in (CROSS // 2, CROSS):
        ens.step(CROSS // 2)
        got = ens.read_state()
        for k, (name, _, free, shift) in enumerate(unis):
            np.testing.assert_array_equal(got[k], chain(("seam", name), first[k], "moore", SHIP_TABLES, "closed")[done], err_msg=f"closed, heading {name}")
            if name != "inside":
                _, _, axis, sign = HEADINGS[name]
                half = [slice(None)] * 3
                half[2 - axis] = slice(0, G // 2) if sign > 0 else slice(G // 2, G)  # [z, y, x]: the half behind the face it left through
                assert not cells(got[k])[tuple(half)].any(), f"closed, heading {name}: it reappeared"
    np.testing.assert_array_equal(got[-1], unis[-1][2][CROSS])  # inside: free space under every boundary

    ens.set_boundary("reference")
    ens.upload_state(0, first)
    ens.step(CROSS)
    got = ens.read_state()
    r = ol.Rules.from_strings(neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    for k, (name, _, free, shift) in enumerate(unis):
        want = ol.packed_run(G, first[k], r, CROSS)
        np.testing.assert_array_equal(got[k], want, err_msg=f"reference, heading {name}")
        print("reference, heading", name, "population after", CROSS, "steps:", int(cells(want).sum()))


# ---------------------------------------------------------------------------------------------- soups

VARIANTS = 6  # distinct (fill, rule) pairs of a soup test; universe u holds pair u % VARIANTS
VN_RULES = [("1,3", "0-6"), ("2,4", "1,3,5"), ("3", "2,3"), ("2", "1-3"), ("2,3", "1"), ("3,4", "0-2")]
MOORE_RULES = [("5", "4,5"), ("6", "5-7"), ("6-8", "5-8"), ("3", "2,3"), ("5-7", "4-7"), ("13-14,17-19", "13-26")]
SIDE_RULES = [("4", "3-5", "3", "2-4"), ("3,4", "2-4", "", ""), ("", "", "2,3", "1-3"), ("2", "", "1", ""), ("", "5-12", "", "0"), ("6", "1", "4", "8")]


def soup_tables(kind, v):
    if kind == "von neumann":
        return mask(VN_RULES[v][0], 7), mask(VN_RULES[v][1], 7)
    if kind == "moore":
        return mask(MOORE_RULES[v][0]), mask(MOORE_RULES[v][1])
    be, se, bc, sc = SIDE_RULES[v]
    return ([mask(MOORE_RULES[v][0]), mask(be, 13), mask(bc, 9)], [mask(MOORE_RULES[v][1]), mask(se, 13), mask(sc, 9)])


def expected_until(t, start, max_steps, every, stop_mask):
    """(steps_done, reason) of a step_until that begins at state t[start] (start > 0: it has a previous state)."""
    k = 0
    while True:
        cur = t[start + k]
        fired = ((0 if cur.any() else EXTINCT) | (STILL if np.array_equal(cur, t[start + k - 1]) else 0)) & stop_mask
        if fired or k == max_steps:
            return k, fired
        k += min(every, max_steps - k)


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("rounds", [0, 3], ids=["density 1/2", "density 1/16"])
@pytest.mark.parametrize("boundary", NEW)
@pytest.mark.parametrize("kind", KINDS)
def test_soups(ens, kind, boundary, rounds, B):
    """9 steps by step, then 64 at most by step_until (check_every 5, mask 3): states, records, steps_done and reason of every universe.
    B = 300 is more universes than compute units."""
    chains = [chain(("soup", rounds, v), lambda: host.seeded_state(G, 700 + v, rounds), kind, soup_tables(kind, v), boundary) for v in range(VARIANTS)]
    configure(ens, B, kind, boundary)
    set_tables(ens, kind, [soup_tables(kind, u % VARIANTS) for u in range(B)])
    ens.upload_state(0, np.stack([chains[u % VARIANTS][0] for u in range(B)]))

    def check(steps_of, what):
        state, recs = ens.read_state(), ens.summaries()
        for u in range(B):
            t, d = chains[u % VARIANTS], steps_of(u)
            np.testing.assert_array_equal(state[u], t[d], err_msg=f"{what}: universe {u} after {d} steps")
            if u < 2 * VARIANTS:  # (the records of the rest repeat these)
                check_record(recs[u], host.state_summary(G, t[d], prev_words=t[d - 1]), d, f"{what}: universe {u}")
            else:
                assert (recs[u].step, recs[u].digest) == (recs[u % VARIANTS].step, recs[u % VARIANTS].digest), f"{what}: universe {u}"

    ens.step(9)
    check(lambda u: 9, "step")
    want = [expected_until(chains[u % VARIANTS], 9, 64, 5, 3) for u in range(B)]
    done, reason = ens.step_until(64, check_every=5, stop_mask=3)
    got = list(zip(done.tolist(), reason.tolist()))
    print(kind, boundary, "and_rounds", rounds, "(steps_done, reason):", got[:VARIANTS])
    assert got == want
    check(lambda u: 9 + want[u][0], "step_until")


# ---------------------------------------------------------------------------------------------- cycle and trace under torus

OSCILLATORS = {4: CYCLE_MOORE[0], 2: CYCLE_MOORE[1]}  # period: (born, survive, seed, and_rounds) of tests/test_gpu_cycle.py's Moore set
_OSC = {}


def oscillator(period):
    """(state, tables): an object of the settled state of the fill that is an oscillator of exactly `period` on its own, centred in the
    cube. Found with the oracle (the fill's trajectory until it repeats), host.census and host.isolate; its own period by the definition."""
    if period not in _OSC:
        b, s, seed, rounds = OSCILLATORS[period]
        r = ol.Rules.from_strings(neighbourhood="moore", born=b, survive=s)
        cur, seen = host.random_fill(W, seed=seed, and_rounds=rounds), set()
        while cur.tobytes() not in seen:
            seen.add(cur.tobytes())
            cur = ol.packed_step(G, cur, r)
            assert len(seen) <= 200
        tables = (mask(b), mask(s))
        comps, n, _ = host.census(cur, 64)
        for c in comps[:n]:
            alone = host.isolate(cur, int(c["first_cell"]), "centre")[0]
            t = Chain(alone, "moore", tables, "closed")
            if [k for k in range(1, period + 1) if np.array_equal(t[k], alone)] == [period]:
                _OSC[period] = (alone, tables)
                break
    return _OSC[period]


def astride():
    """[(period, axis, state, tables)]: each oscillator translated along x, y and z in turn so that the seam 63 / 0 of that axis runs
    through the middle of the cells it occupies over its period — where the reference boundary, dead from the - side, would break it."""
    out = []
    for period in (2, 4):
        alone, tables = oscillator(period)
        t = Chain(alone, "moore", tables, "closed")
        union = np.bitwise_or.reduce([cells(t[k]) for k in range(period)])
        for axis in range(3):
            along = np.moveaxis(union, 2 - axis, 0)  # [z, y, x] with the seam's axis first
            at = np.flatnonzero(along.reshape(G, -1).any(axis=1))
            lo, hi = int(at[0]), int(at[-1])
            shift = [0, 0, 0]
            shift[axis] = -(lo + (hi - lo + 1) // 2)  # the upper half lands on 0 .., the lower half on .. 63
            moved = np.moveaxis(cells(rolled(pack(union), shift)), 2 - axis, 0)
            assert moved[0].any() and (moved[G - 1].any() or hi == lo), "it lies on both sides of the seam"
            out.append((period, axis, rolled(alone, shift), tables))
    return out


def test_cycle_and_trace_across_the_seams_of_a_torus(ens):
    unis = astride()
    chains = [chain(("astride", p, axis), state, "moore", tables, "torus") for p, axis, state, tables in unis]
    configure(ens, len(unis), "moore", "torus")
    set_tables(ens, "moore", [u[3] for u in unis])
    first = np.stack([u[2] for u in unis])
    ens.upload_state(0, first)
    want = [expected_cycle(t, 0, 64, 1, 7, False) for t in chains]
    done, reason, period = ens.step_until_cycle(64, check_every=1, stop_mask=7)
    got = list(zip(done.tolist(), reason.tolist(), period.tolist()))
    print("(steps_done, reason, period):", got)
    assert got == want
    assert [(g[1], g[2]) for g in got] == [(PERIODIC, p) for p, _, _, _ in unis]  # the true period
    state = ens.read_state()
    for u, t in enumerate(chains):
        np.testing.assert_array_equal(state[u], t[got[u][0]])

    ens.upload_state(0, first)
    K = 13
    samples, count, done, reason = ens.step_trace(K - 1, check_every=1, stop_mask=0)
    assert count.tolist() == [K] * len(unis) and done.tolist() == [K - 1] * len(unis) and not reason.any()
    for u, t in enumerate(chains):
        want = [(int(cells(t[0]).sum()), 0, 0)]
        for k in range(1, K):
            d = host.state_summary(G, t[k], prev_words=t[k - 1])
            want.append((int(d["population"]), int(d["births"]), int(d["deaths"])))
        assert [tuple(int(v) for v in row) for row in samples[u]] == want, f"universe {u}"


# ---------------------------------------------------------------------------------------------- moving under torus

class DefinitionTrajectory(Trajectory):
    """tests/test_gpu_moving.py's trajectory (states, populations, boxes) over a chain of the definition instead of the oracle."""

    def __init__(self, t):
        super().__init__(t[0], None)
        self.chain = t

    def __getitem__(self, k):
        return self.chain[k]


def test_a_ship_found_across_a_seam_of_a_torus(ens):
    """The glider crosses x = 63 / 0 (heading +x) and x = 0 / 63 (heading -x) between the anchor (check point 0) and check point 1, 32
    steps and 8 cells later: MOVING, period 32, and a shift congruent modulo 64 to period x velocity — the detector compares boxes, so it
    reports -56 for +8."""
    names = ["+x", "-x"]
    unis = {u[0]: u for u in seam_universes()}
    first = np.stack([unis[n][1] for n in names])
    trajs = [DefinitionTrajectory(chain(("seam", n), first[k], "moore", SHIP_TABLES, "torus")) for k, n in enumerate(names)]
    want = [expected_moving(t, 0, 64, 32, 15, False) for t in trajs]
    assert want == [(32, MOVING, 32, (-56, 8, 0)), (32, MOVING, 32, (56, 8, 0))]
    configure(ens, 2, "moore", "torus")
    ens.set_rule_tables(0, SHIP_TABLES[0], SHIP_TABLES[1])
    ens.upload_state(0, first)
    done, reason, period, shift = ens.step_until_moving(64, check_every=32, stop_mask=15)
    got = [(int(d), int(r), int(p), tuple(int(v) for v in s)) for d, r, p, s in zip(done, reason, period, shift)]
    print("(steps_done, reason, period, shift):", got)
    assert got == want
    for g, sign in zip(got, (+1, -1)):
        assert (g[3][0] - sign * g[2] // 4) % G == 0 and g[3][1] == g[2] // 4 and g[3][2] == 0  # a cell every four steps along both axes
    state = ens.read_state()
    for k, n in enumerate(names):
        np.testing.assert_array_equal(state[k], rolled(unis[n][2][32], unis[n][3]), err_msg=f"heading {n}: the rolled free-space phase")


# ---------------------------------------------------------------------------------------------- switching and refusals

def test_each_step_call_runs_under_the_mode_set_before_it(ens):
    """set_boundary between two step calls that nothing synchronises: the first keeps the torus, the second runs closed."""
    tables = grow_tables("moore")
    firsts = [host.cells_to_words(G, [c]) for c in face_cells()]
    configure(ens, len(firsts), "moore", "torus")
    assert ens.boundary == "torus"
    ens.set_rule_tables(0, tables[0], tables[1])
    ens.upload_state(0, np.stack(firsts))
    ens.step(3)
    ens.set_boundary("closed")
    ens.step(2)
    ens.set_boundary("reference")
    ens.step(1)
    assert ens.boundary == "reference"
    got = ens.read_state()
    r = ol.Rules.from_strings(neighbourhood="moore", born="1", survive="0,2")  # grow_tables as strings
    for u, (c, w) in enumerate(zip(face_cells(), firsts)):
        mid = chain(("cell", c), w, "moore", tables, "torus")[3]
        end = Chain(mid, "moore", tables, "closed")[2]
        np.testing.assert_array_equal(got[u], ol.packed_step(G, end, r), err_msg=f"cell {c}")
    ens.set_boundary("torus")
    ens.configure(2, neighbourhood="moore")
    assert ens.boundary == "reference"  # every configure goes back to the reference


def test_refusals(ens):
    lib = _capi.load()
    out = C.c_int(7)
    assert lib.ca3d_ensemble_set_boundary(ens._h, 1) == -2 and lib.ca3d_ensemble_get_boundary(ens._h, C.byref(out)) == -2  # before configure
    assert out.value == 7
    with pytest.raises(Ca3dError) as e:
        ens.boundary
    assert e.value.code == -2
    configure(ens, 2, "moore")
    assert ens.boundary == "reference"
    assert lib.ca3d_ensemble_set_boundary(ens._h, 3) == -1 and lib.ca3d_ensemble_set_boundary(ens._h, -1) == -1  # an unknown mode
    assert ens.boundary == "reference"
    with pytest.raises(ValueError):
        ens.set_boundary("mirror")
    assert lib.ca3d_ensemble_set_boundary(None, 1) == -1 and lib.ca3d_ensemble_get_boundary(ens._h, None) == -1

    # canon_period steps with the reference boundary inside its own kernel: refused in any other mode, and nothing is touched
    alone, tables = oscillator(2)
    ens.set_rule_tables(0, tables[0], tables[1])
    ens.upload_state(0, np.stack([alone, alone]))
    ens.step(1)
    ens.synchronize()
    before = (ens.read_state().tobytes(), [(s.step, s.population, s.births, s.deaths, s.digest, s.box_min, s.box_max) for s in ens.summaries()])
    allowed = ens.canon_period([2, 2])
    for name in NEW:
        ens.set_boundary(name)
        with pytest.raises(Ca3dError) as e:
            ens.canon_period([2, 2])
        assert e.value.code == -5 and "boundary" in str(e.value), str(e.value)
        ens.census()  # what never steps is allowed in every mode
        ens.canon()
        after = (ens.read_state().tobytes(), [(s.step, s.population, s.births, s.deaths, s.digest, s.box_min, s.box_max) for s in ens.summaries()])
        assert after == before
    ens.set_boundary("reference")
    again = ens.canon_period([2, 2])
    assert again.tobytes() == allowed.tobytes()
