"""unpacked_forms.py without a GPU: the launcher's choice restated and pinned to the form table of DESIGN 4.4 and to the launch
lengths of every slab geometry test_gpu_unpacked_rule_tables.py runs; which of its rules fit the kernels' register form; and the GPU
file's own drivers on a CPU stand-in for the engine — the oracle passes them, and four stand-ins with one fault each (tables read with
`== 1`, side tables applied, a dead - face, the top plane of a Moore count dropped) fail the ids named here."""
import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol
import slab_lone as sl
import test_gpu_unpacked_rule_tables as gpu
import unpacked_forms as uf
from cellularautomatons3d_amd import LAYOUT_UNPACKED, host
from test_slab_lone_cpu import OracleEngine


# ------------------------------------------------------------------------------------------------ the form table

def test_the_form_table():
    f = uf.unpacked_form
    # literal: small grids, a grid that is no power of two, a state or a list the ballot kernel cannot take, a row too long for the LDS
    assert [f(g, g) for g in (32, 64, 96, 384, 2048)] == ["literal"] * 5
    assert f(128, 128, binary=False) == f(128, 128, fast_main=False) == f(512, 512, binary=False) == "literal"
    # ballot8 with the ballot pack and with the dwordx4 pack
    assert (f(128, 128), uf.pack_form(128)) == ("ballot8", "ballot") and (f(256, 256), uf.pack_form(256)) == ("ballot8", "dwordx4 x1")
    # below 512 no range is long enough for 16-plane tiles: 8 * 16 tiles at 256^3 against the 512 the launcher asks for
    assert {f(g, n) for g in (128, 256) for n in range(1, g + 1)} == {"ballot8"}
    # 512: 32-plane tiles for the full grid alone; 16-plane tiles from 497 planes on; 8 below
    assert f(512, 512) == "pipe32" and uf.pack_form(512) == "dwordx4 x2"
    assert {n for n in range(1, 513) if f(512, n) == "pipe16"} == set(range(497, 512))
    assert {f(512, n) for n in range(1, 497)} == {"pipe8"}
    # 1024: the 32-plane image does not fit; 16-plane tiles from 241 planes on; rows of four loads
    assert f(1024, 1024) == "pipe16" and f(1024, 240) == "pipe8" and f(1024, 241) == "pipe16" and uf.pack_form(1024) == "dwordx4 x4"
    assert set(uf.FORMS) >= {f(g, n) for g in (128, 256, 512, 1024) for n in (1, 8, 31, 32, 256, g)}


def test_the_launch_lengths_of_the_slab_geometries():
    """sl.launches of every geometry of the GPU file, and the forms they take."""
    z0, nz, K, batches = gpu.PIPE16
    assert sl.launches(nz, K, batches, False, False) == [(506,), (504,), (502,), (500,), (506,), (504,), (502,)]
    assert set(uf.run_forms(512, sl.launches(nz, K, batches, False, False))) == {"pipe16"}
    phased = sl.launches(nz, K, batches, False, True)
    assert phased[:4] == [(10, 10), (8, 8), (6, 6), (4, 4)] and phased[4:8] == [(486,), (488,), (490,), (492,)]
    assert set(uf.run_forms(512, phased)) == {"pipe8"}
    assert sl.ring_geometries(512) == [(1, 21, 3, (3, 2)), (491, 21, 4, (2, 4)), (17, 21, 2, (2, 1))]
    assert sl.launches(21, 3, (3, 2), False, False) == [(25,), (23,), (21,), (25,), (23,)]
    assert sl.launches(21, 4, (2, 4), False, False) == [(27,), (25,), (27,), (25,), (23,), (21,)]
    assert sl.launches(21, 2, (2, 1), False, False) == [(23,), (21,), (23,)]
    for z0, nz, K, batches in sl.ring_geometries(512) + [gpu.THIN_1024]:
        for ph in (False, True):
            lens = sl.launches(nz, K, batches, False, ph)
            assert sum(len(t) for t in lens) >= sum(batches)
            assert set(uf.run_forms(512, lens)) == set(uf.run_forms(1024, lens)) == {"pipe8"}
    z0, nz, K, batches = gpu.THIN_1024
    assert sl.launches(nz, K, batches, False, False) == [(25,), (23,), (21,), (25,), (23,)] and (nz + 2 * K) * 4 * 1024 * 1024 < 120 << 20


def test_the_knobs_are_looked_for():
    assert uf.knobs_set({"HOME": "/", "CA3D_JIT_CACHE": "0"}) == []
    assert uf.knobs_set({"CA3D_UNPACKED_TZ": "16", "CA3D_UNPACKED_LOADS": "0"}) == ["CA3D_UNPACKED_TZ", "CA3D_UNPACKED_LOADS"]
    assert uf.knobs_set() == [k for k in uf.KNOBS if k in uf.os.environ]


# ------------------------------------------------------------------------------------------------ cube counts

def test_which_rules_fit_the_register_form():
    """kFastCubes = 2. Every coded rule is one cube (a bit of the count, or its complement). Count parity has no cover of two cubes in
    either polarity over the Moore, edges, corners, von Neumann and in-plane Moore tables, so those launches run FAST = false; over the
    in-plane von Neumann table (counts 0 .. 4, don't-cares 5 .. 7) EVERY table fits — one of a table and its complement has two
    counts or fewer — so that neighbourhood has no FAST = false launch to test."""
    for c in uf.U_FULL + uf.U_SHORT:
        N = gl.TABLES[c.kind]
        assert uf.min_cubes(c.rule.born, N) == uf.min_cubes(c.rule.survive, N) == 1, c.id
    for c in uf.U_CUBES:
        assert uf.fits_fast(c.rule, gl.TABLES[c.kind]) == (c.kind == "vn 2D"), c.id
    assert all(uf.min_cubes(m, 5) <= 2 for m in range(32))
    N = 27
    assert uf.min_cubes(uf.parity_rule(N).born, N) > 4 and uf.min_cubes(uf.parity_rule(N).survive, N) > 4
    few = uf.FEW_CUBES
    assert (uf.min_cubes(few.born, N), uf.min_cubes(few.survive, N)) == (3, 4)
    # by hand: B3 alone is the cube 00011; B3,4 differ in three bits and need two; with the don't-care 31, S23,27 share 1-011
    assert [uf.min_cubes(m, N) for m in (1 << 3, 1 << 3 | 1 << 4, 1 << 23 | 1 << 27, (1 << 27) - 2)] == [1, 2, 1, 1]


# ------------------------------------------------------------------------------------------------ a stand-in for the engine

class _Info:
    def __init__(self, name, step):
        self.kernel_name, self.step = name, step


class StandIn(OracleEngine):
    """The Engine methods the GPU file's drivers call, computed by the oracle: full grids here, slabs as tests/test_slab_lone_cpu.py has
    them. The kernel's name follows unpacked_forms.unpacked_form. `step_cells` is what a faulty stand-in replaces."""

    slab = False

    def configure(self, G, layout=LAYOUT_UNPACKED):
        assert layout == LAYOUT_UNPACKED
        self.G, self.slab, self.variant, self.binary, self.nsteps, self.name = G, False, 0, False, 0, b"ca_unpacked"

    def configure_slab(self, G, z0, nz, K, layout=LAYOUT_UNPACKED):
        super().configure_slab(G, z0, nz, K, layout)
        self.slab, self.variant, self.binary, self.name = True, 0, True, b"ca_unpacked"

    def set_option(self, name, value):
        if name == "variant":
            self.variant = value

    def set_rules(self, main, edges, corners, survive, born):
        super().set_rules(main, edges, corners, survive, born)
        named = [np.asarray(v, dtype=np.int32).reshape(-1, 3) for v in host.NEIGHBOURHOOD_MAP.values()]
        m = self.rules.main.reshape(-1, 3)
        self.fast_main = any(len(m) == len(v) and {tuple(t) for t in m} == {tuple(t) for t in v} for v in named)

    def upload_state(self, words):
        if self.slab:
            return super().upload_state(words)
        self.state = np.array(words, dtype=np.uint32)
        self.binary, self.nsteps = bool(self.state.max() <= 1), 0

    def read_state(self):
        return super().read_state() if self.slab else self.state.copy()

    def step_cells(self, state):
        return ol.unpacked_step(self.G, state, self.rules.main, self.rules.survive, self.rules.born)

    def step(self, n):
        for _ in range(n):
            self.name = uf.kernel_of(uf.unpacked_form(self.G, self.G, self.binary and self.variant == 0, self.fast_main))
            self.state, self.binary = self.step_cells(self.state), True
        self.nsteps += n

    def slab_step(self, n):
        super().slab_step(n)
        self.name = uf.BALLOT

    def slab_step_phase(self, n, phase):
        super().slab_step_phase(n, phase)
        self.name = uf.BALLOT

    def info(self):
        return _Info(self.name, self.steps if self.slab else self.nsteps)


def _case(family, cid):
    return next(c for c in family if c.id == cid)


def test_the_drivers_on_the_oracle():
    """What the GPU file expects of an engine follows from the oracle alone: its drivers pass on the stand-in — full grids at the
    literal grids, the lone slabs (both kinds) at 128, where unpacked_form is asked for the forms of 128."""
    eng = StandIn()
    for cid in ("moore-bit4-born", "vn2d-bit2-survive"):
        gpu.test_literal_kernel(eng, 32, _case(uf.U_FULL, cid))
    gpu.test_literal_kernel_where_the_grid_is_no_torus(eng, _case(uf.U_SHORT, "edges-bit3-born"))
    gpu.test_a_table_entry_counts_when_it_is_greater_than_zero(eng, 64, "literal")
    gpu.test_raw_sums_and_the_clamp_at_slot_80(eng, 64)
    case = uf.U_CUBES[0]
    for geometry in sl.ring_geometries(128)[:2]:
        for phased in (False, True):
            uf.slab_case(eng, 128, case, geometry, phased, {"ballot8"})
    for phased in (False, True):
        uf.slab_planes_case(eng, 128, case, (40, 21, 3, (3, 2)), phased, {"ballot8"})


def test_the_plane_array_states_are_the_full_grids():
    """slab_lone.wide_states against full-grid oracle steps: a plane array cut from a full 64^3 state steps as the grid does on the planes
    that are still right."""
    g, K, nz = 64, 3, 21
    case = _case(uf.U_SHORT, "moore-bit3-born")
    r = uf.rules_of(case)
    full = [uf.first_state(g, "x")]
    for _ in range(K):
        full.append(ol.unpacked_step(g, full[-1], r.main, r.survive, r.born))
    W, z_first, pw = nz + 4 * K, 7, g * g
    states = sl.wide_states(g, full[0][z_first * pw:(z_first + W) * pw], r, K)
    for s in range(K + 1):
        np.testing.assert_array_equal(states[s][s * pw:(W - s) * pw], full[s][(z_first + s) * pw:(z_first + W - s) * pw])


# ------------------------------------------------------------------------------------------------ faults the GPU file must notice

KEYS = {26: "T", 6: "F", 12: "E", 8: "C", 4: "F2"}


class NumpyStandIn(StandIn):
    """The step from graded_lib's counts and the tables (0 / 1 states, named main lists), with one fault switched on at a time."""

    fault = None

    def step_cells(self, state):
        G, r = self.G, self.rules
        cells = state.reshape(G, G, G).astype(np.uint8)
        n_main = r.main.size // 3
        key = KEYS[n_main] if n_main != 8 else ("M2" if not r.main.reshape(-1, 3)[:, 2].any() else "C")
        n = gl.counts_of_cells(cells, torus=self.fault != "dead face")
        count = n[key] & 15 if self.fault == "top plane" and key == "T" else n[key]
        on = (lambda t: t == 1) if self.fault == "== 1" else (lambda t: t > 0)
        out = np.where(cells == 1, on(r.survive[:27])[count], on(r.born[:27])[count])
        if self.fault == "side tables":
            for s, k in ((1, "E"), (2, "C")):
                out = out | np.where(cells == 1, on(r.survive[27 * s:27 * s + 27])[n[k]], on(r.born[27 * s:27 * s + 27])[n[k]])
        return out.astype(np.uint32).ravel()


def _numpy(fault=None):
    e = NumpyStandIn()
    e.fault = fault
    return e


def test_the_numpy_stand_in_is_the_oracle():
    for c in uf.U_FULL[::5] + uf.U_CUBES:
        gpu.test_literal_kernel(_numpy(), 32, c)
    gpu.test_a_table_entry_counts_when_it_is_greater_than_zero(_numpy(), 64, "literal")
    gpu.test_the_side_tables_are_ignored(_numpy())


FAULTS = {
    "== 1": lambda e: gpu.test_a_table_entry_counts_when_it_is_greater_than_zero(e, 64, "literal"),
    "side tables": gpu.test_the_side_tables_are_ignored,
    "dead face": lambda e: gpu.test_literal_kernel(e, 32, _case(uf.U_FULL, "vn-bit0-born")),
    "top plane": lambda e: gpu.test_literal_kernel(e, 32, _case(uf.U_FULL, "moore-bit4-born")),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_fault_is_noticed(fault):
    """Each fault fails the id named in FAULTS (and the message says which classes of cells were answered wrongly)."""
    with pytest.raises(pytest.fail.Exception, match=r"\(alive, F, E, C, T\) x cells"):
        FAULTS[fault](_numpy(fault))


def test_a_dead_face_is_noticed_on_every_axis():
    """... by the same von Neumann rule: a stand-in with dead - faces differs from the oracle on the first plane, row and column alone,
    and on the inside of each of the three, whichever axis the state is graded along."""
    case = _case(uf.U_FULL, "vn-bit0-born")
    for name in ("z", "y", "x"):
        e = _numpy("dead face")
        e.configure(32)
        r = uf.rules_of(case)
        e.set_rules(r.main, r.edges, r.corners, r.survive, r.born)
        e.upload_state(uf.first_state(32, name))
        e.step(1)
        bad = (e.read_state() != uf.trajectory(32, name, case)(1)).reshape(32, 32, 32)
        assert not bad[1:, 1:, 1:].any() and bad[0, 1:, 1:].any() and bad[1:, 0, 1:].any() and bad[1:, 1:, 0].any(), name
