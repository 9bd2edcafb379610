"""The per-step kernels on slab plane ranges of any length and offset: one engine stands for one rank, the oracle's full-grid states
play its neighbours (tests/slab_lone.py; the same code drives a CPU stand-in in tests/test_slab_lone_cpu.py).

Full-grid tests give every kernel the range [0, G) with wrap_full = 1, and tests/test_gpu_slab.py splits evenly: the shifted last z-run,
the fall-throughs of ranges shorter than a form's planes per thread, two ranges per launch, a plane array whose global plane 0 lies
inside it — each kernel family meets them here, forced where the launcher would not choose the form by itself. Which form a launch takes
is not asked of the engine: the kernel family is `info().kernel_name`, the depth follows from the launcher's own arithmetic
(ca_packed.hip, launch_packed_step), restated below and asserted on the range lengths `slab.batch_ranges` gives, so that a later change
of geometry cannot quietly turn a deep-form case into a flat-form one."""
import pytest

import slab_lone as sl
from cellularautomatons3d_amd import LAYOUT_PACKED32, LAYOUT_UNPACKED
from gpu_common import rules

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _sweep(eng, G, name, geometries, seed, densities=(0, 2), options=(), layout=LAYOUT_PACKED32, max_value=1, kernel=None, family=None):
    """Every geometry, whole and phased, from a dense start state and one with and_rounds = 2 (`densities` "alternate": geometry i
    takes one of the two); `kernel`: what info().kernel_name must be after a run, `family`: what it must contain."""
    r = rules(name)
    for i, (z0, nz, K, batches) in enumerate(geometries):
        for rounds in ((0, 2)[i % 2],) if densities == "alternate" else densities:
            traj = sl.trajectory(G, name, r, seed=seed + rounds, and_rounds=rounds, layout=layout, max_value=max_value)
            for phased in (False, True):
                sl.run_lone_slab(eng, traj, r, z0, nz, K, batches, phased, layout=layout, options=options)
                got = eng.info().kernel_name
                assert (kernel is None or got == kernel) and (family is None or family in got), got


def _all_launches(geometries, phased, packed=True):
    out = []
    for z0, nz, K, batches in geometries:
        out += sl.launches(nz, K, batches, packed and z0 == 0, phased)
    return out


def _residues(lens_list, Z):
    return sorted({n % Z for lens in lens_list for n in lens})


# ------------------------------------------------------------------------------------------------------------ rows kernel
def _rows_bpp(G):
    C = G // 32
    R = 1 if C >= 64 else 64 // C
    return ((G + R - 1) // R + 3) // 4  # 256-thread blocks per plane


def _rows_zrun(G):
    """Planes per thread of the rows kernel's deep entry (ca_jit.cpp, jit_rows_kernels): the deepest run that fills the chip."""
    for z in (8, 6, 4, 3, 2):
        if _rows_bpp(G) * ((G + z - 1) // z) >= 1024:
            return z
    return 2


def _rows_deep(G, lens):
    """The launcher's choice (launch_packed_step): the deep entry only while every range holds a run and the launch fills the chip."""
    Z = _rows_zrun(G)
    return min(lens) >= Z and _rows_bpp(G) * (sum(lens) // Z) >= 1024


def _dead_face_positions(geometries, Z, takes):
    """Positions 0 .. Z-1 inside a z-run of Z planes at which the whole form computes the first high ghost plane of a top slab — the copy
    of global plane 0, whose z-1 face is dead although the plane below it is there — counted only where a wrong word must show: in
    launches that take the form (`takes(range lengths)`), before the last sub-step of a batch (the owned plane below reads it in the next
    one) and outside the planes the shifted last run computes a second time."""
    out = set()
    for z0, nz, K, batches in geometries:
        p = K + nz  # (the plane is the copy of plane 0 only where the slab ends at plane G: the caller passes top slabs)
        for n in batches:
            for s in range(1, n):
                lo, hi = sl.slab.batch_ranges(nz, K, n, s, z0 == 0)["all"]
                if takes((hi - lo,)) and lo <= p < hi - Z:
                    out.add((p - lo) % Z)
    return sorted(out)


def _top_slabs(G, geometries):
    return [g for g in geometries if g[0] + g[1] == G]


ROWS_FLAT_RULES = ["default", "clustered", "life2d", "vn_edges_only"]


@pytest.mark.parametrize("name", ROWS_FLAT_RULES)
@pytest.mark.parametrize("G", [96, 160, 224])
def test_rows_kernel_flat_form_on_slabs(eng, G, name):
    """ca_packed_rows_kernel.inc serves every grid with G % 128 != 0; no slab of such a grid was ever run. 3, 5 and 7 words per row (21,
    12 and 9 rows per wave, 63, 60 and 63 active lanes); the 2D rule never reads another plane (kZNbr == false)."""
    geometries = sl.even_split_geometries(G)
    assert not any(_rows_deep(G, lens) for ph in (False, True) for lens in _all_launches(geometries, ph))  # these grids never fill the chip
    _sweep(eng, G, name, geometries, seed=G, kernel=b"ca_packed_rows(jit)")


@pytest.mark.parametrize("name", ROWS_FLAT_RULES)
@pytest.mark.parametrize("G", [96, 160, 224])
def test_rows_kernel_flat_form_on_slabs_no_even_split_produces(eng, G, name):
    """A high ghost that straddles plane G, and 0 < z0 < K: global plane 0 sits inside the low ghost, the planes below it hold all ones."""
    _sweep(eng, G, name, sl.uneven_split_geometries(G), seed=G + 1, kernel=b"ca_packed_rows(jit)")


@pytest.mark.parametrize("name", ["default", "clustered"])
@pytest.mark.parametrize("G,ZR", [(288, 3), (320, 4), (352, 6), (480, 8)])
def test_rows_kernel_deep_form_at_each_compiled_depth(eng, G, ZR, name):
    """The deep entry is compiled with 3, 4, 6 and 8 planes per thread at 288, 320, 352 and from 416 up; it is taken only by launches of
    about 282, 296, 342 and 280 planes at these four grids: nearly whole grids. Range lengths that are no multiple of ZR run the shifted
    last z-run (`j0 = hi - ZR`); the phased form adds the two-range flat launches and a deep interior."""
    assert _rows_zrun(G) == ZR
    geometries = sl.nearly_whole_geometries(G)
    whole, phased = _all_launches(geometries, False), _all_launches(geometries, True)
    deep_whole = [lens for lens in whole if _rows_deep(G, lens)]
    deep_phased = [lens for lens in phased if _rows_deep(G, lens)]
    print(f"rows deep G {G} ZR {ZR}: whole launches {whole}, deep residues {_residues(deep_whole, ZR)}; phased launches {phased}, "
          f"deep residues {_residues(deep_phased, ZR)}")
    assert any(n % ZR for lens in deep_whole for n in lens), "no deep launch with a shifted last run"
    assert any(_residues([lens], ZR) == [0] for lens in deep_whole), "no deep launch of whole runs only"
    assert any(not _rows_deep(G, lens) for lens in whole), "no launch below the threshold"
    assert any(len(lens) == 1 and lens[0] % ZR for lens in deep_phased), "no deep interior with a shifted last run"
    assert any(len(lens) == 2 and not _rows_deep(G, lens) for lens in phased), "no two-range flat launch"
    assert _dead_face_positions(_top_slabs(G, geometries), ZR, lambda lens: _rows_deep(G, lens)) == list(range(ZR)), "global plane 0 does not reach every position of a deep z-run"
    _sweep(eng, G, name, geometries, seed=G, kernel=b"ca_packed_rows(jit)")


# ------------------------------------------------------------------------------------------- rolling window, whole rows per wave
@pytest.mark.parametrize("Z", [2, 4, 8])
@pytest.mark.parametrize("name", ["clustered", "edges_main"])
def test_roll_np2_forced_depths_on_slabs(eng, name, Z):
    """roll_step_np2 (rows of 3 uint4 at 384) with 2, 4 and 8 planes per thread forced: range lengths with every residue mod Z, and edge
    zones shorter than Z, which fall through to the class kernel."""
    G = 384
    geometries = sl.even_split_geometries(G)[:4] + sl.uneven_split_geometries(G) + sl.short_edge_geometries(G) + sl.deep_ghost_top_geometries(G)
    every = _all_launches(geometries, False) + _all_launches(geometries, True)
    taken = [lens for lens in every if min(lens) >= Z]
    print(f"roll np2 Z {Z}: launches {every}; residues of those the form takes {_residues(taken, Z)}; fall through {[l for l in every if min(l) < Z]}")
    assert _residues(taken, Z) == list(range(Z)), "a residue mod Z is missing"
    assert any(len(lens) == 2 for lens in taken), "no two-range launch at this depth"
    assert any(min(lens) < Z for lens in every), "no range shorter than Z"
    assert _dead_face_positions(_top_slabs(G, geometries), Z, lambda lens: min(lens) >= Z) == list(range(Z)), "global plane 0 does not reach every position of a z-run"
    try:
        _sweep(eng, G, name, geometries, seed=G + Z, densities="alternate", options=(("roll_z", Z),), kernel=b"ca_packed_roll_np2(jit)")
    finally:
        eng.set_option("roll_z", 0)


# ------------------------------------------------------------------------------------------- rolling window, power-of-two rows
ROLL_DEPTHS = {1: (2, 4, 8, 16, 15, 30), 0: (2, 4, 8, 15, 30), 2: (8, 16), 3: (8, 16)}  # as test_rolling_window_kernel_every_depth


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["clustered", "moore_wide"])
def test_rolling_window_forms_on_slabs(eng, name, tile):
    """ca_packed_roll_kernel.inc's forms (roll_tile 0: every thread shifts its rows; 1: 256-thread tiles; 2: wave tiles; 3: two words per
    thread) at every depth they are compiled for, the looped 15 / 30 included — forced so far on the full 256^3 grid only. Slabs of
    79 .. 101 array planes: odd range lengths, two-range edge launches of 8 .. 41 planes, a top slab with global plane 0 inside a run."""
    G = 256
    geometries = sl.window_geometries(G) + sl.deep_ghost_top_geometries(G)
    every = _all_launches(geometries, False) + _all_launches(geometries, True)
    try:
        for Z in ROLL_DEPTHS[tile]:
            taken = [lens for lens in every if min(lens) >= Z]
            print(f"roll tile {tile} Z {Z}: residues {_residues(taken, Z)}, two-range launches {[l for l in taken if len(l) == 2]}")
            assert any(n % Z for lens in taken for n in lens) and any(len(lens) == 2 for lens in taken)
            at = _dead_face_positions(_top_slabs(G, geometries), Z, lambda lens: min(lens) >= Z)
            print(f"roll tile {tile} Z {Z}: global plane 0 at positions {at} of a run")
            assert Z > 8 or at == list(range(Z))  # (ghost zones deep enough for every position of 15 .. 30 planes would make slabs of 150 planes)
            _sweep(eng, G, name, geometries, seed=G + tile, densities="alternate",
                   options=(("resident", 0), ("roll_tile", tile), ("roll_z", Z)), family=b"roll")
    finally:
        eng.set_option("roll_z", 0)
        eng.set_option("roll_tile", 1)
        eng.set_option("resident", 1)


# --------------------------------------------------------------------------------------------------- class, vn, generic kernels
@pytest.mark.parametrize("name", ["default", "clustered", "life2d", "vn2d", "edges_main"])
def test_class_kernels_on_slabs(eng, name):
    """The class kernels at 128^3, run-time compiled for the rule and pre-built (`jit` 0 never ran on a slab): one slab whose z0, K and
    nz are multiples of 4, three that are not."""
    G = 128
    try:
        for jit in (1, 0):
            _sweep(eng, G, name, sl.aligned_and_not_geometries(G), seed=G + jit, options=(("jit", jit),), family=b"ca_packed_class")
            assert (b"(jit)" in eng.info().kernel_name) == bool(jit)
    finally:
        eng.set_option("jit", 1)


@pytest.mark.parametrize("name", ["default", "vn_b24_s135"])
def test_vn_kernel_on_slabs(eng, name):
    """ca_packed_vn at 256^3: the start-up rule's pre-built tables, another table pair compiled at run time, then through the pre-built
    kernel's run-time tables (`jit` 0)."""
    G = 256
    try:
        for jit in (1, 0):
            _sweep(eng, G, name, sl.aligned_and_not_geometries(G), seed=G + jit, options=(("jit", jit),), family=b"ca_packed_vn")
            assert (b"(jit)" in eng.info().kernel_name) == (bool(jit) and name != "default")
    finally:
        eng.set_option("jit", 1)


@pytest.mark.parametrize("name", ["default", "clustered"])
@pytest.mark.parametrize("G", [96, 128])
def test_generic_kernel_on_slabs(eng, G, name):
    """`variant` 1: the generic kernel takes one range per launch, so the phased form's two-range launches are split in two."""
    geometries = sl.even_split_geometries(G)[:4] + sl.uneven_split_geometries(G)
    assert any(len(lens) == 2 for lens in _all_launches(geometries, True))
    try:
        _sweep(eng, G, name, geometries, seed=G + 7, densities="alternate", options=(("variant", 1),), kernel=b"ca_packed_generic")
    finally:
        eng.set_option("variant", 0)


# ------------------------------------------------------------------------------------------------------------ unpacked layout
@pytest.mark.parametrize("max_value", [1, 2])
@pytest.mark.parametrize("G", [64, 128])
def test_unpacked_kernels_on_slabs(eng, G, max_value):
    """One u32 per cell: a torus, both ghosts filled, no dead face. 0 / 1 states take the ballot kernel from 128 up; a state with cells of
    value 2 takes the literal kernel for its first sub-step (and 64^3 always does)."""
    _sweep(eng, G, "default", sl.ring_geometries(G), seed=G, densities=(0,), layout=LAYOUT_UNPACKED, max_value=max_value,
           kernel=b"ca_unpacked_ballot" if G >= 128 else b"ca_unpacked_literal")
