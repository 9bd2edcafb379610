"""Rule tables bit by bit on every form of the one-u32-per-cell step (ca_unpacked.hip): the literal kernel, the ballot kernel with its
ballot and its dwordx4 pack, and the pipelined kernel on tiles of 32, 16 and 8 planes with two and four loads a row. The random fills of
test_gpu_unpacked.py / test_gpu_slab*.py never hold a dead cell with 24 live Moore neighbours; here every form meets graded states
(graded_lib.unpacked_state: every (alive, count) pair of every table under torus counts, test_graded_cpu.py shows it at these grids)
under coded rules that answer any two counts differently, and under programs too long for the kernels' register form (FAST = false).

One rule per test id. Every id asserts the launcher's form — from unpacked_forms.unpacked_form, on the plane count of every launch of
its run: the engine calls both the plain and the pipelined ballot kernel `ca_unpacked_ballot` — and the name the engine reports, takes
two single steps from each start state (the second from the ping-pong buffer) or whole slab batches, and compares with
oracle_lib.unpacked_step exactly; a difference names form, grid, rule, start state and the (alive, F, E, C, T) classes answered wrongly.

Families (unpacked_forms.py). U_FULL: the coded rules of all six main neighbourhoods (46). U_SHORT: born and survive of the two highest
coded bits of the Moore, edges and corners tables (12). U_CUBES: count parity over each main neighbourhood — no cover of two cubes exists
for either polarity of these tables except the in-plane von Neumann one, which has none that long (test_unpacked_forms_cpu.py) — and a
Moore rule of three and four cubes (7).

The lone slabs at 512 take their planes and ghosts from the oracle's full-grid states (slab_lone.run_lone_slab); the one at 1024, where
a state is 4 GiB, from a graded plane array (run_lone_slab_planes). The ids of one rule at 512 follow each other and share its oracle
states (unpacked_forms.trajectory).

Measured per id on an MI355X host (almost all of it the CPU oracle; the whole file: 364 ids in 143 s): 32 .. 128 at most 0.1 s;
256^3 at most 0.8 s; 512^3 full grid (both start states) at most 4.7 s and the 500-plane slab, which extends the rule's states to
step 7, 4.5 s (Moore; 2.5 s and less for the other tables); a thin slab at 512 0.1 s; the slab at 1024 0.5 s; the 130-step batch
1.7 s. No 512^3 id comes near 15 s, so each keeps both start states."""
import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol
import slab_lone as sl
import unpacked_forms as uf
from cellularautomatons3d_amd import LAYOUT_UNPACKED, Ca3dError, host
from gpu_common import set_rules
from rule_tables_common import ids
from unpacked_forms import BALLOT, LITERAL, U_CUBES, U_FULL, U_SHORT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cellularautomatons3d_amd import Engine

    if uf.knobs_set():
        pytest.skip(f"{uf.knobs_set()} set: the launcher's tuning knobs choose other forms than unpacked_forms.unpacked_form restates")
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ the literal kernel

@pytest.mark.parametrize("case", U_FULL + U_CUBES, ids=ids(U_FULL + U_CUBES))
@pytest.mark.parametrize("g", [32, 64])
def test_literal_kernel(eng, g, case):
    """Grids below 128 never take the ballot kernel: one thread a cell, 26 loads, the tables as bit masks of `> 0`."""
    uf.full_case(eng, g, case, ("z", "x", "zr") + (("y",) if case.kind in uf.FLAT_KINDS else ()), "literal")


@pytest.mark.parametrize("case", U_SHORT, ids=ids(U_SHORT))
def test_literal_kernel_where_the_grid_is_no_torus(eng, case):
    """96 is no power of two: coordinate -1 arrives as 0xFFFFFFFF % 96 = 63, not 95 (compute.wgsl:27). The oracle alone says what is
    right there: the torus counts of graded_lib do not apply."""
    uf.full_case(eng, 96, case, ("z", "x", "zr"), "literal", classes=False)


@pytest.mark.parametrize("case", U_SHORT, ids=ids(U_SHORT))
def test_literal_kernel_at_128_by_option(eng, case):
    uf.full_case(eng, 128, case, uf.starts_of(case), "literal", variant=1)


# ------------------------------------------------------------------------------------------------ the ballot kernel

@pytest.mark.parametrize("case", U_FULL + U_CUBES, ids=ids(U_FULL + U_CUBES))
@pytest.mark.parametrize("g", [128, 256])
def test_ballot_kernel(eng, g, case):
    """Tiles of 8 planes. 128^3: rows of four words packed with __ballot (X256 == 0); 256^3: one dwordx4 load a lane and row, eight rows
    in flight a wave, nibbles gathered over DPP."""
    assert uf.pack_form(g) == {128: "ballot", 256: "dwordx4 x1"}[g]
    uf.full_case(eng, g, case, uf.starts_of(case), "ballot8")


def test_a_batch_long_enough_for_graph_replay(eng):
    """130 steps in one call at 128^3 (graph_min is 128: the batch replays as a captured graph) under the Moore table's top coded bit."""
    g, n = 128, 130
    case = next(c for c in U_SHORT if c.id == "moore-bit4-born")
    r = uf.rules_of(case)
    eng.configure(g, LAYOUT_UNPACKED)
    set_rules(eng, r)
    cur = uf.first_state(g, "z")
    eng.upload_state(cur)
    eng.step(n)
    assert eng.info().kernel_name == BALLOT and eng.info().step == n
    for _ in range(n):
        before, cur = cur, ol.unpacked_step(g, cur, r.main, r.survive, r.born)
    assert cur.any() and not np.array_equal(cur, before)
    uf.rc.settle([uf.differs(g, eng.read_state(), cur, before, f"{n} steps in one batch from graded z at {g}^3")])


# ------------------------------------------------------------------------------------------------ the pipelined kernel at 512

PIPE16 = (6, 500, 4, (4, 3))     # every whole sub-step has 506 .. 500 planes: 16 * ceil(L / 16) >= 512 and L != 512; the last tile is partial
FORMS_512 = ["pipe32", "pipe16"] + [f"pipe8-{i}" for i in range(3)]


def at_512(eng, case, form, phased=False):
    g = 512
    if form == "pipe32":
        return uf.full_case(eng, g, case, ("z", "x"), "pipe32")
    if form == "pipe16":
        # (phased, its edge zones are a few planes and its interior 486 .. 492: under 497, tiles of 8)
        return uf.slab_case(eng, g, case, PIPE16, phased, {"pipe8"} if phased else {"pipe16"})
    return uf.slab_case(eng, g, case, sl.ring_geometries(g)[int(form[-1])], phased, {"pipe8"})


# one rule after the other, so that a rule's ids share its oracle states; the Moore parity rule (the interpreted program, every count
# answered) also takes one phased run per geometry
RUNS_512 = [(c, f, ph) for c in U_SHORT + U_CUBES for f, ph in [(f, False) for f in FORMS_512] + [(f, True) for f in FORMS_512[1:] if c is U_CUBES[0]]]


@pytest.mark.parametrize("case,form,phased", RUNS_512, ids=[f"{c.id}-{f}{'-phased' if ph else ''}" for c, f, ph in RUNS_512])
def test_pipelined_kernel_at_512(eng, case, form, phased):
    """pipe32: the full grid. pipe16: a lone slab of 500 planes. pipe8, two dwordx4 loads a row: thin lone slabs whose ghosts wrap below
    plane 0 and past plane 511 (slab_lone.ring_geometries). Whole batches from the state graded along x: every plane holds every count."""
    at_512(eng, case, form, phased)


# ------------------------------------------------------------------------------------------------ the pipelined kernel at 1024

THIN_1024 = (300, 21, 3, (3, 2))  # a plane array of 27 planes, 108 MiB a buffer


@pytest.mark.parametrize("case", U_SHORT + U_CUBES, ids=ids(U_SHORT + U_CUBES))
def test_pipelined_kernel_at_1024(eng, case):
    """pipe8 with four dwordx4 loads a row (X256 == 4: rows of 1024 only)."""
    assert uf.pack_form(1024) == "dwordx4 x4"
    uf.slab_planes_case(eng, 1024, case, THIN_1024, False, {"pipe8"})


def test_pipelined_kernel_at_1024_phased(eng):
    uf.slab_planes_case(eng, 1024, U_CUBES[0], THIN_1024, True, {"pipe8"})


# ------------------------------------------------------------------------------------------------ what only this layout does

def _with_values(table, values=(2, 0xFFFFFFFF)):
    """The table with other values > 0 where it has 1, taken in turn."""
    out = table.copy()
    at = np.flatnonzero(table == 1)
    out[at] = np.resize(np.array(values, dtype=np.uint32), at.size)
    return out


@pytest.mark.parametrize("g,form", [(64, "literal"), (128, "ballot8")])
def test_a_table_entry_counts_when_it_is_greater_than_zero(eng, g, form):
    """compute.wgsl:160-166 tests `> 0` where the packed kernel tests `== 1` (compute_clustered.wgsl:232): entries of 2 and 0xFFFFFFFF
    give what entries of 1 give — and the packed layout, shown once on the CPU, treats the same arrays as empty tables."""
    case = next(c for c in U_FULL if c.id == "moore-bit2-born")
    r1 = uf.rules_of(case)
    r = ol.Rules(r1.main, r1.edges, r1.corners, _with_values(r1.survive), _with_values(r1.born))
    assert set(r.born[r1.born == 1].tolist()) == {2, 0xFFFFFFFF} and (r.born != 0).tolist() == (r1.born != 0).tolist()
    if g == 64:
        st = gl.graded_state(g, "z")
        silent = ol.Rules(r1.main, r1.edges, r1.corners, np.zeros_like(r1.survive), np.zeros_like(r1.born))
        np.testing.assert_array_equal(ol.packed_step(g, st, r), ol.packed_step(g, st, silent))
        assert not np.array_equal(ol.packed_step(g, st, r1), ol.packed_step(g, st, silent))
        u = uf.first_state(g, "z")
        np.testing.assert_array_equal(ol.unpacked_step(g, u, r.main, r.survive, r.born), ol.unpacked_step(g, u, r1.main, r1.survive, r1.born))
    uf.full_case(eng, g, case, ("z", "x"), form, r=r)


def test_the_side_tables_are_ignored(eng):
    """One rule-set: a von Neumann rule whose edges and corners tables fire (the packed oracle shows that they do) steps as the same rule
    with silent side tables."""
    g = 128
    case = next(c for c in U_FULL if c.id == "vn-bit1-born")
    e, c = gl.coded(13)[3], gl.coded(9)[7]
    kw = dict(gl.strings_of(case.kind, case.rule), born_edges=e.born_str, survive_edges=e.survive_str, born_corners=c.born_str, survive_corners=c.survive_str)
    r = ol.Rules.from_strings(**kw)
    assert r.born[27:].any() and r.survive[27:].any()
    st = gl.graded_state(g, "x")
    assert not np.array_equal(ol.packed_step(g, st, r), ol.packed_step(g, st, uf.rules_of(case)))
    uf.full_case(eng, g, case, ("z", "x"), "ballot8", r=r)


def roll_count(cells, offs):
    """The count of a torus by definition: the cells at every offset (x, y, z triples) of the list added up, duplicates and all."""
    return sum(np.roll(cells, (-dz, -dy, -dx), axis=(0, 1, 2)).astype(np.int32) for dx, dy, dz in np.asarray(offs).reshape(-1, 3))


def _lists():
    moore = np.asarray(host.NEIGHBOURHOOD_MAP["moore"], dtype=np.int32).reshape(-1, 3)
    vn = np.asarray(host.NEIGHBOURHOOD_MAP["von neumann"], dtype=np.int32).reshape(-1, 3)
    twice = moore.copy()
    twice[int(np.flatnonzero((moore == (-1, -1, -1)).all(1))[0])] = (1, 1, 1)  # 26 triples: (1, 1, 1) twice, (-1, -1, -1) not at all
    return moore, {"moore-one-offset-twice": twice, "vn-and-the-own-cell": np.concatenate([vn, [[0, 0, 0]]]).astype(np.int32)}


def test_a_list_longer_than_the_table_is_refused(eng):
    """The Moore list with one offset doubled is 27 triples: a count of 27 would leave the rule-set's 27 table slots, the engine says so."""
    moore, _ = _lists()
    r = ol.Rules.from_strings("moore", "1", "1")
    eng.configure(128, LAYOUT_UNPACKED)
    with pytest.raises(Ca3dError):
        eng.set_rules(np.concatenate([moore, moore[:1]]).ravel(), r.edges, r.corners, r.survive, r.born)


@pytest.mark.parametrize("which", ["moore-one-offset-twice", "vn-and-the-own-cell"])
def test_a_list_that_is_no_named_class_takes_the_literal_kernel(eng, which):
    """A 0 / 1 state at 128^3 would take the ballot kernel; a main list with a duplicate or with (0, 0, 0) is no named class
    (rules.cpp:194-201) and keeps the literal kernel, whose count includes the duplicate / the own cell."""
    g = 128
    offs = _lists()[1][which]
    odd = "1,3,5,7,9,11,13,15,17,19,21,23,25"
    r0 = ol.Rules.from_strings("moore", odd, "0," + odd)
    r = ol.Rules(offs.ravel(), r0.edges, r0.corners, r0.survive, r0.born)
    assert uf.unpacked_form(g, g, fast_main=False) == "literal" and uf.unpacked_form(g, g) == "ballot8"
    eng.configure(g, LAYOUT_UNPACKED)
    set_rules(eng, r)
    lines = []
    for name in ("z", "x"):
        s0 = uf.first_state(g, name)
        cells = s0.reshape(g, g, g)
        count = roll_count(cells, offs)
        named = roll_count(cells, host.NEIGHBOURHOOD_MAP["moore" if which.startswith("moore") else "von neumann"])
        assert (count != named).any()
        s1 = ol.unpacked_step(g, s0, r.main, r.survive, r.born)
        np.testing.assert_array_equal(s1.reshape(g, g, g), np.where(cells == 1, r.survive[count], r.born[count]))  # the oracle counts them too
        assert not np.array_equal(s1.reshape(g, g, g), np.where(cells == 1, r.survive[named], r.born[named]))      # ... and it matters
        s2 = ol.unpacked_step(g, s1, r.main, r.survive, r.born)
        eng.upload_state(s0)
        for step, (want, before) in enumerate(((s1, s0), (s2, s1)), 1):
            eng.step(1)
            assert eng.info().kernel_name == LITERAL
            lines.append(uf.differs(g, eng.read_state(), want, before, f"literal: list {which}, start {name} at {g}^3, step {step}"))
    uf.rc.settle(lines)


def raw_state(g, name="z"):
    """A graded state whose live cells hold 1 .. 4: the legacy kernel adds up the raw values (compute.wgsl:42) — counts up to 104."""
    cells = uf.first_state(g, name)
    # (each bit of the extra value is set in three cells of four: sums of 81 and more are common where the state is dense)
    extra = sum((((w >> 7) | (w >> 13)) & 1).astype(np.uint32) << k for k, w in enumerate(host.random_fill(g ** 3, seed=s) for s in (601, 602)))
    return cells * (1 + extra)


def raw_rules():
    """A Moore rule over all 81 table slots: born at the odd sums and at slot 80, where every sum past it is clamped
    (ca_unpacked.hip:34), survive at the sums that are multiples of 3 but not at 80."""
    r0 = ol.Rules.from_strings("moore")
    k = np.arange(81)
    born = ((k & 1) | (k == 80)).astype(np.uint32)
    survive = ((k % 3 == 0) & (k != 80)).astype(np.uint32)
    return ol.Rules(r0.main, r0.edges, r0.corners, survive, born)


@pytest.mark.parametrize("g", [64, 128])
def test_raw_sums_and_the_clamp_at_slot_80(eng, g):
    """Live cells of 1 .. 4 under a Moore rule: sums pass 80 for dead cells, cells of 1 and cells above 1 alike (asserted), and are read at
    slot 80. The literal kernel takes the step; at 128^3 the state is 0 / 1 afterwards and the ballot kernel takes the next one."""
    r = raw_rules()
    s0 = raw_state(g)
    cells = s0.reshape(g, g, g)
    total = roll_count(cells, r.main)
    assert int(s0.max()) == 4 and int(total.max()) > 81
    assert all(int(((total >= 81) & sel).sum()) >= 16 for sel in (cells == 0, cells == 1, cells > 1))
    assert r.born[80] == 1 and r.born[78] == 0 and ((total >= 81) & (total % 2 == 0) & (cells == 0)).any()  # the clamp is not the table's pattern continued
    s1 = ol.unpacked_step(g, s0, r.main, r.survive, r.born)
    clamped = np.minimum(total, 80)
    np.testing.assert_array_equal(s1.reshape(g, g, g), np.where(cells == 1, r.survive[clamped], np.where(cells == 0, r.born[clamped], 0)))
    s2 = ol.unpacked_step(g, s1, r.main, r.survive, r.born)
    assert uf.unpacked_form(g, g, binary=False) == "literal"
    second = uf.unpacked_form(g, g)
    assert second == {64: "literal", 128: "ballot8"}[g]
    eng.configure(g, LAYOUT_UNPACKED)
    set_rules(eng, r)
    eng.upload_state(s0)
    eng.step(1)
    assert eng.info().kernel_name == LITERAL
    got1 = eng.read_state()
    eng.step(1)
    assert eng.info().kernel_name == uf.kernel_of(second)
    uf.rc.settle([uf.differs(g, got1, s1, s0, f"literal: raw sums at {g}^3, step 1"), uf.differs(g, eng.read_state(), s2, s1, f"{second}: raw sums at {g}^3, step 2")])
