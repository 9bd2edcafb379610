"""The one-u32-per-cell layout's launcher restated, and the rule families of test_gpu_unpacked_rule_tables.py — TEST INFRASTRUCTURE.

`unpacked_form` says which kernel form a launch of the unpacked step takes (ca_unpacked.hip: `ballot_applies`, lines 488-496, and
`launch_ballot_f`, lines 459-479). The engine reports two names only — both the plain and the pipelined ballot kernel are
`ca_unpacked_ballot` — so a test that wants a form asserts it from here, on the plane count of every launch of its run, and
test_unpacked_forms_cpu.py pins this function to the table of DESIGN 4.4. It holds while none of the launcher's tuning knobs is set
(`knobs_set`): those are process-wide statics read once from the environment.

`min_cubes` bounds what rules.cpp makes of a table from below without restating its Quine-McCluskey: the smallest number of cubes (sub-cubes
of the count's bit planes that avoid the off-set, don't-cares free) that cover a table or its complement. A program of more than
`kFastCubes` = 2 cubes takes the kernels' interpreting (FAST = false) instantiation (ca_unpacked.hip:484)."""
import functools
import itertools
import operator
import os

import numpy as np
import pytest

import graded_lib as gl
import rule_tables_common as rc
import slab_lone as sl
from cellularautomatons3d_amd import LAYOUT_UNPACKED
from gpu_common import set_rules
from rule_tables_common import Case, coded_cases

KNOBS = ("CA3D_UNPACKED_PIPE", "CA3D_UNPACKED_TZ", "CA3D_UNPACKED_SUB", "CA3D_UNPACKED_LOADS")
FORMS = ("literal", "ballot8", "ballot16", "pipe8", "pipe16", "pipe32")
TILE_ROWS = 32            # kBTY, ca_unpacked.hip:68
LDS_LIMIT = 160 * 1024


def knobs_set(environ=None):
    """The launcher's tuning knobs found in the environment (their non-default forms are out of scope: the GPU tests skip)."""
    return [k for k in KNOBS if k in (os.environ if environ is None else environ)]


def ballot_applies(G, binary=True, fast_main=True):
    """ca_unpacked.hip:488-496: a 0 / 1 state, a main list that is a named class, a power-of-two grid of 128 or more whose 16-plane
    tile image fits the LDS (1024 does, 2048 does not)."""
    if not binary or not fast_main:
        return False
    if G < 128 or G & (G - 1):
        return False
    return ((16 + 2) * (TILE_ROWS + 2) + 16 * TILE_ROWS) * (G // 32) * 4 <= LDS_LIMIT


def unpacked_form(G, planes, binary=True, fast_main=True):
    """The form of one launch over `planes` output planes: "literal", or the ballot kernel ("ballot8" / "ballot16") or its pipelined
    form ("pipe8" / "pipe16" / "pipe32") with that many planes a tile. ca_unpacked.hip:459-479, every knob at its default."""
    assert planes > 0
    if not ballot_applies(G, binary, fast_main):
        return "literal"
    ny = (G + TILE_ROWS - 1) // TILE_ROWS
    tiles16 = ny * ((planes + 15) // 16)                                                # :463
    lds32 = (34 * (TILE_ROWS + 2) + 2 * 8 * TILE_ROWS) * (G // 32) * 4                  # :473
    if G >= 512 and planes % 32 == 0 and ny * (planes // 32) >= 256 and lds32 <= LDS_LIMIT:   # :474
        return "pipe32"
    if G >= 512:                                                                        # :476-477
        return "pipe16" if tiles16 >= 512 else "pipe8"
    return "ballot16" if tiles16 >= 512 else "ballot8"                                  # :478


def pack_form(G):
    """How a row reaches the LDS image (ca_unpacked.hip:91-92, :454; the pipelined kernel: X256 loads a row): "ballot" below 256,
    else dwordx4 loads a lane, G / 256 of them a row."""
    return "ballot" if G < 256 else f"dwordx4 x{G // 256}"


def run_forms(G, launch_lengths, binary=True, fast_main=True):
    """The forms of a run's launches: `launch_lengths` as slab_lone.launches gives them (tuples of range lengths: the unpacked layout
    launches every range by itself, ca3d_step.cpp:36-43)."""
    return [unpacked_form(G, n, binary, fast_main) for lens in launch_lengths for n in lens]


# ------------------------------------------------------------------------------------------------ cube counts

def _cubes(nvars):
    """Every sub-cube of nvars bit planes as the mask of the counts it holds."""
    out = []
    for lits in itertools.product((0, 1, None), repeat=nvars):
        m = 0
        for k in range(1 << nvars):
            if all(l is None or (k >> i & 1) == l for i, l in enumerate(lits)):
                m |= 1 << k
        out.append(m)
    return out


def _min_cover(on, off, nvars, limit=4):
    """The fewest sub-cubes that hold every count of `on` and none of `off` (the other counts are free), or limit + 1 if more than
    `limit` are needed."""
    if not on:
        return 0
    ok = sorted({c & on for c in _cubes(nvars) if not c & off and c & on}, key=lambda c: -bin(c).count("1"))
    ok = [c for c in ok if not any(c != d and c & d == c for d in ok)]  # maximal ones are enough
    for n in range(1, limit + 1):
        if any(on == functools.reduce(operator.or_, t) for t in itertools.combinations(ok, n)):
            return n
    return limit + 1


def min_cubes(mask, N, limit=4):
    """A lower bound of the cubes of rules.cpp's program for the table `mask` over counts 0 .. N - 1 (compile_rule_prog covers the table
    or its complement, counts above N - 1 as don't-cares, lines 91-110): the smaller of the two minimal covers, capped at limit + 1."""
    nvars = (N - 1).bit_length()  # rules.cpp, bits_for(max_count): the table's list has N - 1 neighbours
    full = (1 << N) - 1
    on, off = mask & full, full & ~mask
    if not on or not off:
        return 0
    return min(_min_cover(on, off, nvars, limit), _min_cover(off, on, nvars, limit))


def fits_fast(rule, N):
    """True: both tables CAN be covered by two cubes or fewer. False: neither polarity of one of them can — whatever cover the host
    picks, the launch takes the FAST = false instantiation."""
    return min_cubes(rule.born, N, 2) <= 2 and min_cubes(rule.survive, N, 2) <= 2


# ------------------------------------------------------------------------------------------------ the families

KINDS = [("moore", "moore"), ("edges main", "edges"), ("corners main", "corners"), ("vn", "vn"), ("moore 2D", "moore2d"), ("vn 2D", "vn2d")]
FLAT_KINDS = ("moore 2D", "vn 2D")

U_FULL = [c for kind, tag in KINDS for c in coded_cases(kind, tag)]
U_SHORT = [c for kind, tag in KINDS[:3] for c in coded_cases(kind, tag, bits=2)]


def _rule(name, born, survive):
    return gl.Rule(name, born, survive, gl.mask_string(born), gl.mask_string(survive))


def parity_rule(N):
    """Born at the counts with an odd number of set bits, survive at the others: no two counts of one table share a cube unless a
    don't-care joins them — the longest programs a table of N entries can have (16 cubes over five bits: the kMaxCubes clamp's case)."""
    odd = sum(1 << c for c in range(N) if bin(c).count("1") & 1)
    return _rule("count parity, born where odd", odd, ((1 << N) - 1) & ~odd)


# a Moore rule of three born and four survive cubes: no two of its counts differ in one bit only, and none has a don't-care
# (27 .. 31) beside it that joins it to another (test_unpacked_forms_cpu.py shows both bounds)
FEW_CUBES = _rule("B3,12,21/S5,10,17,22", 1 << 3 | 1 << 12 | 1 << 21, 1 << 5 | 1 << 10 | 1 << 17 | 1 << 22)

U_CUBES = [Case(f"{tag}-parity", kind, parity_rule(gl.TABLES[kind]), True) for kind, tag in KINDS] + [Case("moore-few-cubes", "moore", FEW_CUBES, True)]
assert (len(U_FULL), len(U_SHORT), len(U_CUBES)) == (46, 12, 7)


def starts_of(case, names=("z", "x")):
    """The graded start states of a case: `names`, the reversed z for top-bit rules, y for the in-plane neighbourhoods (a state graded
    along z is uniform inside a plane)."""
    out = tuple(names)
    if case.top and "zr" not in out:
        out += ("zr",)
    if case.kind in FLAT_KINDS and "y" not in out:
        out += ("y",)
    return out


# ------------------------------------------------------------------------------------------------ the wording of a failure

def differs(g, got, want, before, what, planes=None):
    """rule_tables_common.differs for one-u32-per-cell states with torus counts: None when got == want, else which (alive, F, E, C, T)
    cells of `before` were answered wrongly. `planes`: the arrays are that many planes of g x g cells, the first and last not compared
    (a slab's plane array: no z wrap inside)."""
    got, want = np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32)
    if np.array_equal(got, want):
        return None
    nz = g if planes is None else planes
    bad = (got != want).reshape(nz, g, g)
    cells = (np.asarray(before).reshape(nz, g, g) != 0).astype(np.uint8)
    z, y, x = (int(v[0]) for v in np.nonzero(bad))
    head = f"{what}: {int(bad.sum())} cells differ from the oracle, the first at (x, y, z) = ({x}, {y}, {z})"
    if planes is None:  # a torus: turn the first differing plane to plane 1
        bad, cells, z = np.roll(bad, 1 - z, axis=0), np.roll(cells, 1 - z, axis=0), 1
    lo, hi = max(z, 1), min(z + 4, nz - 1)  # a few planes from the first difference on: enough to name the classes
    if lo >= hi:
        return head
    alive, n = gl.cells_counts_of_planes(cells, lo, hi, dtype=np.int8, torus=True)
    sel = bad[lo:hi]
    rows = np.stack([alive[sel], n["F"][sel], n["E"][sel], n["C"][sel], n["T"][sel]], axis=1)
    uniq, cnt = np.unique(rows, axis=0, return_counts=True)
    return head + f"; (alive, F, E, C, T) x cells in the first {hi - lo} such planes: {[(tuple(int(v) for v in u), int(c)) for u, c in zip(uniq[:8], cnt[:8])]}"


# ------------------------------------------------------------------------------------------------ driving an engine (or a stand-in)

BALLOT, LITERAL = b"ca_unpacked_ballot", b"ca_unpacked_literal"
_FIRST, _LAST = {}, {}


def kernel_of(form):
    """What info().kernel_name reports after a launch of a form: the pipelined kernel goes by the ballot kernel's name."""
    return LITERAL if form == "literal" else BALLOT


def first_state(g, name):
    """A graded start state, one u32 per cell (read-only: shared by every id of the process)."""
    if (g, name) not in _FIRST:
        w = gl.unpacked_state(g, name)
        w.setflags(write=False)
        _FIRST[g, name] = w
    return _FIRST[g, name]


def rules_of(case):
    return rc.rules_of(case.kind, case.rule)


def trajectory(g, name, case):
    """The oracle's states from a graded start state under a case's rule (slab_lone.Trajectory: computed on demand), kept for the ids
    that follow at once with the same grid and rule and no longer: one rule's states at a time, whatever the grid."""
    key = (g, case.kind, case.rule.born, case.rule.survive)
    if _LAST.get("key") != key:
        _LAST.clear()
        _LAST["key"] = key
    if name not in _LAST:
        _LAST[name] = sl.Trajectory(g, rules_of(case), LAYOUT_UNPACKED, first_state(g, name))
    t = _LAST[name]
    # the rule decides something on this state
    assert t(1).any() and not np.array_equal(t(1), t(0)), f"{rc.label(case.kind, case.rule, name)} at {g}^3 leaves nothing to compare"
    return t


def full_case(eng, g, case, names, want, variant=0, classes=True, r=None):
    """The rule of `case` on the full grid g: the launcher's form must be `want` (unpacked_form of a 0 / 1 state; option `variant` 1
    keeps the literal kernel), then from every start state two single steps, the second from the ping-pong buffer, each against the
    oracle and each with the kernel's name asked afterwards. `classes` False: a grid that is no torus (not a power of two) — a
    difference is reported by position only. `r`: other rule arrays that must give the same states (tables with other values > 0, side
    tables that fire)."""
    form = unpacked_form(g, g, binary=variant == 0)
    assert form == want, (g, form, want)
    what = f"{form} ({pack_form(g)} pack)" if form != "literal" else form
    lines = []
    eng.configure(g, LAYOUT_UNPACKED)
    try:
        eng.set_option("variant", variant)
        set_rules(eng, rules_of(case) if r is None else r)
        for name in names:
            t = trajectory(g, name, case)
            eng.upload_state(t(0))
            for step in (1, 2):
                eng.step(1)
                got = eng.info().kernel_name
                assert got == kernel_of(form), (got, form)
                at = f"{what}: {rc.label(case.kind, case.rule, name)} at {g}^3, step {step}"
                if classes:
                    lines.append(differs(g, eng.read_state(), t(step), t(step - 1), at))
                elif not np.array_equal(eng.read_state(), t(step)):
                    lines.append(f"{at}: differs from the oracle, first at cell index {int(np.flatnonzero(eng.read_state() != t(step))[0])}")
    finally:
        eng.set_option("variant", 0)
    rc.settle(lines)


def _slab_failure(eng, g, nz, before, want, what, err):
    """A lone-slab run that failed on its owned planes: add the classes of the last sub-step's cells that were answered wrongly."""
    if "owned planes" not in str(err):
        return str(err)
    line = differs(g, eng.read_state(), want, before, what, planes=nz)
    return f"{err}\n{line}" if line else str(err)


def slab_case(eng, g, case, geometry, phased, want_forms, name="x"):
    """A lone slab of the full-grid oracle states of a case (slab_lone.run_lone_slab, both ghosts from the oracle): every launch
    length of the run must give one of `want_forms`, and all of them must occur; after every batch the engine must name the ballot
    kernel."""
    z0, nz, K, batches = geometry
    forms = run_forms(g, sl.launches(nz, K, batches, False, phased))
    assert set(forms) == set(want_forms), (geometry, phased, sorted(set(forms)), want_forms)
    t, r, seen = trajectory(g, name, case), rules_of(case), []

    def after(n):
        seen.append(n)
        assert eng.info().kernel_name == BALLOT, eng.info().kernel_name

    what = f"{'/'.join(sorted(set(forms)))}: {rc.label(case.kind, case.rule, name)} at {g}^3, slab {geometry}{' phased' if phased else ''}"
    try:
        sl.run_lone_slab(eng, t, r, z0, nz, K, batches, phased, layout=LAYOUT_UNPACKED, after_batch=after)
    except AssertionError as err:
        done = sum(seen) + batches[len(seen)]
        before = sl.owned_planes(g, LAYOUT_UNPACKED, t(done - 1), z0, nz)
        pytest.fail(_slab_failure(eng, g, nz, before, sl.owned_planes(g, LAYOUT_UNPACKED, t(done), z0, nz), what, err), pytrace=False)
    assert tuple(seen) == tuple(batches)


_WIDE = {}


def wide_array(g, nz, K, name="x"):
    """A graded plane array of nz + 4 K planes of g x g cells, one u32 per cell (slab_lone.run_lone_slab_planes), kept."""
    key = (g, nz + 4 * K, name)
    if key not in _WIDE:
        axis, reverse = gl.ORIENTATIONS[name]
        _WIDE[key] = gl.graded_cells(g, axis, reverse, planes=nz + 4 * K).astype(np.uint32).ravel()
        _WIDE[key].setflags(write=False)
    return _WIDE[key]


def slab_planes_case(eng, g, case, geometry, phased, want_forms, name="x"):
    """slab_case on a grid too large for a full-grid oracle state: the slab's planes and ghosts come from a graded plane array and the
    expectation from the oracle's plane-range step on it."""
    z0, nz, K, batches = geometry
    forms = run_forms(g, sl.launches(nz, K, batches, False, phased))
    assert set(forms) == set(want_forms), (geometry, phased, sorted(set(forms)), want_forms)
    r, seen = rules_of(case), []
    states = sl.wide_states(g, wide_array(g, nz, K, name), r, max(batches))
    pw = g * g
    assert states[1][K * pw:-K * pw].any() and not np.array_equal(states[1][K * pw:-K * pw], states[0][K * pw:-K * pw])

    def after(n):
        seen.append(n)
        assert eng.info().kernel_name == BALLOT, eng.info().kernel_name

    what = f"{'/'.join(sorted(set(forms)))}: {rc.label(case.kind, case.rule, name)} at {g}^2 x {nz + 2 * K} planes, slab {geometry}{' phased' if phased else ''}"
    try:
        sl.run_lone_slab_planes(eng, g, states, r, z0, nz, K, batches, phased, after_batch=after)
    except AssertionError as err:
        n = batches[len(seen)]
        own = slice(2 * K * pw, (2 * K + nz) * pw)
        pytest.fail(_slab_failure(eng, g, nz, states[n - 1][own], states[n][own], what, err), pytrace=False)
    assert tuple(seen) == tuple(batches)
