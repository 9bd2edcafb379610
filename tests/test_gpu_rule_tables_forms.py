"""Rule tables bit by bit on every kernel form the engine selects: each form adds up the three neighbour classes in its own way (a
three-plane register window, whole rows per wave, halo planes from eight neighbour tiles, rows of 1 / 3 / 11 words), and a random fill
at density 1/2 never asks what a form does at a Moore count of 24, an edges count of 12 or a corners count of 8. Here every form meets
graded states (graded_lib: every (alive, count) pair of every table, test_graded_cpu.py shows it at these grids) under coded rules that
answer any two counts differently, each at the smallest grid that selects it — the power-of-two rolling-window kernels at the smallest
grid that compiles them, 256^3, with the form forced: launches that small are not given to them otherwise (see the tests).

One rule per test id. Every id asserts the kernel it is about by name before its first step, takes two single steps from each graded
state (the second from the ping-pong buffer), and compares with oracle_lib.packed_step exactly; a difference names form, grid, rule,
orientation and the (alive, F, E, C, T) classes answered wrongly. The resident forms take steps 1, 1, 8 inside resident launches.

Families. FULL: the coded rules of the Moore (27), edges-as-main (13) and corners-as-main (9) tables, six clustered combinations of all
three classes, and two rules each of a von Neumann main with a coded edges / corners table. SHORT: born and survive of the two highest
coded bits of those three main tables (the planes a lost carry hits) and one clustered combination. Orientations z and x, plus the
reversed z for the top-bit rules."""
import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol
from cellularautomatons3d_amd import host
from gpu_common import set_rules
from rule_tables_common import FLAT, FLAT_TOP, FULL, SHORT, Case, coded_cases, differs, first_state, form, ids, label, rules_of, settle, starts
from test_gpu_ca_parity import VN_TABLE_PAIRS

pytestmark = pytest.mark.gpu


def _pair_case(born, survive):
    """A (born, survive) pair of rule strings as a case of kind "vn"."""
    masks = [sum(1 << c for c in host.rules_components_to_values(s)) for s in (born, survive)]
    return Case(f"B{born}_S{survive}", "vn", gl.Rule(f"B{born}/S{survive}", masks[0], masks[1], born, survive), False)


VN = coded_cases("vn", "vn") + [_pair_case(b, s) for b, s in VN_TABLE_PAIRS]
assert len(VN) == 22


TAGS = {"von neumann": "vn", "von neumann 2D": "vn2d", "moore": "moore", "moore 2D": "moore2d", "edges": "edges", "corners": "corners"}


def class_tag(case):
    """What the class kernels' names carry between < and >: the main list, then E / C where that side table can fire."""
    kw = gl.strings_of(*form(case.kind, case.rule))
    r = rules_of(case.kind, case.rule)
    fires = [bool(r.born[27 * s:27 * s + n].any() or r.survive[27 * s:27 * s + n].any()) for s, n in ((1, 13), (2, 9))]
    return TAGS[kw["neighbourhood"]] + (",E" if fires[0] else "") + (",C" if fires[1] else "")


@pytest.fixture(scope="module")
def eng():
    from cellularautomatons3d_amd import Engine

    e = Engine(0)
    yield e
    e.close()


DEFAULTS = {"resident": 1, "resident_min": 8, "roll": 1, "roll_tile": 1, "roll_z": 0}


_LAST = {}


def oracle_states(g, name, case):
    """Oracle states 0, 1, 2 of a case from a graded state, kept for the ids that follow at once with the same grid and rule (the forced
    forms of one kernel: the rule is the slowest parameter there) and no longer: one rule's states at a time, whatever the grid."""
    key = (g, tuple(sorted(gl.strings_of(*form(case.kind, case.rule)).items())))
    if _LAST.get("key") != key:
        _LAST.clear()
        _LAST["key"] = key
    if name not in _LAST:
        r = rules_of(case.kind, case.rule)
        t = [first_state(g, name)]
        for _ in range(2):
            t.append(ol.packed_step(g, t[-1], r))
        _LAST[name] = t
    t = _LAST[name]
    # the rule decides something on this state
    assert t[1].any() and not np.array_equal(t[1], t[0]), f"{label(case.kind, case.rule, name)} at {g}^3 leaves nothing to compare"
    return t


def form_case(eng, g, case, want_name, names, options=None, resident=False):
    """The rule of `case` on grid g under `options`: assert the form by name, then from every start state two single steps against the
    oracle (resident: 1, 1 and 8 steps inside resident launches). Options go back to the defaults whatever happens."""
    options = dict(options or {}, **({"resident_min": 1} if resident else {}))
    what = f"{want_name.decode()} {sorted(options.items())}"
    lines = []
    eng.configure(g)
    try:
        for k, v in options.items():
            eng.set_option(k, v)
        r = rules_of(case.kind, case.rule)
        set_rules(eng, r)
        assert eng.info().kernel_name == want_name, (eng.info().kernel_name, want_name)
        for name in names:
            t = oracle_states(g, name, case)
            eng.upload_state(t[0])
            for step in (1, 2):
                eng.step(1)
                lines.append(differs(g, eng.read_state(), t[step], t[step - 1], f"{what}: {label(case.kind, case.rule, name)} at {g}^3, step {step}"))
            if resident:
                eng.step(8)
                if not np.array_equal(eng.read_state(), ol.packed_run(g, t[2], r, 8)):
                    lines.append(f"{what}: {label(case.kind, case.rule, name)} at {g}^3 differs after the 8-step launch (steps 3 .. 10)")
                assert eng.info().step == 10 and eng.info().current_buffer == 0
        if resident:
            # the launches did not quietly give up and hand their steps to the per-step kernels
            assert eng.recovered_launches() == 0
            assert eng.info().kernel_name == want_name, eng.info().kernel_name
    finally:
        for k in options:
            eng.set_option(k, DEFAULTS[k])
        if resident:
            eng.set_option("resident", 1)  # (a launch that gave up switches the path off: on again for the next id)
    settle(lines)


# ------------------------------------------------------------------------------------------------ the rows kernel

@pytest.mark.parametrize("case", FULL + FLAT, ids=ids(FULL + FLAT))
@pytest.mark.parametrize("g", [32, 96])
def test_rows_kernel_one_and_three_words_a_row(eng, g, case):
    """ca_packed_rows_kernel.inc at 32^3 (a row is one word: both x neighbours of a word are the word itself or nothing) and 96^3 (three
    words, 21 rows a wave and a lane left over)."""
    form_case(eng, g, case, b"ca_packed_rows(jit)", starts(case))


@pytest.mark.parametrize("case", SHORT, ids=ids(SHORT))
def test_rows_kernel_at_352(eng, case):
    """Rows of 11 words, six planes a thread, and 352 % 6 = 4: the last z-run is shifted back over planes already written."""
    form_case(eng, 352, case, b"ca_packed_rows(jit)", starts(case))


# ------------------------------------------------------------------------------------------------ the rolling window, whole rows per wave

@pytest.mark.parametrize("case", FULL, ids=ids(FULL))
def test_roll_np2_kernel_at_384(eng, case):
    """roll_step_np2 (ca_packed_roll_kernel.inc) at the launcher's own depth: rows of three uint4, 21 whole rows a wave."""
    form_case(eng, 384, case, b"ca_packed_roll_np2(jit)", starts(case))


@pytest.mark.parametrize("z", [2, 4, 8])
@pytest.mark.parametrize("case", SHORT, ids=ids(SHORT))
def test_roll_np2_kernel_at_384_every_depth(eng, z, case):
    form_case(eng, 384, case, b"ca_packed_roll_np2(jit)", starts(case), {"roll_z": z})


# ------------------------------------------------------------------------------------------------ the rolling window at 256, the class kernel

def roll_name(case):
    return b"ca_packed_class_roll<" + class_tag(case).encode() + b">(jit)"


def class_name(case):
    return b"ca_packed_class<" + class_tag(case).encode() + b">(jit)"


@pytest.mark.parametrize("case", FULL, ids=ids(FULL))
def test_class_roll_selection_at_256(eng, case):
    """What a 256^3 engine without the resident kernel runs with every option at its default. The name says which kernels were SELECTED
    (the rolling-window module is compiled); it does not say what a launch runs: with roll_z 0 the launcher keeps the rolling kernels
    for launches of two resident generations of waves or more (ca_packed.hip: tiles_per_plane * nruns * 4 >= 4096), and a 256^3 launch
    is smaller, so these steps run the run-time compiled ca_packed_class — the device code of test_class_kernel_at_256, reached through
    the default selection. The rolling-window kernels themselves meet the full family in the test below."""
    form_case(eng, 256, case, roll_name(case), starts(case), {"resident": 0})


# On the rows below the kernel's name does not depend on roll_tile / roll_z: that a forced form is the one launched rests on the launcher
# (ca_packed.hip, launch_class): a forced depth is taken when its entry point exists and the shortest plane range holds it, else the
# launch falls through to the class kernel. Both hold here: the run-time compiler makes every entry point of the module mandatory on
# rows of up to 16 uint4 (ca_jit.cpp, jit_roll_kernels: get_entries fails the whole module otherwise, and the name would lose "roll"),
# and a full 256^3 grid is one range of 256 planes >= 30.

@pytest.mark.parametrize("tile,z", [(1, 16), (0, 8)])
@pytest.mark.parametrize("case", FULL, ids=ids(FULL))
def test_class_roll_kernel_full_family(eng, tile, z, case):
    """The rolling-window kernels under the full family — every coded bit of the three main tables, the clustered combinations, and the
    von Neumann mains with an edges or a corners table (the kernels' E / C_ template flags) — in the two forms the launcher chooses by
    itself on grids large enough: the 256-thread tile form at 16 planes a thread (tile_step: 1024^3 and up) and every thread shifting
    its own rows at 8 (roll_step). Forced here, since 256^3 is the smallest grid that compiles them and too small to be given them."""
    form_case(eng, 256, case, roll_name(case), starts(case), {"resident": 0, "roll_tile": tile, "roll_z": z})


@pytest.mark.parametrize("tile,z", [(1, 2), (1, 30), (0, 4), (0, 15), (2, 8), (3, 16)])
@pytest.mark.parametrize("case", SHORT, ids=ids(SHORT))
def test_class_roll_kernel_every_tile_form(eng, tile, z, case):
    """ca_packed_roll_kernel.inc with the other forms and depths forced: the 256-thread tile form (2 planes a thread, the looped 30), every
    thread shifting its own rows (4, the looped 15), wave tiles (8) and two words a thread (16); (1, 16) runs the full family above, the
    short one included. Partial sums A, B, c over a three-plane register window: the top planes of A(z) + c(z - 1) + c(z + 1) are what
    the top-bit rules read."""
    form_case(eng, 256, case, roll_name(case), starts(case), {"resident": 0, "roll_tile": tile, "roll_z": z})


@pytest.mark.parametrize("case", FULL + FLAT, ids=ids(FULL + FLAT))
def test_class_kernel_at_256(eng, case):
    """ca_packed_class compiled for the rule at run time where a row of eight words spans two lanes."""
    form_case(eng, 256, case, class_name(case), starts(case), {"resident": 0, "roll": 0})


@pytest.mark.parametrize("case", FLAT_TOP, ids=ids(FLAT_TOP))
def test_class_np2_entry_at_768(eng, case):
    """The class kernel's run-time compiled np2 entry points (rows of six uint4): the 2D rules keep them at 768 and up."""
    name = class_name(case)
    assert b"class" in name and b"(jit)" in name
    form_case(eng, 768, case, name, ("y", "x"))


# ------------------------------------------------------------------------------------------------ the resident kernels

@pytest.mark.parametrize("case", FULL, ids=ids(FULL))
@pytest.mark.parametrize("g", [256, 512])
def test_resident_class_kernel(eng, g, case):
    """ca_resident_class_kernel.inc: 256^3 (two z groups a tile) and 512^3 (one), halo planes and corner rows from eight neighbour tiles;
    launches of 1, 1 and 8 steps (odd and even landing buffers, several steps inside one launch)."""
    form_case(eng, g, case, b"ca_resident_class(jit)", starts(case), resident=True)


@pytest.mark.parametrize("case", VN, ids=ids(VN))
@pytest.mark.parametrize("g", [64, 256, 512])
def test_resident_von_neumann_kernels(eng, g, case):
    """ca_resident_kernel.inc: one workgroup at 64^3, z groups at 256^3, the row-pair form at 512^3 — the coded von Neumann rules and the
    table pairs that take every branch of vn_next (test_gpu_ca_parity.py)."""
    prebuilt = (case.rule.born, case.rule.survive) == (0b1010, 0b1111111)  # the start-up rule
    form_case(eng, g, case, b"ca_resident_vn" if prebuilt else b"ca_resident_vn(jit)", starts(case), resident=True)
