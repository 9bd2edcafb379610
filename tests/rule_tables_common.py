"""Start states, oracle trajectories and the wording of a failure — TEST INFRASTRUCTURE shared by test_gpu_rule_tables.py and
test_gpu_rule_tables_forms.py. Expected states always come from CPU-oracle steps (oracle_lib.packed_step), computed once per process;
graded_lib's counts serve the wording of a failure only."""
from collections import namedtuple

import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol
from cellularautomatons3d_amd import host
from gpu_common import set_rules

_FIRST, _TRAJ = {}, {}


def first_state(g, name):
    """A start state by name: a graded orientation, "full" or "empty"."""
    if (g, name) not in _FIRST:
        if name in gl.ORIENTATIONS:
            axis, reverse = gl.ORIENTATIONS[name]
            w = gl.graded_state(g, axis, reverse)
        else:
            w = np.full(host.words_per_buffer(g), 0xFFFFFFFF if name == "full" else 0, dtype=np.uint32)
        _FIRST[g, name] = w
    return _FIRST[g, name]


def form(kind, rule):
    """(oracle kind, rule) of a table kind: the plain kinds ("vn", "moore", "edges main", ...) and the mixed ones ("vn+edges",
    "vn+corners") take the rule as it is, a clustered class ("main", "edges", "corners") fires alone; "all": `rule` is a (main, edges,
    corners) triple already."""
    if kind in gl.PLAIN or kind in gl.MIXED:
        return kind, rule
    return "clustered", (rule if kind == "all" else gl.clustered(kind, rule))


def rules_of(kind, rule):
    """The oracle's / the engine's rule arrays of a table kind's rule."""
    return ol.Rules.from_strings(**gl.strings_of(*form(kind, rule)))


def trajectory(g, name, kind, rule, steps):
    """Oracle states 0 .. steps from a named start state under a rule, computed once per module and extended on demand."""
    k, r = form(kind, rule)
    kw = gl.strings_of(k, r)
    t = _TRAJ.setdefault((g, name, tuple(sorted(kw.items()))), [first_state(g, name)])
    if len(t) <= steps:
        rules = ol.Rules.from_strings(**kw)
        while len(t) <= steps:
            t.append(ol.packed_step(g, t[-1], rules))
    return t


def label(kind, rule, name):
    k, r = form(kind, rule)
    return f"{gl.name_of(k, r)}, start {name}"


def differs(g, got, want, before, what):
    """None when got == want, else a line that says which (alive, faces, edges, corners) cells of `before` were answered wrongly."""
    if np.array_equal(got, want):
        return None
    bad = gl.unpack(g, np.asarray(got, dtype=np.uint32) ^ want).astype(bool)
    n = gl.counts_of(g, before, dtype=np.int8)
    alive = gl.unpack(g, before)
    rows = np.stack([alive[bad], n["F"][bad], n["E"][bad], n["C"][bad], n["T"][bad]], axis=1)
    uniq, cnt = np.unique(rows, axis=0, return_counts=True)
    z, y, x = (int(v[0]) for v in np.nonzero(bad))
    return (f"{what}: {int(bad.sum())} cells differ from the oracle, the first at (x, y, z) = ({x}, {y}, {z}); "
            f"(alive, F, E, C, T) x cells: {[(tuple(int(v) for v in u), int(c)) for u, c in zip(uniq[:8], cnt[:8])]}")


def settle(lines):
    """Fail with every difference found, not the first alone: which bits fail together is what locates a fault."""
    lines = [m for m in lines if m]
    if lines:
        pytest.fail(f"{len(lines)} cases differ:\n" + "\n".join(lines[:60]), pytrace=False)


def engine_case(eng, g, kind, rule, name, modes):
    """One step, then a second (the engine's ping-pong buffers) under every mode, against the oracle -> the differences found."""
    lines = []
    t = trajectory(g, name, kind, rule, 2)
    rules = rules_of(kind, rule)
    for jit, variant in modes:
        eng.set_option("jit", jit)
        eng.set_option("variant", variant)
        set_rules(eng, rules)
        eng.upload_state(t[0])
        for step in (1, 2):
            eng.step(1)
            lines.append(differs(g, eng.read_state(), t[step], t[step - 1],
                                 f"{label(kind, rule, name)} at {g}^3, step {step}, jit={jit} variant={variant} {eng.info().kernel_name}"))
    return lines


# ------------------------------------------------------------------------------------------------ the families of test_gpu_rule_tables_forms.py

Case = namedtuple("Case", "id kind rule top")  # top: a rule of a table's highest coded bit — it also runs on the reversed z state


def coded_cases(kind, tag, bits=None):
    """The coded rules of a table kind, or those of its `bits` highest coded bits only."""
    fam, nb = gl.coded(gl.TABLES[kind]), gl.coded_bits(gl.TABLES[kind])
    keep = range(nb) if bits is None else range(nb - bits, nb)
    return [Case(f"{tag}-bit{j}-{'born' if h == 0 else 'survive'}", kind, fam[h * nb + j], j == nb - 1) for j in keep for h in (0, 1)]


MAINS = [("moore", "moore"), ("edges main", "edges"), ("corners main", "corners")]
VN_MAIN = gl.Rule("B2/S1-3", 0b100, 0b1110, "2", "1,2,3")  # the main rule of gpu_common's vn_edges_only / vn_corners_only


def _mixed_cases():
    out = []
    for cls, N in (("edges", 13), ("corners", 9)):
        fam, nb = gl.coded(N), gl.coded_bits(N)
        # the side table's top bit under the sparse main rule; its lowest bit, survive where set, under a coded von Neumann main
        for tag, main, side in (("top", VN_MAIN, fam[nb - 1]), ("low", gl.coded(7)[1], fam[nb])):
            kind, rule = gl.vn_with(cls, main, side)
            out.append(Case(f"vn+{cls}-{tag}", kind, rule, tag == "top"))
    return out


FULL = [c for kind, tag in MAINS for c in coded_cases(kind, tag)] + [Case(f"all-{j}", "all", gl.coded_all(j), False) for j in range(6)] + _mixed_cases()
SHORT = [c for kind, tag in MAINS for c in coded_cases(kind, tag, bits=2)] + [Case("all-0", "all", gl.coded_all(0), False)]
FLAT = coded_cases("moore 2D", "moore2d") + coded_cases("vn 2D", "vn2d")  # counts from the cell's own plane
FLAT_TOP = coded_cases("moore 2D", "moore2d", bits=2) + coded_cases("vn 2D", "vn2d", bits=2)
assert (len(FULL), len(SHORT), len(FLAT), len(FLAT_TOP)) == (36, 13, 14, 8)


def ids(cases):
    return [c.id for c in cases]


def starts(case, names=("z", "x")):
    return names + (("zr",) if case.top else ())


# grid -> the graded states the forms file starts from there (768: the 2D rules only, graded across and along the rows)
FORM_STARTS = {32: ("z", "x", "zr"), 96: ("z", "x", "zr"), 256: ("z", "x", "zr"), 352: ("z", "x", "zr"), 384: ("z", "x", "zr"),
               512: ("z", "x", "zr"), 768: ("y", "x")}
