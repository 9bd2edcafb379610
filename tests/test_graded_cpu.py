"""graded_lib without a GPU: the graded states reach every (alive, count) pair of every table often enough for a wrong leaf or a wrong
carry to show, and class_counts / plane_counts — the plain numpy restatement of the three neighbour classes and of the two in-plane
neighbourhoods — give the oracle's next state under rules that answer any two counts differently. The families of
test_gpu_rule_tables_forms.py decide something on every start state it uses, and its short family sees a count that lost one of its top
planes. Run with -s for the coverage figures."""
import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol
import rule_tables_common as rc

FLOOR = 32  # occurrences of every (alive, count) pair, whatever the orientation and the grid

_STATE, _COUNTS = {}, {}


def state(G, name):
    if (G, name) not in _STATE:
        axis, reverse = gl.ORIENTATIONS[name]
        _STATE[G, name] = gl.graded_state(G, axis, reverse)
    return _STATE[G, name]


def counts(G, name):
    if (G, name) not in _COUNTS:
        _COUNTS[G, name] = gl.counts_of(G, state(G, name))
    return _COUNTS[G, name]


def test_the_density_rises_along_the_axis():
    """Blocks of G / 9 planes at densities 0, 1/8 .. 7/8, 1: the first is empty, the last is full, the middle ones are near their
    density, and the three axes and the reversal are the same construction turned."""
    G = 64
    for name, (axis, reverse) in gl.ORIENTATIONS.items():
        cells = np.moveaxis(gl.unpack(G, state(G, name)), gl.AXES[axis], 0)
        if reverse:
            cells = cells[::-1]
        thr = np.minimum(9 * np.arange(G) // G, 8)
        assert thr[0] == 0 and thr[-1] == 8 and set(thr.tolist()) == set(range(9))
        for k in range(9):
            d = cells[thr == k].mean()
            assert abs(d - k / 8) < 0.01, (name, k, d)
        assert not cells[thr == 0].any() and cells[thr == 8].all()
    # with "x" the dense end lies in the high bits of a row's last word
    rows = state(G, "x").reshape(G * G, 2)
    assert (rows[:, 1] >> 25 == 0x7F).all() and not (rows[:, 0] & 0xFF).any()
    np.testing.assert_array_equal(gl.pack(G, gl.unpack(G, state(G, "y"))), state(G, "y"))


@pytest.mark.parametrize("G", [64, 128])
@pytest.mark.parametrize("name", list(gl.ORIENTATIONS))
def test_every_count_occurs_alive_and_dead(G, name):
    cov = gl.coverage(G, state(G, name), counts(G, name))
    mins = {k: (int(v[0].min()), int(v[1].min())) for k, v in cov.items()}
    print(f"graded {name} at {G}^3: (dead, alive) minima over the counts", mins)
    for k, v in cov.items():
        assert v.min() >= FLOOR, f"{k}: (alive, count) pair {np.unravel_index(v.argmin(), v.shape)} occurs {v.min()} times in graded {name} at {G}"


@pytest.mark.parametrize("name", ["z", "y", "zr"])
def test_the_word_boundary_columns_see_every_moore_count(name):
    """x = 31 | 32 is the seam between a row's two words and x = 63 the column whose + neighbour wraps; column 0's - neighbours are dead,
    so it cannot exceed T = 17."""
    G = 64
    alive, T = gl.unpack(G, state(G, name)).astype(np.int64), counts(G, name)["T"]
    got = {}
    for x in (31, 32, 63):
        c = np.bincount((alive[:, :, x] * 27 + T[:, :, x]).ravel(), minlength=54)
        got[x] = int(c.min())
        assert c.min() >= 1, f"column {x} of graded {name}: (alive, T) pair {divmod(int(c.argmin()), 27)} is missing"
    print(f"graded {name}: minimum occurrences of an (alive, T) pair in columns 31 / 32 / 63:", got)
    assert T[:, :, 0].max() == 17


def test_the_classes_occur_in_combination():
    G = 64
    n = counts(G, "z")
    key = ((gl.unpack(G, state(G, "z")).astype(np.int64) * 7 + n["F"]) * 13 + n["E"]) * 9 + n["C"]
    combos = np.unique(key).size
    print(f"graded z: {combos} of {2 * 7 * 13 * 9} (alive, F, E, C) combinations occur")
    assert combos >= 1300


def test_the_rule_families():
    for N in (7, 27, 13, 9, 5):
        hot, cod = gl.one_hot(N), gl.coded(N)
        assert len(hot) == 2 * N and len(cod) == 2 * gl.coded_bits(N) and 1 << gl.coded_bits(N) >= N > 1 << (gl.coded_bits(N) - 1)
        assert sorted(r.born for r in hot if r.born) == sorted(r.survive for r in hot if r.survive) == [1 << k for k in range(N)]
        assert all(bool(r.born) != bool(r.survive) for r in hot)
        full = (1 << N) - 1
        for r in cod:
            assert r.born ^ r.survive == full  # born and survive differ at every count
        for a in range(N):
            for b in range(a + 1, N):  # any two counts are told apart, dead and alive
                assert any((r.born >> a ^ r.born >> b) & 1 for r in cod) and any((r.survive >> a ^ r.survive >> b) & 1 for r in cod)
        for r in hot + cod:  # the strings say what the masks say
            for s, m in ((r.born_str, r.born), (r.survive_str, r.survive)):
                assert sum(1 << int(c) for c in s.split(",") if c) == m
    fams = [gl.coded(gl.TABLES[c]) for c in gl.CLASSES]
    for j in range(10):  # all three classes at once: class s runs coded rule (j + s) mod its family size
        assert gl.coded_all(j) == tuple(f[(j + s) % len(f)] for s, f in enumerate(fams))
    assert len({gl.coded_all(j) for j in range(10)}) == 10


def rules_of(kind):
    """(oracle kind, rule) list: the coded rules of a table; a clustered class fires alone."""
    fam = gl.coded(gl.TABLES[kind])
    return [(kind, r) for r in fam] if kind in gl.PLAIN else [("clustered", gl.clustered(kind, r)) for r in fam]


def pin(G, name, kind, rule):
    st = state(G, name)
    want = ol.packed_step(G, st, ol.Rules.from_strings(**gl.strings_of(kind, rule)))
    got = gl.next_state(G, st, kind, rule, counts(G, name))
    assert want.any() and (want != st).any()
    np.testing.assert_array_equal(got, want, err_msg=f"{gl.name_of(kind, rule)} on graded {name}")


@pytest.mark.parametrize("name", list(gl.ORIENTATIONS))
@pytest.mark.parametrize("kind", list(gl.TABLES))
def test_class_counts_give_the_oracles_next_state(kind, name):
    """Every coded rule of the kind, on every orientation: a y- or x-graded state has live cells on both z faces, so each axis' dead -
    side and wrapping + side is told apart from the other by some orientation."""
    for k, rule in rules_of(kind):
        pin(64, name, k, rule)


@pytest.mark.parametrize("kind", list(gl.TABLES))
def test_the_lowest_and_highest_bit_of_every_table(kind):
    N = gl.TABLES[kind]
    hot = gl.one_hot(N)
    for r in (hot[0], hot[N - 1], hot[N], hot[2 * N - 1]):
        if kind in gl.PLAIN:
            pin(64, "z", kind, r)
        else:
            pin(64, "z", "clustered", gl.clustered(kind, r))


def test_all_three_classes_at_once():
    for j in (0, 7):
        pin(64, "x", "clustered", gl.coded_all(j))


# ------------------------------------------------------------------------------------------------ the kinds and grids of test_gpu_rule_tables_forms.py

NEW_PLAIN = ["edges main", "corners main", "moore 2D", "vn 2D"]


def test_the_plane_counts_by_hand():
    """F2 / M2 on a state small enough to count by eye: a plus and a far corner cell in plane 3 of a 32^3 grid, nothing else."""
    G = 32
    cells = np.zeros((G, G, G), dtype=np.uint8)
    for y, x in ((5, 5), (4, 5), (6, 5), (5, 4), (5, 6), (31, 31)):
        cells[3, y, x] = 1
    n = gl.counts_of(G, gl.pack(G, cells))
    assert (n["F2"][3, 5, 5], n["M2"][3, 5, 5]) == (4, 4) and (n["F2"][3, 4, 4], n["M2"][3, 4, 4]) == (2, 3)
    assert not n["F2"][2].any() and not n["M2"][4].any() and n["F"][2, 5, 5] == 1  # the planes above and below see it through F only
    # (31, 31) is the + neighbour of x = 30 / y = 30 and, wrapped, of nobody's - side: coordinate -1 is dead, coordinate G wraps to 0
    assert n["M2"][3, 30, 30] == 1 and n["F2"][3, 30, 31] == 1 and n["M2"][3, 0, 0] == 0 and n["M2"][3, 31, 31] == 0
    cells[3, 0, 0] = 1
    n = gl.counts_of(G, gl.pack(G, cells))
    assert n["M2"][3, 31, 31] == 1 and n["F2"][3, 31, 0] == 1 and n["M2"][3, 0, 0] == 0
    F2, M2 = gl.plane_counts(G, gl.pack(G, cells))
    np.testing.assert_array_equal(F2, n["F2"])
    np.testing.assert_array_equal(M2, n["M2"])


@pytest.mark.parametrize("G,name", [(32, n) for n in gl.ORIENTATIONS] + [(64, "z"), (64, "x")])
@pytest.mark.parametrize("kind", NEW_PLAIN)
def test_the_new_main_tables_give_the_oracles_next_state(kind, G, name):
    """One one-hot rule per table entry (a count off by one, or taken from another neighbourhood, answers for the wrong entry) and the
    coded family, at 32^3 and 64^3."""
    N = gl.TABLES[kind]
    for r in gl.one_hot(N) + gl.coded(N):
        pin(G, name, kind, r)


@pytest.mark.parametrize("G,name", [(32, n) for n in gl.ORIENTATIONS] + [(64, "z"), (64, "x")])
@pytest.mark.parametrize("cls", ["edges", "corners"])
def test_a_von_neumann_main_with_one_side_table(cls, G, name):
    """The mixed kinds: the side table one-hot and coded under the sparse main rule, and coded under a coded main."""
    N = gl.TABLES[cls]
    for side in gl.one_hot(N) + gl.coded(N):
        pin(G, name, *gl.vn_with(cls, rc.VN_MAIN, side))
    for j, side in enumerate(gl.coded(N)):
        pin(G, name, *gl.vn_with(cls, gl.coded(7)[j % 6], side))


def test_counts_of_a_plane_range():
    G, st = 64, state(64, "x")
    alive, n = gl.counts_of_planes(G, st, 5, 40, dtype=np.int8)
    np.testing.assert_array_equal(alive, gl.unpack(G, st)[5:40])
    for k, v in counts(G, "x").items():
        np.testing.assert_array_equal(n[k], v[5:40], err_msg=k)


@pytest.mark.parametrize("G,floor", [(32, 8), (96, 32), (256, 32), (384, 32)])
def test_every_count_occurs_at_the_grids_of_the_kernel_forms(G, floor):
    """What test_gpu_rule_tables_forms.py rests on: every (alive, count) pair of every table — the two in-plane counts included — at least
    32 times on every orientation at 96, 256 and 384, and at least 8 times at 32 (one graded axis is enough there too). At 256 and 384
    the pairs are counted on a part of the planes only — 64 planes of a state graded along y or x, 12 planes around each of the eight
    density steps of one graded along z: what occurs there occurs in the grid, so the bound holds for the grid all the more."""
    for name, (axis, reverse) in gl.ORIENTATIONS.items():
        st = gl.graded_state(G, axis, reverse)
        if G < 256:
            cov = gl.coverage(G, st, gl.counts_of(G, st, dtype=np.int8))
        else:
            steps = [-(-k * G // 9) for k in range(1, 9)] if axis == "z" else []  # the first plane of each denser block ("zr": mirrored)
            ranges = [(max(b - 6, 1), min(b + 6, G - 1)) for b in steps] or [(G // 2, G // 2 + 64)]
            if reverse:
                ranges = [(G - hi, G - lo) for lo, hi in ranges]
            cov = {k: np.zeros((2, N), dtype=np.int64) for k, N in gl.SIZES.items()}
            for lo, hi in ranges:
                alive, n = gl.counts_of_planes(G, st, lo, hi, dtype=np.int8)
                for k, N in gl.SIZES.items():
                    cov[k] += np.bincount((alive.astype(np.int16) * N + n[k]).ravel(), minlength=2 * N).reshape(2, N)
        print(f"graded {name} at {G}^3: smallest number of occurrences of an (alive, count) pair", {k: int(v.min()) for k, v in cov.items()})
        for k, v in cov.items():
            assert v.min() >= floor, f"{k}: (alive, count) pair {np.unravel_index(v.argmin(), v.shape)} occurs {v.min()} times in graded {name} at {G}"


def slab_of(G, name):
    """Up to 16 inner planes of a graded state that hold its dense end: across the step from density 7/8 to 1 where z is the graded axis."""
    if name not in ("z", "zr"):
        return G // 2, min(G // 2 + 16, G - 1)
    edge = -(-8 * G // 9)  # the first full plane of "z"
    lo, hi = edge - 8, min(edge + 8, G - 1)
    return (lo, hi) if name == "z" else (G - hi, G - lo)


LOST_PLANES = {"T": (4, 3), "E": (3, 2), "C": (3, 2), "M2": (3, 2), "F2": (2, 1)}  # the two top planes of each count
KEY_OF = {"moore": "T", "edges main": "E", "corners main": "C", "moore 2D": "M2", "vn 2D": "F2"}


@pytest.mark.parametrize("G", sorted(rc.FORM_STARTS))
def test_the_short_family_sees_a_lost_top_plane(G):
    """Sensitivity without a kernel: on every start state the GPU file uses, a count that lost one of its two top planes (a dropped carry)
    makes at least one rule of the family that runs there differ from the oracle — and the intact counts do not. On a plane range of
    the dense end (the counts of a whole 768^3 state are not needed to show it)."""
    family = rc.FLAT_TOP if G == 768 else rc.SHORT
    for name in rc.FORM_STARTS[G]:
        st = state(G, name) if G <= 128 else gl.graded_state(G, *gl.ORIENTATIONS[name])
        lo, hi = slab_of(G, name)
        alive, n = gl.counts_of_planes(G, st, lo, hi, dtype=np.int8)
        want = {}

        def notices(c, broken):
            """The rule answers the broken counts differently from the oracle (and the intact ones as the oracle does)."""
            if c.id not in want:
                want[c.id] = gl.unpack(G, ol.packed_step(G, st, rc.rules_of(c.kind, c.rule)))[lo:hi]
                np.testing.assert_array_equal(gl.next_cells(alive, n, c.kind, c.rule), want[c.id], err_msg=f"{c.id} on graded {name} at {G}")
            return bool((gl.next_cells(alive, broken, c.kind, c.rule) != want[c.id]).any())

        for key in sorted({KEY_OF[c.kind] for c in family if c.kind in KEY_OF}):
            for plane in LOST_PLANES[key]:
                broken = dict(n)
                broken[key] = n[key] & ~np.int8(1 << plane)
                assert (broken[key] != n[key]).any()
                rules = sorted((c for c in family if KEY_OF.get(c.kind) == key), key=lambda c: f"bit{plane}-" not in c.id)  # that bit's rules first
                assert any(notices(c, broken) for c in rules), f"no rule notices plane {plane} of {key} missing on graded {name} at {G}"


@pytest.mark.parametrize("G", [32, 64, 96])
def test_the_families_decide_something(G):
    """Every rule of the GPU file's families changes the graded state and leaves it non-empty (asserted again where the oracle states are
    made on the larger grids)."""
    for c in rc.FULL + rc.FLAT:
        for name in rc.starts(c):
            nxt = ol.packed_step(G, state(G, name), rc.rules_of(c.kind, c.rule))
            assert nxt.any() and (nxt != state(G, name)).any(), (c.id, name, G)


# ------------------------------------------------------------------------------------------------ the torus of the one-u32-per-cell layout

def test_the_unpacked_state_is_the_graded_state_one_word_a_cell():
    G = 32
    for name in gl.ORIENTATIONS:
        u = gl.unpacked_state(G, name)
        assert u.dtype == np.uint32 and u.shape == (G ** 3,) and int(u.max()) == 1
        cells = gl.unpack(G, state(G, name))
        np.testing.assert_array_equal(u.reshape(G, G, G), cells)
        for x, y, z in ((0, 0, 0), (31, 0, 0), (5, 9, 2), (30, 31, 17), (31, 31, 31)):
            assert u[x + G * y + G * G * z] == cells[z, y, x]


def test_the_torus_counts_by_hand():
    """Coordinate -1 is coordinate G - 1 on every axis: the live cell in the last corner is a neighbour of cell (0, 0, 0) and of the
    other cells that look at it across a - face; with the packed layout's boundary those see nothing there."""
    G = 32
    cells = np.zeros((G, G, G), dtype=np.uint8)
    cells[31, 31, 31] = 1
    n = gl.counts_of_cells(cells, torus=True)
    assert n["C"][0, 0, 0] == n["C"][30, 30, 30] == n["C"][0, 30, 0] == 1 and n["C"].sum() == 8
    assert n["F"][0, 31, 31] == n["F"][31, 0, 31] == n["F"][31, 31, 0] == n["F"][30, 31, 31] == 1 and n["F"].sum() == 6
    assert n["E"].sum() == 12 and n["T"].sum() == 26 and n["F2"].sum() == 4 and n["M2"].sum() == 8 and n["M2"][31, 0, 0] == 1
    dead = gl.counts_of_cells(cells)  # the packed layout's boundary: only the + side wraps
    assert dead["T"].sum() == 7 and dead["C"][30, 30, 30] == 1 and dead["C"][0, 0, 0] == 0 and dead["M2"][31, 0, 0] == 0
    np.testing.assert_array_equal(gl.counts_of(G, gl.pack(G, cells), torus=True)["T"], n["T"])


@pytest.mark.parametrize("G", [32, 64])
@pytest.mark.parametrize("name", list(gl.ORIENTATIONS))
@pytest.mark.parametrize("kind", list(gl.PLAIN))
def test_torus_counts_give_the_unpacked_oracles_next_state(kind, name, G):
    """gl.next_cells from the torus counts against ol.unpacked_step (compute.wgsl restated: a torus at a power-of-two grid), every coded
    rule of every main neighbourhood."""
    u = gl.unpacked_state(G, name)
    cells = u.reshape(G, G, G).astype(np.uint8)
    n = gl.counts_of_cells(cells, torus=True)
    for rule in gl.coded(gl.TABLES[kind]):
        r = ol.Rules.from_strings(**gl.strings_of(kind, rule))
        want = ol.unpacked_step(G, u, r.main, r.survive, r.born)
        assert want.any() and (want != u).any()
        np.testing.assert_array_equal(gl.next_cells(cells, n, kind, rule).ravel(), want, err_msg=f"{gl.name_of(kind, rule)} on graded {name}")
    packed = gl.next_cells(cells, gl.counts_of_cells(cells), kind, gl.coded(gl.TABLES[kind])[0])
    assert (packed != gl.next_cells(cells, n, kind, gl.coded(gl.TABLES[kind])[0])).any()  # the dead faces would show


TORUS_FLOOR = 16  # the rarest pair: (alive, T) at 32^3, graded z


@pytest.mark.parametrize("G", [32, 64, 128])
@pytest.mark.parametrize("name", ["z", "x"])
def test_every_count_occurs_on_the_torus(G, name):
    """What test_gpu_unpacked_rule_tables.py rests on: every (alive, count) pair of T (27), F (7), E (13), C (9), F2 (5) and M2 (9) under
    torus counts, in the two states every id there starts from."""
    cells = gl.unpacked_state(G, name).reshape(G, G, G).astype(np.uint8)
    cov = gl.coverage_of_cells(cells, gl.counts_of_cells(cells, dtype=np.int8, torus=True))
    print(f"graded {name} at {G}^3, torus: smallest number of occurrences of an (alive, count) pair", {k: int(v.min()) for k, v in cov.items()})
    assert {k: v.shape for k, v in cov.items()} == {k: (2, N) for k, N in gl.SIZES.items()}
    for k, v in cov.items():
        assert v.min() >= TORUS_FLOOR, f"{k}: (alive, count) pair {np.unravel_index(v.argmin(), v.shape)} occurs {v.min()} times in graded {name} at {G}"


def _range_coverage(cells, ranges):
    cov = {k: np.zeros((2, N), dtype=np.int64) for k, N in gl.SIZES.items()}
    for lo, hi in ranges:
        alive, n = gl.cells_counts_of_planes(cells, lo, hi, dtype=np.int8, torus=True)
        for k, v in gl.coverage_of_cells(alive, n).items():
            cov[k] += v
    return cov


@pytest.mark.parametrize("G,name", [(256, "z"), (256, "x"), (512, "z"), (512, "x"), (1024, "x")])
def test_every_count_occurs_on_the_torus_at_the_larger_grids(G, name):
    """The same on a part of the planes (what occurs there occurs in the grid): four planes of a state graded along x, four around each
    of the eight density steps of one graded along z — and, at 1024, four planes of the plane array the thin slab there is cut from."""
    if G == 1024:
        cells, ranges = gl.graded_cells(G, "x", planes=21 + 4 * 3), [(14, 18)]  # (test_gpu_unpacked_rule_tables.THIN_1024: nz 21, K 3)
    else:
        cells = gl.graded_cells(G, *gl.ORIENTATIONS[name])
        ranges = [(b - 2, b + 2) for b in (-(-k * G // 9) for k in range(1, 9))] if name == "z" else [(G // 2, G // 2 + 4)]
    cov = _range_coverage(cells, ranges)
    print(f"graded {name} at {G}, torus, planes {ranges}: smallest number of occurrences", {k: int(v.min()) for k, v in cov.items()})
    for k, v in cov.items():
        assert v.min() >= 32, f"{k}: (alive, count) pair {np.unravel_index(v.argmin(), v.shape)} occurs {v.min()} times in graded {name} at {G}"
