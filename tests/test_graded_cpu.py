"""graded_lib without a GPU: the graded states reach every (alive, count) pair of every table often enough for a wrong leaf or a wrong
carry to show, and class_counts — the plain numpy restatement of the three neighbour classes — gives the oracle's next state under rules
that answer any two counts differently. Run with -s for the coverage figures."""
import numpy as np
import pytest

import graded_lib as gl
import oracle_lib as ol

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
    for N in (7, 27, 13, 9):
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
    return [(kind, r) for r in fam] if kind in ("vn", "moore") else [("clustered", gl.clustered(kind, r)) for r in fam]


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
        if kind in ("vn", "moore"):
            pin(64, "z", kind, r)
        else:
            pin(64, "z", "clustered", gl.clustered(kind, r))


def test_all_three_classes_at_once():
    for j in (0, 7):
        pin(64, "x", "clustered", gl.coded_all(j))
