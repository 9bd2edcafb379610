"""`ca3d_ensemble_isolate_connected` with CA3D_CONNECT_TORUS on the GPU (kernel ca_ensemble_isolate64_torus, csrc/ca_objects_torus.hip)
against `host.isolate(..., connectivity="torus")`, the numpy restatement of the definition in include/ca3d.h, with jobs taken from
`host.census(..., "torus")` and records from `host.state_summary` — never from the engine. Every comparison is exact: the destination's
states, populations, shifts and records, and the untouched source. The states are tests/objects_torus_cases.py's;
tests/test_isolate_torus_cpu.py checks the host definition itself."""
import ctypes as C
import re

import numpy as np
import pytest

import census_cases as cc
import objects_torus_cases as tc
import oracle_lib as ol
from cellularautomatons3d_amd import Ca3dError, _capi, host
from test_gpu_isolate import KINDS, check_record, hold
from test_gpu_moving import MOVING, SHIP, Trajectory, expected, glider, moore_rules

pytestmark = pytest.mark.gpu

G, W = 64, 8192
PLACEMENTS = ("keep", "centre", "origin")

_ISOLATED = {}


def isolated(key, words, cell, placement, connectivity="torus"):
    """`host.isolate(words, cell, placement, connectivity)`, kept under `key` (which names `words`) for the run and never changed."""
    k = (key, int(cell), placement, connectivity)
    if k not in _ISOLATED:
        w, pop, shift = host.isolate(words, int(cell), placement, connectivity)
        w.setflags(write=False)
        _ISOLATED[k] = (w, pop, shift)
    return _ISOLATED[k]


@pytest.fixture()
def ens():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


@pytest.fixture()
def nursery():
    from cellularautomatons3d_amd import Ensemble

    e = Ensemble(0)
    yield e
    e.close()


def isolate_and_check(dst, src, jobs, keys, states, placement, dst_first=0, copy_rules=False, connectivity="torus", asked=None):
    """One call; job k = (universe, cell) against isolated(keys[universe], states[universe], cell, placement, connectivity). `src` None:
    one handle. `asked`: what the call is given where that is not `connectivity` itself ("boundary")."""
    source = dst if src is None else src
    sources = sorted({u for u, _ in jobs})
    before = [(source.read_state(u, 1).tobytes(), source.summaries(u, 1)) for u in sources]
    pop, shift = dst.isolate(np.array(jobs, dtype=np.uint32).reshape(-1, 2), dst_first, src, placement, copy_rules, connectivity=asked or connectivity)
    n = len(jobs)
    assert pop.shape == (n,) and pop.dtype == np.uint32 and shift.shape == (n, 3) and shift.dtype == np.int32
    got, recs = dst.read_state(dst_first, n), dst.summaries(dst_first, n)
    for k, (u, cell) in enumerate(jobs):
        where = f"job {k}: universe {u} ({keys[u]}), cell {cell}, {placement}, {connectivity}"
        words, want_pop, want_shift = isolated(keys[u], states[u], cell, placement, connectivity)
        assert (int(pop[k]), tuple(int(v) for v in shift[k])) == (want_pop, want_shift), where
        np.testing.assert_array_equal(got[k], words, err_msg=where)
        check_record(recs[k], words, where)
    assert [(source.read_state(u, 1).tobytes(), source.summaries(u, 1)) for u in sources] == before  # the source is only read
    return pop, shift


def torus_jobs(keyed, picks=(0,)):
    """Every torus component of every state [(key, words)] as jobs (universe, cell): its first cell, and with picks (0, -1) also its
    last; the lists are complete on the reference's side. -> (jobs, the census record of each job)."""
    jobs, records = [], []
    for u, (key, w) in enumerate(keyed):
        comps, n, rest = tc.reference(key, w, 64)
        assert rest == 0, key
        for c in comps[:n]:
            cells = tc.cells_list(isolated(key, w, int(c["first_cell"]), "keep")[0])
            assert int(cells[0]) == int(c["first_cell"]) and cells.size == int(c["population"])
            for p in picks:
                jobs.append((u, int(cells[p])))
                records.append(c)
    return jobs, records


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("d", tc.ROLLS)
def test_rolled_crafted_states(ens, nursery, d, placement):
    """Every object of census_cases' states rolled across the word seam, a wave seam or a face, selected by its first and by its last
    cell. ORIGIN: the nursery's record carries the torus census record's digest — the device's own census of the same handle."""
    keyed = [((name, d), tc.state(name, d)) for name in tc.ROLLED]
    hold(ens, [w for _, w in keyed])
    jobs, records = torus_jobs(keyed, picks=(0, -1))
    assert len(jobs) == 2 * (3 + 1 + 1 + 1 + 2 + 3 + 3)
    nursery.configure(len(jobs), neighbourhood="von neumann")  # without COPY_RULES the two may differ in kind
    pop, shift = isolate_and_check(nursery, ens, jobs, [k for k, _ in keyed], [w for _, w in keyed], placement)
    got = nursery.read_state()
    for k in range(0, len(jobs), 2):
        assert got[k].tobytes() == got[k + 1].tobytes() and int(pop[k]) == int(records[k]["population"]) > 0
    if placement == "origin":
        comps, n, rest = ens.census(max_components=64, connectivity="torus")
        by_cell = {(u, int(c["first_cell"])): c for u in range(ens.n) for c in comps[u, :int(n[u])]}
        for k, s in enumerate(nursery.summaries()):
            rec = by_cell[(jobs[k - k % 2][0], jobs[k - k % 2][1])]
            assert rec.tobytes() == records[k].tobytes()
            assert s.digest == int(rec["digest"]) and s.population == int(rec["population"]), jobs[k]
            assert tuple(-int(v) for v in shift[k]) == host.unpack_box(rec["box_min"])
    assert nursery.isolate_gpu_ms() > 0.0


def test_rings_a_dead_cell_and_the_whole_universe(ens, nursery):
    """A ring around an axis is not moved along it; a ring with a gap is, modulo 64; a dead cell gives nothing; the full universe
    stays."""
    keyed = []
    for axis in range(3):
        keyed.append((("rod", axis, ()), host.cells_to_words(G, tc.rod(axis))))
        keyed.append((("rod", axis, (31, 32)), host.cells_to_words(G, tc.rod(axis, (31, 32)))))
    keyed += [("full", cc.state("full")), ("empty", cc.state("empty"))]
    hold(ens, [w for _, w in keyed])
    jobs = [(u, int(tc.cells_list(w)[17])) for u, (_, w) in enumerate(keyed[:7])] + [(7, 4711), (0, 0), (6, (1 << 18) - 1)]
    nursery.configure(len(jobs), neighbourhood="moore")
    for placement in PLACEMENTS:
        pop, shift = isolate_and_check(nursery, ens, jobs, [k for k, _ in keyed], [w for _, w in keyed], placement)
        assert [int(p) for p in pop] == [64, 62] * 3 + [G ** 3, 0, 0, G ** 3]
        assert not shift[6:].any() and not nursery.read_state(7, 2).any()
        for axis in range(3):
            assert int(shift[2 * axis][axis]) == 0
            want = {"keep": 0, "origin": -33, "centre": 1 - 33}[placement]  # the gapped ring's box starts at 33 and is 62 long
            assert int(shift[2 * axis + 1][axis]) == want
            if placement != "keep":  # the gapped ring arrives in one piece
                s = nursery.summaries(2 * axis + 1, 1)[0]
                assert s.box_max[axis] - s.box_min[axis] == 61 and s.box_min[axis] == 33 + want


SEAM_SHIPS = {
    # name -> (glider arguments, roll): the doubled glider astride the x seam (moving +x +y), the y seam (moving -y +z), the z seam
    # (moving +x +z), and astride all three at once
    "x": (("xy", (28, 30, 30), (False, False)), (34, 0, 0)),
    "y": (("yz", (40, 30, 12), (True, False)), (0, 33, 0)),
    "z": (("xz", (20, 20, 30), (False, False)), (0, 0, 33)),
    "xyz": (("xy", (28, 30, 30), (False, False)), (34, 33, 33)),
}


def test_gliders_astride_the_seams(ens, nursery):
    """The point of it: a glider caught halfway through a face of a torus universe. The torus census finds ONE object; isolated with
    CENTRE into a reference-boundary nursery with its rule, step_until_moving names it MOVING with the glider's true shift. The closed
    isolate of the same cell gives a fragment that does not move."""
    rules = moore_rules(*SHIP)
    names = list(SEAM_SHIPS)
    whole = [glider(*SEAM_SHIPS[k][0]) for k in names]
    states = [tc.rolled(w, SEAM_SHIPS[k][1]) for w, k in zip(whole, names)]
    hold(ens, states)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    ens.set_boundary("torus")
    comps, n, rest = ens.census(max_components=8, connectivity="boundary")
    closed = ens.census(max_components=8)
    jobs = []
    for u, k in enumerate(names):
        want = tc.reference(("seam ship", k), states[u], 8)
        assert (int(n[u]), int(rest[u])) == (1, 0) == want[1:] and comps[u].tobytes() == want[0].tobytes(), k
        assert int(comps[u, 0]["population"]) == 10 and int(closed[1][u]) >= 2, k
        jobs.append((u, int(comps[u, 0]["first_cell"])))
    assert comps[3, 0]["digest"] == comps[0, 0]["digest"] == host.census(whole[0], 1)[0][0]["digest"]
    nursery.configure(2 * len(jobs), neighbourhood="moore")
    assert nursery.boundary == "reference"
    keys = [("seam ship", k) for k in names]
    pop, shift = isolate_and_check(nursery, ens, jobs, keys, states, "centre", copy_rules=True, asked="boundary")  # the source's boundary: torus
    isolate_and_check(nursery, ens, jobs, keys, states, "centre", dst_first=len(jobs), copy_rules=True, connectivity="closed")
    centred = nursery.read_state()
    for u, k in enumerate(names):  # in one piece: what the closed isolate makes of the glider clear of the faces
        np.testing.assert_array_equal(centred[u], host.isolate(whole[u], int(tc.cells_list(whole[u])[0]), "centre")[0])
    done, reason, period, moved = nursery.step_until_moving(64, check_every=4)
    true_shift = {"x": (1, 1, 0), "y": (0, -1, 1), "z": (1, 0, 1), "xyz": (1, 1, 0)}
    for u, k in enumerate(names):
        for which, connectivity in ((u, "torus"), (len(jobs) + u, "closed")):
            t = Trajectory(isolated(keys[u], states[u], jobs[u][1], "centre", connectivity)[0], rules)
            want = expected(t, 0, 64, 4, 15, False)
            assert (int(done[which]), int(reason[which]), int(period[which]), tuple(int(v) for v in moved[which])) == want, (k, connectivity)
        assert (int(reason[u]), int(period[u]), tuple(int(v) for v in moved[u])) == (MOVING, 4, true_shift[k]), k
        assert not int(reason[len(jobs) + u]) & MOVING and int(pop[u]) == 10, k


@pytest.mark.parametrize("kind", list(KINDS))
def test_rules_follow_the_source(ens, nursery, kind):
    """2, 6 and 1 rule words a universe: source universes alternate between two rules, the nursery takes them in another order, and
    after four steps every nursery universe is the oracle's under ITS source's rule."""
    conf, two = KINDS[kind]
    nb = conf["neighbourhood"]
    d = tc.ROLLS[1]
    keyed = [((name, d), tc.state(name, d)) for name in ("shell_core", "shapes", "staircase", "corners")]
    ens.configure(4, **conf)
    ens.upload_state(0, np.stack([w for _, w in keyed]))
    for u in range(4):
        ens.set_rule_strings(u, neighbourhood=nb, **two[u % 2])
    every, _ = torus_jobs(keyed)
    jobs = [every[i] for i in (5, 0, 3, 1, 6, 2)]
    nursery.configure(len(jobs), **conf)
    isolate_and_check(nursery, ens, jobs, [k for k, _ in keyed], [w for _, w in keyed], "centre", copy_rules=True)
    nursery.step(4)
    got = nursery.read_state()
    differ = 0
    for k, (u, cell) in enumerate(jobs):
        start = isolated(keyed[u][0], keyed[u][1], cell, "centre")[0]
        want = ol.packed_run(G, start, ol.Rules.from_strings(neighbourhood=nb, **two[u % 2]), 4)
        np.testing.assert_array_equal(got[k], want, err_msg=f"job {k} under rule {two[u % 2]}")
        differ += not np.array_equal(want, ol.packed_run(G, start, ol.Rules.from_strings(neighbourhood=nb, **two[1 - u % 2]), 4))
    assert differ  # the two rules tell the universes apart: a nursery that took the wrong one would show
    assert [s.step for s in nursery.summaries()] == [4] * len(jobs)


def test_one_handle(ens):
    """Sources and destinations in one ensemble, on one stream."""
    d = tc.ROLLS[0]
    keyed = [((name, d), tc.state(name, d)) for name in ("shapes", "shell_core", "corners")]
    states = [w for _, w in keyed] + [cc.state("full")] * 6
    hold(ens, states)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    jobs, _ = torus_jobs(keyed)
    assert len(jobs) == 6
    isolate_and_check(ens, None, jobs, [k for k, _ in keyed], states, "centre", dst_first=3, copy_rules=True)
    got = ens.read_state()
    for u in range(3):
        np.testing.assert_array_equal(got[u], states[u])


def test_scale_and_a_range(ens, nursery):
    """300 jobs, more than compute units, into universes 7 .. 306 of 310: the ten universes around the range keep what they held."""
    keyed = [((name, d), tc.state(name, d)) for d in tc.ROLLS for name in tc.ROLLED if name != "serpentine"]
    hold(ens, [w for _, w in keyed])
    every, _ = torus_jobs(keyed)
    jobs = [every[k % len(every)] for k in range(300)]
    marker = host.random_fill(W, seed=5, and_rounds=3)
    nursery.configure(310, neighbourhood="moore")
    nursery.upload_state(0, np.stack([marker] * 7))
    nursery.upload_state(307, np.stack([marker] * 3))
    isolate_and_check(nursery, ens, jobs, [k for k, _ in keyed], [w for _, w in keyed], "centre", dst_first=7)
    for u in (0, 6, 307, 309):
        np.testing.assert_array_equal(nursery.read_state(u, 1)[0], marker)
        check_record(nursery.summaries(u, 1)[0], marker, u)


def test_closed_through_the_new_entry_point(ens, nursery):
    """CA3D_CONNECT_CLOSED is ca3d_ensemble_isolate: the same states, records and results, on states whose objects lie on faces."""
    lib = _capi.load()
    d = tc.ROLLS[1]
    keyed = [((name, d), tc.state(name, d)) for name in ("shapes", "corners", "shell_core")]
    hold(ens, [w for _, w in keyed])
    jobs_list, _ = torus_jobs(keyed)
    jobs = (_capi.IsolateJobStruct * len(jobs_list))()
    for k, (u, c) in enumerate(jobs_list):
        jobs[k].universe, jobs[k].cell = u, c
    nursery.configure(len(jobs_list), neighbourhood="moore")
    for flags in (0, 1, 2):
        results = []
        for new in (False, True):
            out = (_capi.IsolatedStruct * len(jobs_list))()
            args = (nursery._h, 0, ens._h, len(jobs_list), jobs, flags)
            rc = lib.ca3d_ensemble_isolate_connected(*args, 0, out, None) if new else lib.ca3d_ensemble_isolate(*args, out, None)
            assert rc == 0
            results.append((bytes(out), nursery.read_state().tobytes(), nursery.summaries()))
        assert results[0] == results[1]
        got = np.frombuffer(results[1][1], dtype=np.uint32).reshape(len(jobs_list), W)
        for k, (u, c) in enumerate(jobs_list):
            np.testing.assert_array_equal(got[k], isolated(keyed[u][0], keyed[u][1], c, PLACEMENTS[flags], "closed")[0])


def test_refusals(ens, nursery):
    lib = _capi.load()
    out = (_capi.IsolatedStruct * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    ms = C.c_float(-1.0)
    KEEP, CENTRE, ORIGIN, COPY, TORUS = 0, 1, 2, 0x100, 1

    def jobs_of(*pairs):
        j = (_capi.IsolateJobStruct * max(len(pairs), 1))()
        for k, (u, c) in enumerate(pairs):
            j[k].universe, j[k].cell = u, c
        return j

    watched = []  # the ensembles that hold a state everywhere: compared before and after every refusal

    def snapshot(e):
        return (e.read_state().tobytes(), e.summaries())

    def refused(code, pattern, dst, dst_first, src, n_jobs, jobs, flags, connectivity=TORUS):
        before = [snapshot(e) for e in watched]
        rc = lib.ca3d_ensemble_isolate_connected(dst._h if dst else None, dst_first, src._h if src else None, n_jobs, jobs, flags, connectivity, out,
                                                 C.byref(ms))
        msg = lib.ca3d_last_error().decode()
        assert rc == code, (rc, msg)
        assert re.search(pattern, msg), msg
        assert bytes(out) == b"\x5a" * C.sizeof(out) and ms.value == -1.0, msg
        assert [snapshot(e) for e in watched] == before, msg

    two = jobs_of((0, 0), (1, 5))
    refused(-1, "NULL", None, 0, ens, 2, two, CENTRE)
    refused(-1, "NULL", nursery, 0, None, 2, two, CENTRE)
    refused(-2, "configure.*destination", nursery, 0, ens, 2, two, CENTRE)
    nursery.configure(4, neighbourhood="moore")
    refused(-2, "configure.*source", nursery, 0, ens, 2, two, CENTRE)
    ens.configure(3, neighbourhood="moore")
    nursery.upload_state(0, np.stack([cc.state("shapes")] * 4))
    watched.append(nursery)
    refused(-1, "NULL", nursery, 0, ens, 2, None, CENTRE)
    refused(-2, "job 0.*universe 0", nursery, 0, ens, 2, two, CENTRE)  # no state anywhere
    ens.upload_state(0, cc.state("shell_core")[None])
    refused(-2, "job 1.*universe 1", nursery, 0, ens, 2, two, CENTRE)  # universe 1 has none
    ens.upload_state(1, np.stack([cc.state("corners")] * 2))
    watched.append(ens)
    refused(-1, "jobs", nursery, 0, ens, 0, two, CENTRE)               # no job
    refused(-1, "jobs", nursery, 3, ens, 2, two, CENTRE)               # more than fit behind dst_first
    refused(-1, "jobs", nursery, 4, ens, 1, two, CENTRE)
    refused(-1, "job 1.*universe 3", nursery, 0, ens, 2, jobs_of((0, 0), (3, 0)), CENTRE)
    refused(-1, "job 1.*cell 262144", nursery, 0, ens, 2, jobs_of((0, 0), (1, 1 << 18)), CENTRE)
    refused(-1, "placement 3", nursery, 0, ens, 2, two, 3)
    refused(-1, "flags", nursery, 0, ens, 2, two, CENTRE | 0x200)
    refused(-1, "flags", nursery, 0, ens, 2, two, ORIGIN | 1 << 31)
    refused(-1, r"connectivity 2\b", nursery, 0, ens, 2, two, CENTRE, 2)
    refused(-1, r"connectivity 256\b", nursery, 0, ens, 2, two, CENTRE, 0x100)
    # one handle: a source among the destinations
    refused(-1, "job 1.*universe 1.*destinations", ens, 1, ens, 2, two, KEEP)
    refused(-1, "job 0.*universe 2.*destinations", ens, 2, ens, 1, jobs_of((2, 0)), KEEP)
    # COPY_RULES: no rules on the source, then ensembles of different kinds
    refused(-2, "job 0.*set_rules.*universe 0", nursery, 0, ens, 2, two, CENTRE | COPY)
    ens.set_rule_strings(0, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    refused(-2, "job 1.*set_rules.*universe 1", nursery, 0, ens, 2, two, CENTRE | COPY)
    ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=SHIP[0], survive=SHIP[1])
    for conf in (dict(neighbourhood="von neumann"), dict(neighbourhood="moore", clustered=True)):
        nursery.configure(4, **conf)
        nursery.upload_state(0, np.stack([cc.state("shapes")] * 4))
        refused(-5, "COPY_RULES", nursery, 0, ens, 2, two, CENTRE | COPY)
    # the Python face
    with pytest.raises(ValueError):
        nursery.isolate([(0, 0)], connectivity="open")
    with pytest.raises(Ca3dError) as e:
        nursery.isolate(np.zeros((0, 2), dtype=np.uint32), 0, ens, connectivity="torus")
    assert e.value.code == -1
    # and the call that is not refused: out and gpu_ms may be NULL. The corners' eight cells are one object of the torus
    good = jobs_of((1, 63), (1, 5))  # the corner (63, 0, 0); a dead cell of `corners`
    assert lib.ca3d_ensemble_isolate_connected(nursery._h, 2, ens._h, 2, good, CENTRE, TORUS, None, None) == 0
    assert bytes(out) == b"\x5a" * C.sizeof(out)
    assert lib.ca3d_ensemble_isolate_connected(nursery._h, 0, ens._h, 2, good, ORIGIN, TORUS, out, C.byref(ms)) == 0
    assert ms.value > 0.0
    cube = host.isolate(cc.state("corners"), 63, "origin", "torus")
    assert (out[0].population, tuple(out[0].shift)) == (cube[1], cube[2]) == (8, (-63, -63, -63))
    assert (out[1].population, tuple(out[1].shift)) == (0, (0, 0, 0))
    got = nursery.read_state()
    np.testing.assert_array_equal(got[0], cube[0])
    np.testing.assert_array_equal(got[0], host.cells_to_words(G, [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]))
    assert not got[1].any() and not got[3].any()
