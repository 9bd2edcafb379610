"""Ensemble against the path that existed before it: B universes of 64^3 in ONE launch of ca_ensemble_vn64 (Ensemble.step) vs. the same
universes stepped one after another through one Engine at 64^3 (Engine.step: the resident one-workgroup kernel compiled for the rule).

For B = 1, 256, 1024, 4096 and 256 steps per launch (random fills, rule B2,4 / S1,3,5, which never settles): microseconds per launch,
universe-steps per second, Tcells per second, for both paths and their ratio. Same machine, same process, the two paths alternating,
after the final states of both have been compared. The baseline is timed at its best: B back-to-back step(256) calls on an engine that
already holds a state, one synchronisation at the end — no upload, no summary and no read-back per universe, all of which a real sweep
through one engine would pay on top.

    python tools/bench_ensemble.py --out profiles/ensemble_64.json --commit <hash>

--neighbourhood moore measures a Moore ensemble (ca_ensemble_moore64, rule B5-7 / S4-6) against the same sweep through one Engine, which
for a Moore rule at 64^3 is one launch per step of the kernel compiled for the rule; same protocol, written to
profiles/ensemble_moore_64.json unless --out says otherwise.

--neighbourhood clustered measures a clustered ensemble (ca_ensemble_clustered64, three table pairs a universe, bench.py's `clustered` rule:
Moore B5-7 / S4-7, edges B4 / S3-5, corners B3 / S2-4) against the same universes one after another through one Engine, which steps that
rule at 64^3 with the class kernel compiled for it; same protocol, written to profiles/ensemble_clustered_64.json unless --out says
otherwise.

--cycle measures what watching CA3D_STOP_PERIODIC costs, for both neighbourhoods: Ensemble.step_until_cycle (stop mask 7, the *_cycle
kernels) against Ensemble.step_until (stop mask 3, the kernels above) on the same universes — B = 256 and 1024, 256 steps, check_every 1
and 8, density-1/2 fills on which nothing stops within the call, so every check is paid. Before timing, both calls must have left the same
states with every universe still running; then the two alternate from freshly uploaded states and the medians of the hipEvent time around
the launch (Ensemble.stats) and of the host clock around the call are reported. Written to profiles/ensemble_cycle_64.json unless --out
says otherwise.

--moving measures what watching CA3D_STOP_MOVING costs on top of that, for the three kernels (von Neumann, Moore, and clustered holding the
Moore rule with silent side tables — the rule is data, the kernel's work does not depend on it, and bench.py's clustered rule lets
universes stop within the call): Ensemble.step_until_moving (stop mask 15, the *_moving kernels: a population and bounding-box reduction on every check's
barrier) against Ensemble.step_until_cycle (stop mask 7, the *_cycle kernels) on the same universes, built like --cycle: B = 256 and 1024,
256 steps, check_every 1 and 8, density-1/2 fills on which nothing stops, the same verification, medians of the hipEvent time. Written to
profiles/ensemble_moving_64.json unless --out says otherwise.

--trace measures what a population curve costs, for both neighbourhoods: (a) Ensemble.step_trace(steps, check_every, stop mask 0) — the
*_trace kernels write one sample (population, births, deaths) per check point and universe — against (b) the path without it, K - 1
rounds of ca3d_ensemble_step(check_every) + ca3d_ensemble_summarize collecting the same three numbers from the records (through the C
ABI into one preallocated array, no Python object per record: the loop at its best), and (c) a plain step(steps) as the floor — B = 256
and 1024, 256 steps, check_every 1 and 8, density-1/2 fills. Before timing, (a) and (b) must give identical arrays; then the three
alternate from freshly uploaded states and the medians of the hipEvent time around the launches (Ensemble.stats; (b): summed over its
launches, in a run of its own) and of the host clock around the call are reported with their spread. The host clock is the fair one for (b), whose cost is
its synchronisations. Written to profiles/ensemble_trace_64.json unless --out says otherwise; the tool fails when (a) does not beat
(b) by the host clock by more than the spread, after the file is written.

--sheet measures the contact sheet (ca3d_ensemble_render_sheet, kernel ca_render_sheet64: every universe drawn as a tile, one launch)
against the loop it replaces: one Engine at 64^3 and, per universe, upload_state from a host array plus ca3d_render with a host
presentation pointer (the engine's default options). B = 256 and 1024 universes seeded with and_rounds 4 (a different seed each),
camera host.orbit_camera(), tiles 64 x 64 and 128 x 128 at 1 and 4 samples. Before timing, sampled tiles must equal the engine's
"render_skip" 0 frames byte for byte. Reported: medians of --repeats measurements of the sheet's hipEvent time (Ensemble.sheet_stats)
and of the host clock around a call that reads the presentation sheet back, and of the host clock around the loop. No ratio is
required. Written to profiles/ensemble_sheet_64.json unless --out says otherwise.

--census measures the census (ca3d_ensemble_census, kernel ca_ensemble_census64: every universe's connected objects listed in one
launch) against the path that exists without it: read_state of the same universes plus labelling on the CPU (scipy.ndimage.label with a
full 3 x 3 x 3 structure when scipy can be imported, else host.census; the profile says which). B = 256 and 1024 universes of ash —
seed_states (seeds 1 .. B), then step_until_cycle(512) under Moore B5-7 / S4-6 (and_rounds 2) and under Moore B6 / S5-7 (and_rounds 1),
what a soup search would census — and of two synthetic states in every universe: host.seeded_state(64, 0xCA3D0009, 8) (509 objects of
518 cells) and host.seeded_state(64, 77, 2, box 20 .. 43) (190 objects, one of 1 306 cells); max_components 1024. Before timing, the
census must equal the CPU path's components (population, first cell, box, order) in every universe and host.census byte for byte,
digests included, in sampled ones. Reported: medians of --repeats measurements of the census' hipEvent time and of the host clock around
the call, of read_state alone, and of read_state + labelling. No ratio is required. Written to profiles/ensemble_census_64.json unless
--out says otherwise.

--census-torus measures the torus forms of census and isolate (ca3d_ensemble_census_connected / ca3d_ensemble_isolate_connected with
CA3D_CONNECT_TORUS, kernels ca_ensemble_census64_torus / ca_ensemble_isolate64_torus) against the closed forms on the same universes in
the same run: the ash of --census produced under the torus boundary, B = 256 and 1024, the census launch and the isolate launch of all
census objects under each connectivity, the two alternating. Both are checked against host.census / host.isolate in three sampled
universes first. Reported: medians of --repeats hipEvent times, their ratios, and the object counts under the two connectivities. No ratio
is required. Written to profiles/ensemble_census_torus_64.json unless --out says otherwise.

--isolate measures the isolate (ca3d_ensemble_isolate, kernel ca_ensemble_isolate64: objects a census named, each made the only thing
in a universe of its own, centred, with its source's rule) on the ash workload of --census (Moore B6 / S5-7, and_rounds 1, seeds 1 .. B,
step_until_cycle(512)): a census at max_components 1024, then EVERY object of the B = 256 universes isolated into a second ensemble in
one call. Against the loop it replaces on the same objects: per universe read_state and a labelling on the CPU (scipy.ndimage.label
with a full 3 x 3 x 3 structure when scipy can be imported — one labelling a universe, the objects cut out of it — else host.isolate per
object; the profile says which), per object the centred state built with numpy and upload_state into the second ensemble. Before timing,
the isolated states, populations and shifts must equal host.isolate for every object of sampled universes, and after the loop the second
ensemble must hold what the call left there. Reported: medians of --repeats measurements of the call's hipEvent time, of the host clock
around the call, and of the host clock around the loop. No ratio is required. Written to profiles/ensemble_isolate_64.json unless --out
says otherwise.

--compose measures the compose (ca3d_ensemble_compose, kernel ca_ensemble_compose64: whole universes staged, turned and shifted, into
universes of their union) on the objects of --isolate: the ash of B = 256 universes, a census, EVERY object isolated (centred) into a
nursery whose last universe holds a 2 x 2 x 2 block, then one destination an object, each of two parts — the object, turned, and the
block — in one call. Three mixes of orientations: all 48 (k % 48), the eight that leave x on x, and the other forty; and, beside them,
one part at orientation 0 (the bytes isolate writes) and the isolate launch on the same objects; and the dense case, 4096 destinations
of one whole soup each (and_rounds 1), for the eight and for the forty, without a loop beside it. Against the loop it replaces on the same
layouts, on the first --loop-destinations destinations: read_state of the sources, host.compose, upload_state. Before timing, states
and records must equal host.compose in sampled destinations, and after the loop the destinations must hold what the call left there.
Reported: medians of --repeats measurements. No ratio is required. Written to profiles/ensemble_compose_64.json unless --out says
otherwise.

--canon measures the canon (ca3d_ensemble_canon, kernel ca_ensemble_canon64: a universe's key up to the 48 orientations and translation,
its orientation and its symmetry group) on two workloads: the objects of --isolate — the ash of B = 256 universes, a census, EVERY object
isolated (centred) into a nursery, then ONE call over the nursery — and B dense soups (and_rounds 1). For each: the launch's hipEvent
time without and with the digests array, the host clock around the call, the census launch on the same universes for scale, and the
loop the call replaces — read_state and host.canon — on the first --loop-destinations universes ONLY (1 024 by default); for the ash,
the number of distinct census digests against the number of distinct keys, which is the point of it. Before timing, records and all 48
digests must equal host.canon in sampled universes, and every loop's keys must equal the call's. Reported: medians of --repeats
measurements. No ratio is required. Written to profiles/ensemble_canon_64.json unless --out says otherwise.

--canon-period measures canon over a period (ca3d_ensemble_canon_period, kernels ca_ensemble_canon_period_moore64 ...: the smallest
canon key over the phases of a period stepped INSIDE the launch, and whether the period closes) against Ensemble.canon_phases, the
Python loop it replaces (per phase a canon launch and a step launch; it leaves the ensemble max(periods) steps further), on the
nursery of --canon with periods all 4 and all 1, and on B dense soups (and_rounds 1, the ash's rule) with periods all 4. For each: the
launch's hipEvent time and the host clock around the call; canon_phases' host clock and its summed hipEvent time, period x (canon
launch + step launch), measured by the same loop written out; for period 1 the plain canon launch beside it, the price of carrying the
step's registers and LDS. The universes are put back before every measurement. Before timing, records and keys must equal
host.canon_period of the CPU oracle's phases in sampled universes, and canon_phases' key, phase, orientation and symmetry must equal
the call's everywhere. Reported: medians of --repeats measurements. No ratio is required. Written to
profiles/ensemble_canon_period_64.json unless --out says otherwise.

--envelope measures the envelope over a period (ca3d_ensemble_envelope, kernel ca_ensemble_envelope_moore64: envelope, stator, rotor
and heat over a period stepped INSIDE the launch) against the loop it replaces — per phase read_state + step(1), numpy OR / AND and
popcounts on the host — run on a copy of the same universes in the same process: the nursery of --canon with periods all 4, and B dense
soups (and_rounds 1, the ash's rule) with periods all 4. For each: the launch's hipEvent time and the host clock around the call; the
loop's host clock and the summed hipEvent time of its step launches. Before timing, the records must equal host.envelope in sampled
universes, and every loop's heat, envelope and stator populations must equal the call's everywhere. Reported: medians of --repeats
measurements. No ratio is required. Written to profiles/ensemble_envelope_64.json unless --out says otherwise.

--usage measures rule usage (ca3d_ensemble_usage, kernels ca_ensemble_usage_{vn,moore,clustered}64: which table entries a run reads,
one launch) against the loop it replaces — per step read_state, the neighbour counts and a bincount per universe in numpy, step(1), run
on --loop-samples steps and scaled — and against the floor, one plain step(--steps) launch of the same ensemble. Before timing, the
records must equal host.usage in sampled universes over 3 steps, and the loop's histograms the call's. Writes
profiles/ensemble_usage_64.json unless --out says otherwise.

--damage measures damage spreading (ca3d_ensemble_damage, kernels ca_ensemble_damage_{vn,moore,clustered}64: a universe and its twin
with one random cell flipped, stepped side by side INSIDE one launch, their Hamming distance at every step) for all three kinds at
B = 256 and 1024 over --steps steps, with the curve: the launch's hipEvent time and the host clock around the call. First against the
loop it replaces — two ensembles kept in lock step, per sample step(1) on each, read_state of both, numpy XOR and byte-table popcounts on
the host — run on --loop-samples samples and scaled to --steps (the loop's cost a sample does not depend on the sample). Second against
the floor: two plain step(--steps) launches of the same kind on the same two ensembles, one after the other, their hipEvent times summed, since damage does
twice the stepping. Before timing, the records and curves must equal host.damage in sampled universes over 3 steps, and the loop's
distances must equal the call's curve in every universe. Reported: medians of --repeats measurements. No ratio is required. Written to
profiles/ensemble_damage_64.json unless --out says otherwise.

With --boundary: the plain step kernel of each new boundary mode (Ensemble.set_boundary: "torus", "closed") against the reference
boundary's kernel on the same universes, for all three kinds (von Neumann, Moore, clustered) at B = 256 and 1024: Ensemble.step(--steps)
from the same uploaded fills, the modes alternating inside one process, hipEvent times. Before timing, the state of sampled universes
after 3 steps must equal host.ensemble_step's under every mode. Reported: medians of --repeats measurements and the ratio to the
reference's. No ratio is required. Written to profiles/ensemble_boundary_64.json unless --out says otherwise.

Needs an MI355X; without one the engines cannot be created and the tool fails.
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cellularautomatons3d_amd import Engine, Ensemble, _capi, host  # noqa: E402

G, W, CELLS = 64, 8192, 64 ** 3
RULES = {"von neumann": ("2,4", "1,3,5"), "moore": ("5-7", "4-6")}  # born, survive
KERNELS = {"von neumann": "ca_ensemble_vn64", "moore": "ca_ensemble_moore64"}
# bench.py's `clustered` rule: the keyword arguments of set_rule_strings
CLUSTERED = dict(neighbourhood="moore", born="5-7", survive="4-7", born_edges="4", survive_edges="3-5", born_corners="3", survive_corners="2-4")


def fills(B):
    return np.stack([host.random_fill(W, seed=1 + u) for u in range(B)])


def verify(ens, eng, words, steps, sample):
    """Final states of the ensemble against the engine's, universe by universe (the engine itself is checked against the CPU oracle
    by the test suite)."""
    ens.upload_state(0, words)
    ens.step(steps)
    got = ens.read_state()
    for u in sample:
        eng.upload_state(words[u])
        eng.step(steps)
        if not np.array_equal(got[u], eng.read_state()):
            raise SystemExit(f"universe {u}: the ensemble and the engine disagree after {steps} steps")


def timed(fn, sync, min_seconds):
    """Seconds per call of fn: enough calls for min_seconds of work, one synchronisation at the end."""
    fn(); sync()
    t0 = time.perf_counter(); fn(); sync()
    once = time.perf_counter() - t0
    reps = max(1, int(min_seconds / max(once, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def boundary_rows(args):
    """Ensemble.step under "torus" and "closed" against "reference": one row per (kernel, B)."""
    from cellularautomatons3d_amd.ensemble import BOUNDARIES

    def masks(s, bits):
        return sum(1 << v for v in host.rules_components_to_values(s)) & ((1 << bits) - 1)

    ens = Ensemble(0)
    rows = []
    for kind in ("von neumann", "moore", "clustered"):
        clustered = kind == "clustered"
        nb = "moore" if clustered else kind
        if clustered:
            keys = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")
            tables = ([masks(CLUSTERED[keys[2 * i]], b) for i, b in enumerate((27, 13, 9))], [masks(CLUSTERED[keys[2 * i + 1]], b) for i, b in enumerate((27, 13, 9))])
        else:
            tables = (masks(RULES[nb][0], 27 if nb == "moore" else 7), masks(RULES[nb][1], 27 if nb == "moore" else 7))
        for B in args.universes:
            words = fills(B)
            ens.configure(B, neighbourhood=nb, clustered=clustered)
            if clustered:
                ens.set_clustered_tables(0, tables[0], tables[1])
            else:
                ens.set_rule_tables(0, tables[0], tables[1])
            sample = sorted({0, B // 2, B - 1})
            for mode in BOUNDARIES:
                ens.set_boundary(mode)
                ens.upload_state(0, words)
                ens.step(3)
                got = ens.read_state()
                for u in sample:
                    want = words[u]
                    for _ in range(3):
                        want = host.ensemble_step(want, kind, tables, mode)
                    if not np.array_equal(got[u], want):
                        raise SystemExit(f"{kind} B={B} {mode}: universe {u} differs from host.ensemble_step after 3 steps")

            def call(mode):
                """One step call from the uploaded fills -> event ms."""
                ens.set_boundary(mode)
                ens.upload_state(0, words)
                ens.step(args.steps)
                ens.synchronize()
                return ens.stats().gpu_ms

            for mode in BOUNDARIES:
                call(mode)  # warm-up: every kernel has run once
            times = {mode: [] for mode in BOUNDARIES}
            for _ in range(args.repeats):
                for mode in BOUNDARIES:
                    times[mode].append(call(mode))
            med = {mode: statistics.median(t) for mode, t in times.items()}
            row = {"kernel": kind, "universes": B, "steps": args.steps, "states_verified": len(sample)}
            for mode in BOUNDARIES:
                row[mode] = {"event_us": med[mode] * 1e3, "event_us_min_max": [min(times[mode]) * 1e3, max(times[mode]) * 1e3],
                             "cell_steps_per_s": B * CELLS * args.steps / (med[mode] * 1e-3)}
            row["torus_over_reference_event"] = med["torus"] / med["reference"]
            row["closed_over_reference_event"] = med["closed"] / med["reference"]
            rows.append(row)
            print(json.dumps(row))
    ens.close()
    return rows


def cycle_rows(args):
    """step_until_cycle (mask 7) against step_until (mask 3): one row per (neighbourhood, B, check_every)."""
    ens = Ensemble(0)
    rows = []
    for nb in ("von neumann", "moore"):
        born, survive = RULES[nb]
        for B in args.universes:
            words = fills(B)
            ens.configure(B, neighbourhood=nb)
            ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood=nb, born=born, survive=survive)
            for every in (1, 8):
                def call(cycle):
                    """One call from the uploaded fills -> (event ms, wall ms, steps_done, reason)."""
                    ens.upload_state(0, words)
                    t0 = time.perf_counter()
                    out = ens.step_until_cycle(args.steps, check_every=every, stop_mask=7) if cycle else ens.step_until(args.steps, check_every=every, stop_mask=3)
                    wall = (time.perf_counter() - t0) * 1e3
                    return ens.stats().gpu_ms, wall, out[0], out[1]

                _, _, done, reason = call(True)
                with_cycle = ens.read_state()
                _, _, done0, reason0 = call(False)
                if not np.array_equal(with_cycle, ens.read_state()):
                    raise SystemExit(f"{nb} B={B} check_every={every}: step_until_cycle and step_until left different states")
                if reason.any() or reason0.any() or (done != args.steps).any() or (done0 != args.steps).any():
                    raise SystemExit(f"{nb} B={B} check_every={every}: a universe stopped within {args.steps} steps — not every check would be paid")
                tc, tp = [], []
                for _ in range(args.repeats):
                    tc.append(call(True)[:2])
                    tp.append(call(False)[:2])
                ev_c, ev_p = statistics.median(t[0] for t in tc), statistics.median(t[0] for t in tp)
                wall_c, wall_p = statistics.median(t[1] for t in tc), statistics.median(t[1] for t in tp)
                row = {"neighbourhood": nb, "universes": B, "steps": args.steps, "check_every": every,
                       "step_until_cycle": {"event_us": ev_c * 1e3, "event_us_min_max": [min(t[0] for t in tc) * 1e3, max(t[0] for t in tc) * 1e3], "wall_us": wall_c * 1e3},
                       "step_until": {"event_us": ev_p * 1e3, "event_us_min_max": [min(t[0] for t in tp) * 1e3, max(t[0] for t in tp) * 1e3], "wall_us": wall_p * 1e3},
                       "cycle_over_plain_event": ev_c / ev_p, "cycle_over_plain_wall": wall_c / wall_p, "states_verified": B}
                rows.append(row)
                print(json.dumps(row))
    ens.close()
    return rows


def moving_rows(args):
    """step_until_moving (mask 15) against step_until_cycle (mask 7): one row per (kernel, B, check_every)."""
    ens = Ensemble(0)
    rows = []
    for kind in ("von neumann", "moore", "clustered"):
        clustered = kind == "clustered"
        nb = "moore" if clustered else kind
        rule = dict(neighbourhood=nb, born=RULES[nb][0], survive=RULES[nb][1])  # clustered: the Moore rule, both side tables silent
        for B in args.universes:
            words = fills(B)
            ens.configure(B, neighbourhood=nb, clustered=clustered)
            ens.set_rule_strings(_capi.ENSEMBLE_ALL, **rule)
            for every in (1, 8):
                def call(moving):
                    """One call from the uploaded fills -> (event ms, wall ms, steps_done, reason)."""
                    ens.upload_state(0, words)
                    t0 = time.perf_counter()
                    out = ens.step_until_moving(args.steps, check_every=every, stop_mask=15) if moving else ens.step_until_cycle(args.steps, check_every=every, stop_mask=7)
                    wall = (time.perf_counter() - t0) * 1e3
                    return ens.stats().gpu_ms, wall, out[0], out[1]

                _, _, done, reason = call(True)
                with_moving = ens.read_state()
                _, _, done0, reason0 = call(False)
                if not np.array_equal(with_moving, ens.read_state()):
                    raise SystemExit(f"{kind} B={B} check_every={every}: step_until_moving and step_until_cycle left different states")
                if reason.any() or reason0.any() or (done != args.steps).any() or (done0 != args.steps).any():
                    raise SystemExit(f"{kind} B={B} check_every={every}: a universe stopped within {args.steps} steps — not every check would be paid")
                tm, tc = [], []
                for _ in range(args.repeats):
                    tm.append(call(True)[:2])
                    tc.append(call(False)[:2])
                ev_m, ev_c = statistics.median(t[0] for t in tm), statistics.median(t[0] for t in tc)
                wall_m, wall_c = statistics.median(t[1] for t in tm), statistics.median(t[1] for t in tc)
                row = {"kernel": kind, "universes": B, "steps": args.steps, "check_every": every,
                       "step_until_moving": {"event_us": ev_m * 1e3, "event_us_min_max": [min(t[0] for t in tm) * 1e3, max(t[0] for t in tm) * 1e3], "wall_us": wall_m * 1e3},
                       "step_until_cycle": {"event_us": ev_c * 1e3, "event_us_min_max": [min(t[0] for t in tc) * 1e3, max(t[0] for t in tc) * 1e3], "wall_us": wall_c * 1e3},
                       "moving_over_cycle_event": ev_m / ev_c, "moving_over_cycle_wall": wall_m / wall_c, "states_verified": B}
                rows.append(row)
                print(json.dumps(row))
    ens.close()
    return rows


def trace_rows(args):
    """step_trace against the step + summaries loop and against plain stepping: one row per (neighbourhood, B, check_every)."""
    import ctypes as C

    lib = _capi.load()
    ens = Ensemble(0)
    rows = []
    for nb in ("von neumann", "moore"):
        born, survive = RULES[nb]
        for B in args.universes:
            words = fills(B)
            ens.configure(B, neighbourhood=nb)
            ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood=nb, born=born, survive=survive)
            recs = (_capi.SummaryStruct * B)()
            view = np.frombuffer(recs, dtype=np.dtype(_capi.SummaryStruct))
            for every in (1, 8):
                K = host.trace_samples(args.steps, every)

                def traced():
                    """(a) -> (event ms, wall ms, samples)"""
                    ens.upload_state(0, words)
                    t0 = time.perf_counter()
                    samples = ens.step_trace(args.steps, check_every=every, stop_mask=0)[0]
                    wall = (time.perf_counter() - t0) * 1e3
                    return ens.stats().gpu_ms, wall, samples

                def looped(events=False):
                    """(b) -> (event ms summed over the launches when asked for — a call per round the host clock should not pay, wall ms, samples)"""
                    ens.upload_state(0, words)
                    t0 = time.perf_counter()
                    samples = np.zeros((B, K, 3), dtype=np.uint32)
                    event = 0.0
                    done = 0
                    for j in range(K):
                        if j:
                            n = min(every, args.steps - done)
                            ens.step(n)
                            done += n
                        _capi.check(lib.ca3d_ensemble_summarize(ens._h, 0, B, recs))  # synchronises the stream
                        samples[:, j, 0], samples[:, j, 1], samples[:, j, 2] = view["population"], view["births"], view["deaths"]
                        if j and events:
                            event += ens.stats().gpu_ms
                    wall = (time.perf_counter() - t0) * 1e3
                    return event, wall, samples

                def plain():
                    """(c) -> (event ms, wall ms, None)"""
                    ens.upload_state(0, words)
                    t0 = time.perf_counter()
                    ens.step(args.steps)
                    ens.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    return ens.stats().gpu_ms, wall, None

                a, b = traced()[2], looped()[2]
                if not np.array_equal(a, b):
                    raise SystemExit(f"{nb} B={B} check_every={every}: step_trace and the step + summaries loop gave different samples")
                plain()
                paths = {"step_trace": traced, "step_summaries_loop": looped, "plain_step": plain}
                times = {name: [] for name in paths}
                for _ in range(args.repeats):
                    for name, fn in paths.items():
                        times[name].append(fn()[:2])
                    # (b) again for its event time alone
                    times["step_summaries_loop"][-1] = (looped(events=True)[0], times["step_summaries_loop"][-1][1])
                row = {"neighbourhood": nb, "universes": B, "steps": args.steps, "check_every": every, "samples_per_universe": K, "samples_verified": int(a.size)}
                for name, t in times.items():
                    row[name] = {"event_us": statistics.median(x[0] for x in t) * 1e3, "event_us_min_max": [min(x[0] for x in t) * 1e3, max(x[0] for x in t) * 1e3],
                                 "wall_us": statistics.median(x[1] for x in t) * 1e3, "wall_us_min_max": [min(x[1] for x in t) * 1e3, max(x[1] for x in t) * 1e3]}
                row["loop_over_trace_wall"] = row["step_summaries_loop"]["wall_us"] / row["step_trace"]["wall_us"]
                row["loop_over_trace_event"] = row["step_summaries_loop"]["event_us"] / row["step_trace"]["event_us"]
                row["trace_over_plain_event"] = row["step_trace"]["event_us"] / row["plain_step"]["event_us"]
                row["trace_over_plain_wall"] = row["step_trace"]["wall_us"] / row["plain_step"]["wall_us"]
                # by more than the spread: the slowest traced call against the fastest loop
                row["trace_beats_loop_beyond_spread"] = row["step_trace"]["wall_us_min_max"][1] < row["step_summaries_loop"]["wall_us_min_max"][0]
                rows.append(row)
                print(json.dumps(row))
    ens.close()
    return rows


def sheet_rows(args):
    """render_sheet against the upload + render loop: one row per (B, tile, spp)."""
    import ctypes as C

    ens, eng = Ensemble(0), Engine(0)
    eng.configure(G)
    fp = C.POINTER(C.c_float)
    rows = []
    for B in args.universes:
        ens.configure(B)
        ens.seed_states(0, np.arange(1, B + 1), 4)
        words = ens.read_state()
        columns = int(np.ceil(np.sqrt(B)))
        for tile in (64, 128):
            u = host.uniform_block(tile, tile, host.orbit_camera())
            frame = np.empty((tile, tile, 4), dtype=np.uint8)

            def loop(universes, spp):
                for k in universes:
                    eng.upload_state(words[k])
                    _capi.check(eng._lib.ca3d_render(eng._h, u.ctypes.data_as(fp), tile, tile, spp, frame.ctypes.data, None, None))

            for spp in (1, 4):
                sheet = ens.render_sheet(u, tile, tile, columns, spp)
                eng.set_option("render_skip", 0)
                for k in sorted({0, 1, columns, B // 2, B - 1}):
                    loop([k], spp)
                    if not np.array_equal(host.sheet_tile(sheet, k, tile, tile, columns), frame):
                        raise SystemExit(f"B {B}, tile {tile}, spp {spp}: tile {k} is not the engine's frame of universe {k}")
                eng.set_option("render_skip", 1)  # the default: the loop as its users run it
                gpu, wall_sheet, wall_loop = [], [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ens.render_sheet(u, tile, tile, columns, spp)
                    wall_sheet.append((time.perf_counter() - t0) * 1e3)
                    gpu.append(ens.sheet_stats().gpu_ms)
                    t0 = time.perf_counter()
                    loop(range(B), spp)
                    wall_loop.append((time.perf_counter() - t0) * 1e3)
                st = ens.sheet_stats()
                row = {"universes": B, "tile": tile, "spp": spp, "columns": columns, "sheet": list(host.sheet_shape(B, tile, tile, columns))[::-1],
                       "sheet_gpu_ms": statistics.median(gpu), "sheet_gpu_ms_all": gpu,
                       "sheet_wall_ms": statistics.median(wall_sheet), "sheet_wall_ms_all": wall_sheet,
                       "loop_wall_ms": statistics.median(wall_loop), "loop_wall_ms_all": wall_loop,
                       "loop_over_sheet_wall": statistics.median(wall_loop) / statistics.median(wall_sheet),
                       "primary_rays": int(st.primary_rays), "shadow_rays": int(st.shadow_rays),
                       "cell_visits": int(st.primary_cell_visits + st.shadow_cell_visits), "tiles_verified": 5}
                rows.append(row)
                print(json.dumps(row))
    ens.close()
    eng.close()
    return rows


CENSUS_ASH = {"ash B5-7/S4-6": ("5-7", "4-6", 2), "ash B6/S5-7": ("6", "5-7", 1)}  # born, survive, and_rounds of the seed
CENSUS_SYNTHETIC = {"sparse (509 objects, 518 cells)": (G, 0xCA3D0009, 8), "giant (190 objects, one of 1306 cells)": (G, 77, 2, ((20, 20, 20), (43, 43, 43)))}


def census_rows(args):
    """census against read_state + labelling on the CPU: one row per (workload, B). -> (rows, the labeller's name)"""
    try:
        from scipy import ndimage
        labeller = "scipy.ndimage.label, full 3 x 3 x 3 structure"
    except ImportError:
        ndimage, labeller = None, "host.census"
    full = np.ones((3, 3, 3), dtype=int)
    M = 1024

    def cells_of(words):
        return np.unpackbits(words.view(np.uint8), bitorder="little").reshape(G, G, G)

    def label_only(states):
        for w in states:
            if ndimage is not None:
                ndimage.label(cells_of(w), structure=full)
            else:
                host.census(w, M)

    def by_label(w):
        """(first_cell, population, box_min, box_max) of every component, in the census' order."""
        if ndimage is None:
            c, n, _ = host.census(w, M)
            return [(int(r["first_cell"]), int(r["population"]), int(r["box_min"]), int(r["box_max"])) for r in c[:n]]
        lab, n = ndimage.label(cells_of(w), structure=full)
        flat = lab.ravel()
        live = np.flatnonzero(flat)
        firsts = np.full(n + 1, 1 << 30, dtype=np.int64)
        np.minimum.at(firsts, flat[live], live)
        pops = np.bincount(flat, minlength=n + 1)
        out = []
        for k, sl in enumerate(ndimage.find_objects(lab), start=1):
            out.append((int(firsts[k]), int(pops[k]), sl[2].start | sl[1].start << 8 | sl[0].start << 16,
                        (sl[2].stop - 1) | (sl[1].stop - 1) << 8 | (sl[0].stop - 1) << 16))
        return sorted(out)

    ens = Ensemble(0)
    rows = []
    for B in args.universes:
        for name in list(CENSUS_ASH) + list(CENSUS_SYNTHETIC):
            ens.configure(B, neighbourhood="moore")
            steps = None
            if name in CENSUS_ASH:
                born, survive, rounds = CENSUS_ASH[name]
                ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
                ens.seed_states(0, np.arange(1, B + 1), rounds)
                done, reason, _ = ens.step_until_cycle(512)
                steps = {"max_steps": 512, "stopped": int(np.count_nonzero(reason)), "median_steps_done": float(np.median(done))}
            else:
                ens.upload_state(0, np.broadcast_to(host.seeded_state(*CENSUS_SYNTHETIC[name]), (B, W)))
            states = ens.read_state()
            comps, n, rest = ens.census(max_components=M)
            for u in range(B):
                want = by_label(states[u])
                got = [(int(r["first_cell"]), int(r["population"]), int(r["box_min"]), int(r["box_max"])) for r in comps[u, :n[u]]]
                if got != want[:M] or int(rest[u]) != sum(w[1] for w in want[M:]):
                    raise SystemExit(f"{name}, B {B}: the census of universe {u} is not the CPU labelling's")
            sample = sorted({0, B // 2, B - 1})
            for u in sample:
                c, k, r = host.census(states[u], M)
                if c.tobytes() != comps[u].tobytes() or (k, r) != (int(n[u]), int(rest[u])):
                    raise SystemExit(f"{name}, B {B}: the census of universe {u} is not host.census'")
            gpu, wall, read, cpu = [], [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                ens.census(max_components=M)
                wall.append((time.perf_counter() - t0) * 1e3)
                gpu.append(ens.census_gpu_ms())
                t0 = time.perf_counter()
                got = ens.read_state()
                read.append((time.perf_counter() - t0) * 1e3)
                label_only(got)
                cpu.append((time.perf_counter() - t0) * 1e3)
            row = {"workload": name, "universes": B, "max_components": M, "stepping": steps,
                   "components_per_universe": {"min": int(n.min()), "median": float(np.median(n)), "max": int(n.max())},
                   "live_cells_per_universe_median": float(np.median(comps["population"].sum(axis=1) + rest)),
                   "complete_universes": int(np.count_nonzero(rest == 0)), "universes_verified": B, "digests_verified_in": sample,
                   "census_gpu_ms": statistics.median(gpu), "census_gpu_ms_all": gpu,
                   "census_wall_ms": statistics.median(wall), "census_wall_ms_all": wall,
                   "read_state_wall_ms": statistics.median(read), "read_state_wall_ms_all": read,
                   "read_state_and_label_wall_ms": statistics.median(cpu), "read_state_and_label_wall_ms_all": cpu,
                   "cpu_path_over_census_wall": statistics.median(cpu) / statistics.median(wall)}
            rows.append(row)
            print(json.dumps(row))
    ens.close()
    return rows, labeller


def isolate_rows(args):
    """isolate against the read_state + cut + upload_state loop: one row per B. -> (rows, the cutter's name)"""
    try:
        from scipy import ndimage
        cutter = "scipy.ndimage.label, full 3 x 3 x 3 structure, one labelling a universe"
    except ImportError:
        ndimage, cutter = None, "host.isolate per object"
    full = np.ones((3, 3, 3), dtype=int)
    M = 1024
    born, survive, rounds = CENSUS_ASH["ash B6/S5-7"]

    def centred_by_label(words, cells):
        """The centred states of the objects that hold `cells`, from one labelling of the universe."""
        lab, _ = ndimage.label(np.unpackbits(words.view(np.uint8), bitorder="little").reshape(G, G, G), structure=full)
        boxes = ndimage.find_objects(lab)
        out = []
        for cell in cells:
            k = int(lab[cell >> 12, (cell >> 6) & 63, cell & 63])
            sl = boxes[k - 1]
            part = lab[sl] == k
            moved = np.zeros((G, G, G), dtype=np.uint8)
            lo = [(G - n) // 2 for n in part.shape]
            moved[lo[0]:lo[0] + part.shape[0], lo[1]:lo[1] + part.shape[1], lo[2]:lo[2] + part.shape[2]] = part
            out.append(np.packbits(moved.ravel(), bitorder="little").view("<u4"))
        return out

    ens, nursery = Ensemble(0), Ensemble(0)
    rows = []
    for B in args.universes:
        ens.configure(B, neighbourhood="moore")
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        ens.seed_states(0, np.arange(1, B + 1), rounds)
        done, reason, _ = ens.step_until_cycle(512)
        comps, n, rest = ens.census(max_components=M)
        if rest.any():
            raise SystemExit(f"B {B}: a census of {M} objects a universe is not complete")
        jobs = np.array([(u, int(c["first_cell"])) for u in range(B) for c in comps[u, :n[u]]], dtype=np.uint32).reshape(-1, 2)
        starts = np.concatenate([[0], np.cumsum(n)])
        J = len(jobs)
        nursery.configure(J, neighbourhood="moore")
        pop, shift = nursery.isolate(jobs, 0, ens, "centre", True)
        sample = sorted({0, B // 2, B - 1})
        for u in sample:
            words = ens.read_state(u, 1)[0]
            got = nursery.read_state(int(starts[u]), int(n[u]))
            for k in range(int(n[u])):
                j = int(starts[u]) + k
                w, p, d = host.isolate(words, int(jobs[j, 1]), "centre")
                if not np.array_equal(got[k], w) or (int(pop[j]), tuple(int(v) for v in shift[j])) != (p, d):
                    raise SystemExit(f"B {B}: object {k} of universe {u} is not host.isolate's")
        if not np.array_equal(pop, np.concatenate([comps["population"][u, :n[u]] for u in range(B)])):
            raise SystemExit(f"B {B}: the isolated populations are not the census'")
        left = nursery.read_state()
        gpu, wall, loop = [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            nursery.isolate(jobs, 0, ens, "centre", True)
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(nursery.isolate_gpu_ms())
            t0 = time.perf_counter()
            for u in range(B):
                words = ens.read_state(u, 1)[0]
                a, b = int(starts[u]), int(starts[u + 1])
                cells = [int(c) for c in jobs[a:b, 1]]
                cut = centred_by_label(words, cells) if ndimage is not None else [host.isolate(words, c, "centre")[0] for c in cells]
                for k, w in enumerate(cut):
                    nursery.upload_state(a + k, w)
            loop.append((time.perf_counter() - t0) * 1e3)
            if not np.array_equal(nursery.read_state(), left):
                raise SystemExit(f"B {B}: the loop left other states than the call")
        row = {"workload": "ash B6/S5-7", "universes": B, "max_components": M, "placement": "centre", "copy_rules": True,
               "stepping": {"max_steps": 512, "stopped": int(np.count_nonzero(reason)), "median_steps_done": float(np.median(done))},
               "objects": J, "objects_per_universe": {"min": int(n.min()), "median": float(np.median(n)), "max": int(n.max())},
               "cells_per_object_median": float(np.median(pop)), "verified_against_host_isolate_in": sample,
               "isolate_gpu_ms": statistics.median(gpu), "isolate_gpu_ms_all": gpu,
               "isolate_wall_ms": statistics.median(wall), "isolate_wall_ms_all": wall,
               "loop_wall_ms": statistics.median(loop), "loop_wall_ms_all": loop,
               "loop_over_isolate_wall": statistics.median(loop) / statistics.median(wall)}
        rows.append(row)
        print(json.dumps(row))
    ens.close()
    nursery.close()
    return rows, cutter


def census_torus_rows(args):
    """census and isolate under CA3D_CONNECT_TORUS against the same launches under CA3D_CONNECT_CLOSED on the same universes: one row
    per B."""
    M = 1024
    born, survive, rounds = CENSUS_ASH["ash B6/S5-7"]
    ens, nursery = Ensemble(0), Ensemble(0)
    rows = []
    for B in args.universes:
        ens.configure(B, neighbourhood="moore")
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        ens.seed_states(0, np.arange(1, B + 1), rounds)
        ens.set_boundary("torus")
        done, reason, _ = ens.step_until_cycle(512)
        sample = sorted({0, B // 2, B - 1})
        found, jobs = {}, {}
        for how in host.CONNECTIVITIES:
            comps, n, rest = ens.census(max_components=M, connectivity=how)
            if rest.any():
                raise SystemExit(f"B {B}, {how}: a census of {M} objects a universe is not complete")
            for u in sample:
                c, k, r = host.census(ens.read_state(u, 1)[0], M, how)
                if (int(n[u]), int(rest[u])) != (k, r) or comps[u].tobytes() != c.tobytes():
                    raise SystemExit(f"B {B}, {how}: the census of universe {u} is not host.census'")
            found[how] = (comps, n)
            jobs[how] = np.array([(u, int(c["first_cell"])) for u in range(B) for c in comps[u, :n[u]]], dtype=np.uint32).reshape(-1, 2)
        nursery.configure(max(len(j) for j in jobs.values()), neighbourhood="moore")
        for how in host.CONNECTIVITIES:
            comps, n = found[how]
            starts = np.concatenate([[0], np.cumsum(n)])
            pop, shift = nursery.isolate(jobs[how], 0, ens, "centre", True, connectivity=how)
            for u in sample:
                words = ens.read_state(u, 1)[0]
                got = nursery.read_state(int(starts[u]), int(n[u]))
                for k in range(int(n[u])):
                    j = int(starts[u]) + k
                    w, p, d = host.isolate(words, int(jobs[how][j, 1]), "centre", how)
                    if not np.array_equal(got[k], w) or (int(pop[j]), tuple(int(v) for v in shift[j])) != (p, d):
                        raise SystemExit(f"B {B}, {how}: object {k} of universe {u} is not host.isolate's")
        census_ms, isolate_ms = {h: [] for h in host.CONNECTIVITIES}, {h: [] for h in host.CONNECTIVITIES}
        for _ in range(args.repeats):  # the two alternate
            for how in host.CONNECTIVITIES:
                ens.census(max_components=M, connectivity=how)
                census_ms[how].append(ens.census_gpu_ms())
                nursery.isolate(jobs[how], 0, ens, "centre", True, connectivity=how)
                isolate_ms[how].append(nursery.isolate_gpu_ms())
        med = statistics.median
        row = {"workload": "ash B6/S5-7 under the torus boundary", "universes": B, "max_components": M, "placement": "centre", "copy_rules": True,
               "stepping": {"max_steps": 512, "stopped": int(np.count_nonzero(reason)), "median_steps_done": float(np.median(done))},
               "objects": {h: int(len(jobs[h])) for h in host.CONNECTIVITIES},
               "objects_the_closed_census_splits": int(len(jobs["closed"]) - len(jobs["torus"])),
               "universes_where_the_counts_differ": int(np.count_nonzero(found["closed"][1] != found["torus"][1])),
               "verified_against_host_in": sample,
               "census_gpu_ms": {h: med(census_ms[h]) for h in host.CONNECTIVITIES}, "census_gpu_ms_all": census_ms,
               "isolate_gpu_ms": {h: med(isolate_ms[h]) for h in host.CONNECTIVITIES}, "isolate_gpu_ms_all": isolate_ms,
               "census_torus_over_closed": med(census_ms["torus"]) / med(census_ms["closed"]),
               "isolate_torus_over_closed": med(isolate_ms["torus"]) / med(isolate_ms["closed"])}
        rows.append(row)
        print(json.dumps(row))
    ens.close()
    nursery.close()
    return rows


def compose_rows(args):
    """compose against the read_state + host.compose + upload_state loop: one row per B and mix of orientations. -> rows"""
    M = 1024
    born, survive, rounds = CENSUS_ASH["ash B6/S5-7"]
    x_keeping = [o for o in range(48) if host.ORIENTATION_PERMS[o % 6][0] == 0]
    mixes = {"all 48": list(range(48)), "the 8 that leave x on x": x_keeping, "the other 40": [o for o in range(48) if o not in x_keeping],
             "one part, orientation 0": None}
    block = host.cells_to_words(G, [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    ens, nursery, stage = Ensemble(0), Ensemble(0), Ensemble(0)
    rows = []
    for B in args.universes:
        ens.configure(B, neighbourhood="moore")
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        ens.seed_states(0, np.arange(1, B + 1), rounds)
        done, reason, _ = ens.step_until_cycle(512)
        comps, n, rest = ens.census(max_components=M)
        if rest.any():
            raise SystemExit(f"B {B}: a census of {M} objects a universe is not complete")
        jobs = np.array([(u, int(c["first_cell"])) for u in range(B) for c in comps[u, :n[u]]], dtype=np.uint32).reshape(-1, 2)
        J = len(jobs)
        nursery.configure(J + 1, neighbourhood="moore")
        nursery.upload_state(J, block)
        nursery.set_rule_strings(J, neighbourhood="moore", born=born, survive=survive)
        pop, _ = nursery.isolate(jobs, 0, ens, "centre", True)
        iso = []
        for _ in range(args.repeats):
            nursery.isolate(jobs, 0, ens, "centre", True)
            iso.append(nursery.isolate_gpu_ms())
        stage.configure(J, neighbourhood="moore")
        L = min(args.loop_destinations, J)
        for name, mix in mixes.items():
            if mix is None:
                layouts = [[(k, 0, (8, 8, 8))] for k in range(J)]
            else:
                layouts = [[(k, mix[k % len(mix)], (8 + k % 24, 8, 8)), (J, 0, (48, 48, 48))] for k in range(J)]
            recs = stage.compose(layouts, 0, nursery, False, True)
            sample = sorted({0, 1, J // 3, J // 2, J - 2, J - 1} | set(range(100, 148)))
            for k in sample:
                pieces = {u: nursery.read_state(u, 1)[0] for u, _, _ in layouts[k]}
                w, r = host.compose(pieces, layouts[k])
                if not np.array_equal(stage.read_state(k, 1)[0], w) or recs[k].tolist() != r.tolist():
                    raise SystemExit(f"B {B}, {name}: destination {k} is not host.compose's")
            left = stage.read_state(0, L)
            gpu, wall, loop = [], [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                stage.compose(layouts, 0, nursery, False, True)
                wall.append((time.perf_counter() - t0) * 1e3)
                gpu.append(stage.compose_gpu_ms())
                t0 = time.perf_counter()
                for k in range(L):
                    pieces = {u: nursery.read_state(u, 1)[0] for u, _, _ in layouts[k]}
                    stage.upload_state(k, host.compose(pieces, layouts[k])[0])
                loop.append((time.perf_counter() - t0) * 1e3)
                if not np.array_equal(stage.read_state(0, L), left):
                    raise SystemExit(f"B {B}, {name}: the loop left other states than the call")
            row = {"workload": "ash B6/S5-7", "universes": B, "mix": name, "destinations": J, "parts_per_destination": len(layouts[0]),
                   "cells_per_object_median": float(np.median(pop)), "clipped_cells": int(recs["clipped"].sum()),
                   "verified_against_host_compose_in": len(sample),
                   "compose_gpu_ms": statistics.median(gpu), "compose_gpu_ms_all": gpu,
                   "compose_wall_ms": statistics.median(wall), "compose_wall_ms_all": wall,
                   "isolate_gpu_ms_same_objects": statistics.median(iso), "isolate_gpu_ms_same_objects_all": iso,
                   "loop_destinations": L, "loop_wall_ms": statistics.median(loop), "loop_wall_ms_all": loop,
                   "loop_wall_ms_per_destination": statistics.median(loop) / L,
                   "compose_wall_ms_per_destination": statistics.median(wall) / J}
            rows.append(row)
            print(json.dumps(row))
        # the dense case: whole soups, one part a destination, where every bit of the gather is a cell
        D = 4096
        ens.seed_states(0, np.arange(1, B + 1), 1)
        stage.configure(D, neighbourhood="moore")
        for name in ("the 8 that leave x on x", "the other 40"):
            mix = mixes[name]
            layouts = [[(k % B, mix[k % len(mix)], (k % 5 - 2, 0, 0))] for k in range(D)]
            recs = stage.compose(layouts, 0, ens, False, True)
            sample = list(range(0, D, D // 48))
            for k in sample:
                w, r = host.compose({layouts[k][0][0]: ens.read_state(layouts[k][0][0], 1)[0]}, layouts[k])
                if not np.array_equal(stage.read_state(k, 1)[0], w) or recs[k].tolist() != r.tolist():
                    raise SystemExit(f"B {B}, soups, {name}: destination {k} is not host.compose's")
            gpu, wall = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                stage.compose(layouts, 0, ens, False, True)
                wall.append((time.perf_counter() - t0) * 1e3)
                gpu.append(stage.compose_gpu_ms())
            row = {"workload": "soups, and_rounds 1 (65 536 cells, box 64^3)", "universes": B, "mix": name, "destinations": D, "parts_per_destination": 1,
                   "clipped_cells": int(recs["clipped"].sum()), "verified_against_host_compose_in": len(sample),
                   "compose_gpu_ms": statistics.median(gpu), "compose_gpu_ms_all": gpu,
                   "compose_wall_ms": statistics.median(wall), "compose_wall_ms_all": wall, "loop_wall_ms": None}
            rows.append(row)
            print(json.dumps(row))
    for e in (ens, nursery, stage):
        e.close()
    return rows


def canon_rows(args):
    """canon against the read_state + host.canon loop, with the census launch on the same universes for scale: per B one row for the
    ash's objects in a nursery and one for B dense soups. -> rows"""
    M = 1024
    born, survive, rounds = CENSUS_ASH["ash B6/S5-7"]
    ens, nursery = Ensemble(0), Ensemble(0)
    rows = []

    def measure(e, n, label, B, extra):
        """One row: canon over universes 0 .. n - 1 of `e`, verified against host.canon in a sample, then timed."""
        L = min(args.loop_destinations, n)
        rec, dig = e.canon(0, n, digests=True)
        sample = sorted({0, 1, n // 3, n // 2, n - 1} | set(range(min(100, n - 1), min(124, n))))
        for k in sample:
            r, d = host.canon(e.read_state(k, 1)[0])
            if rec[k].tobytes() != r.tobytes() or not np.array_equal(dig[k], d):
                raise SystemExit(f"B {B}, {label}: universe {k} is not host.canon's")
        gpu, gpu_dig, wall, cen, loop = [], [], [], [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            plain = e.canon(0, n)
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(e.canon_gpu_ms())
            e.canon(0, n, digests=True)
            gpu_dig.append(e.canon_gpu_ms())
            e.census(0, n, max_components=M)
            cen.append(e.census_gpu_ms())
            t0 = time.perf_counter()
            keys = [host.canon(e.read_state(k, 1)[0])[0]["key"] for k in range(L)]
            loop.append((time.perf_counter() - t0) * 1e3)
            if plain["key"][:L].tolist() != [int(k) for k in keys] or plain.tobytes() != rec.tobytes():
                raise SystemExit(f"B {B}, {label}: the loop found other keys than the call")
        row = {"workload": label, "universes": B, "canon_universes": n, "verified_against_host_canon_in": len(sample),
               "canon_gpu_ms": statistics.median(gpu), "canon_gpu_ms_all": gpu,
               "canon_gpu_ms_with_digests": statistics.median(gpu_dig), "canon_gpu_ms_with_digests_all": gpu_dig,
               "canon_gpu_us_per_universe": statistics.median(gpu) * 1e3 / n,
               "canon_wall_ms": statistics.median(wall), "canon_wall_ms_all": wall,
               "census_gpu_ms_same_universes": statistics.median(cen), "census_gpu_ms_same_universes_all": cen,
               "loop_universes": L, "loop_wall_ms": statistics.median(loop), "loop_wall_ms_all": loop,
               "loop_wall_ms_per_universe": statistics.median(loop) / L, "canon_wall_ms_per_universe": statistics.median(wall) / n}
        row.update(extra(rec, dig))
        rows.append(row)
        print(json.dumps(row))

    for B in args.universes:
        ens.configure(B, neighbourhood="moore")
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        ens.seed_states(0, np.arange(1, B + 1), rounds)
        done, reason, _ = ens.step_until_cycle(512)
        comps, n, rest = ens.census(max_components=M)
        if rest.any():
            raise SystemExit(f"B {B}: a census of {M} objects a universe is not complete")
        jobs = np.array([(u, int(c["first_cell"])) for u in range(B) for c in comps[u, :n[u]]], dtype=np.uint32).reshape(-1, 2)
        census_digests = np.concatenate([comps["digest"][u, :n[u]] for u in range(B)])
        J = len(jobs)
        nursery.configure(J, neighbourhood="moore")
        pop, _ = nursery.isolate(jobs, 0, ens, "centre", True)

        def catalogue(rec, dig):
            if not np.array_equal(dig[:, 0], census_digests):
                raise SystemExit(f"B {B}: digests[:, 0] are not the census digests")
            keys, counts = np.unique(rec["key"], return_counts=True)
            groups = np.array([bin(int(s)).count("1") for s in rec["symmetry"]])
            return {"objects": J, "cells_per_object_median": float(np.median(pop)),
                    "distinct_census_digests": int(np.unique(census_digests).size), "distinct_keys": int(keys.size),
                    "most_common_key_count": int(counts.max()), "objects_with_a_symmetry_besides_the_identity": int((groups > 1).sum()),
                    "chiral_objects": int(sum(host.is_chiral(s) for s in rec["symmetry"]))}

        measure(nursery, J, "ash B6/S5-7: every object of a census, isolated (centred) into a nursery", B, catalogue)
        # the dense case: whole soups, where every bit of the forty's gather is a cell
        ens.seed_states(0, np.arange(1, B + 1), 1)
        measure(ens, B, "soups, and_rounds 1 (65 536 cells, box 64^3)", B, lambda rec, dig: {"distinct_keys": int(np.unique(rec["key"]).size)})
    ens.close()
    nursery.close()
    return rows


def canon_period_rows(args):
    """canon_period against canon_phases: per B the ash nursery with periods 4 and 1 and B dense soups with period 4. -> rows"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol

    M = 1024
    born, survive, rounds = CENSUS_ASH["ash B6/S5-7"]
    rules = ol.Rules.from_strings(neighbourhood="moore", born=born, survive=survive)
    ens, nursery = Ensemble(0), Ensemble(0)
    rows = []

    def measure(e, n, restore, period, label, B):
        """One row: canon_period over universes 0 .. n - 1 of `e` with one period, verified, then timed beside canon_phases."""
        periods = np.full(n, period, dtype=np.uint32)
        restore()
        rec, keys = e.canon_period(periods, 0, n, keys=True)
        sample = sorted({0, 1, n // 3, n // 2, n - 1} | set(range(min(100, n - 1), min(108, n))))
        for k in sample:
            t = [e.read_state(k, 1)[0]]
            for _ in range(period):
                t.append(ol.packed_step(G, t[-1], rules))
            r, ks = host.canon_period(np.stack(t))
            if rec[k].tobytes() != r.tobytes() or not np.array_equal(keys[k], ks):
                raise SystemExit(f"B {B}, {label}: universe {k} is not host.canon_period's")
        gpu, gpu_keys, wall, old_wall, old_gpu, old_canon, old_step, plain = [], [], [], [], [], [], [], []
        for _ in range(args.repeats):
            restore()
            e.synchronize()
            t0 = time.perf_counter()
            now = e.canon_period(periods, 0, n)
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(e.canon_period_gpu_ms())
            e.canon_period(periods, 0, n, keys=True)
            gpu_keys.append(e.canon_period_gpu_ms())
            if now.tobytes() != rec.tobytes():
                raise SystemExit(f"B {B}, {label}: two calls differ")
            e.canon(0, n)
            plain.append(e.canon_gpu_ms())
            t0 = time.perf_counter()
            key, phase, orientation, symmetry = e.canon_phases(periods, 0, n, max_period=max(64, period))
            e.synchronize()
            old_wall.append((time.perf_counter() - t0) * 1e3)
            if not (np.array_equal(key, rec["key"]) and np.array_equal(phase, rec["phase"]) and np.array_equal(orientation, rec["orientation"])
                    and np.array_equal(symmetry, rec["symmetry"])):
                raise SystemExit(f"B {B}, {label}: canon_phases found something else than the call")
            restore()
            c_ms = s_ms = 0.0
            for _ in range(period):  # canon_phases' launches, timed one by one
                e.canon(0, n)
                c_ms += e.canon_gpu_ms()
                e.step(1)
                e.synchronize()
                s_ms += e.stats().gpu_ms
            old_canon.append(c_ms)
            old_step.append(s_ms)
            old_gpu.append(c_ms + s_ms)
        med = statistics.median
        row = {"workload": label, "universes": B, "canon_universes": n, "period": period, "verified_against_host_canon_period_in": len(sample),
               "closed": int((rec["flags_shift"] & 1).sum()), "ships": int(((rec["flags_shift"] & 1).astype(bool) & ((rec["flags_shift"] >> 8) != 0)).sum()),
               "distinct_keys": int(np.unique(rec["key"]).size),
               "canon_period_gpu_ms": med(gpu), "canon_period_gpu_ms_all": gpu,
               "canon_period_gpu_ms_with_keys": med(gpu_keys), "canon_period_gpu_ms_with_keys_all": gpu_keys,
               "canon_period_wall_ms": med(wall), "canon_period_wall_ms_all": wall,
               "canon_gpu_ms_one_launch": med(plain), "canon_gpu_ms_one_launch_all": plain,
               "canon_phases_wall_ms": med(old_wall), "canon_phases_wall_ms_all": old_wall,
               "canon_phases_gpu_ms_summed": med(old_gpu), "canon_phases_gpu_ms_summed_all": old_gpu,
               "canon_phases_canon_gpu_ms_summed": med(old_canon), "canon_phases_step_gpu_ms_summed": med(old_step),
               "gpu_ratio_phases_over_period": med(old_gpu) / med(gpu), "wall_ratio_phases_over_period": med(old_wall) / med(wall)}
        rows.append(row)
        print(json.dumps(row))

    for B in args.universes:
        ens.configure(B, neighbourhood="moore")
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        ens.seed_states(0, np.arange(1, B + 1), rounds)
        ens.step_until_cycle(512)
        comps, n, rest = ens.census(max_components=M)
        if rest.any():
            raise SystemExit(f"B {B}: a census of {M} objects a universe is not complete")
        jobs = np.array([(u, int(c["first_cell"])) for u in range(B) for c in comps[u, :n[u]]], dtype=np.uint32).reshape(-1, 2)
        J = len(jobs)
        nursery.configure(J, neighbourhood="moore")
        put_back = lambda: nursery.isolate(jobs, 0, ens, "centre", True)  # noqa: E731
        for period in (4, 1):
            measure(nursery, J, put_back, period, "ash B6/S5-7: every object of a census, isolated (centred) into a nursery", B)
        soups = Ensemble(0)
        soups.configure(B, neighbourhood="moore")
        soups.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        measure(soups, B, lambda: soups.seed_states(0, np.arange(1, B + 1), 1), 4, "soups, and_rounds 1 (65 536 cells, box 64^3), B6/S5-7", B)
        soups.close()
    ens.close()
    nursery.close()
    return rows


def envelope_rows(args):
    """envelope against the loop it replaces — read_state + step(1) per phase with numpy OR / AND / popcount on the host, run on a copy of
    the universes in the same process: per B the ash nursery with periods all 4 and B dense soups with period 4. -> rows"""
    M = 1024
    born, survive, rounds = CENSUS_ASH["ash B6/S5-7"]
    tables = tuple(sum(1 << v for v in host.rules_components_to_values(s)) & ((1 << 27) - 1) for s in (born, survive))
    ens, nursery, copy = Ensemble(0), Ensemble(0), Ensemble(0)
    rows = []
    bits = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)

    def popcounts(a):
        """popcount of every row of a [n, words] array, through a table of the 256 bytes"""
        return bits[np.ascontiguousarray(a).view(np.uint8)].sum(axis=1, dtype=np.uint64)

    def measure(e, n, period, label, B):
        """One row: envelope over universes 0 .. n - 1 of `e` with one period, verified against host.envelope in a sample, then timed
        beside the loop on `copy`, which holds the same universes and is uploaded again before every loop."""
        periods = np.full(n, period, dtype=np.uint32)
        rec = e.envelope(periods)
        first = e.read_state()
        sample = sorted({0, 1, n // 3, n // 2, n - 1} | set(range(min(100, n - 1), min(108, n))))
        for k in sample:
            if rec[k].tobytes() != host.envelope(first[k], "moore", tables, period)[0].tobytes():
                raise SystemExit(f"B {B}, {label}: universe {k} is not host.envelope's")
        copy.configure(n, neighbourhood="moore")
        copy.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        gpu, wall, loop_wall, loop_gpu = [], [], [], []
        for _ in range(args.repeats):
            e.synchronize()
            t0 = time.perf_counter()
            now = e.envelope(periods)
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(e.envelope_gpu_ms())
            if now.tobytes() != rec.tobytes():
                raise SystemExit(f"B {B}, {label}: two calls differ")
            copy.upload_state(0, first)
            copy.synchronize()
            t0 = time.perf_counter()
            s_ms = 0.0
            prev = copy.read_state()
            env, sta = prev.copy(), prev.copy()
            heat = np.zeros(n, dtype=np.uint64)
            for t in range(period):
                copy.step(1)
                cur = copy.read_state()
                s_ms += copy.stats().gpu_ms
                heat += popcounts(prev ^ cur)
                if t + 1 < period:
                    env |= cur
                    sta &= cur
                prev = cur
            loop_wall.append((time.perf_counter() - t0) * 1e3)
            loop_gpu.append(s_ms)
            if not (np.array_equal(heat, rec["heat"]) and np.array_equal(popcounts(env), rec["envelope_population"]) and np.array_equal(popcounts(sta), rec["stator_population"])):
                raise SystemExit(f"B {B}, {label}: the loop found something else than the call")
        med = statistics.median
        row = {"workload": label, "universes": B, "envelope_universes": n, "period": period, "verified_against_host_envelope_in": len(sample),
               "returns": int((rec["flags"] & 1).sum()), "with_a_rotor": int((rec["envelope_population"] > rec["stator_population"]).sum()),
               "heat_per_step_median": float(np.median(rec["heat"] / period)),
               "envelope_gpu_ms": med(gpu), "envelope_gpu_ms_all": gpu, "envelope_gpu_us_per_universe": med(gpu) * 1e3 / n,
               "envelope_wall_ms": med(wall), "envelope_wall_ms_all": wall,
               "loop_wall_ms": med(loop_wall), "loop_wall_ms_all": loop_wall, "loop_step_gpu_ms_summed": med(loop_gpu),
               "wall_ratio_loop_over_envelope": med(loop_wall) / med(wall)}
        rows.append(row)
        print(json.dumps(row))

    for B in args.universes:
        ens.configure(B, neighbourhood="moore")
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, neighbourhood="moore", born=born, survive=survive)
        ens.seed_states(0, np.arange(1, B + 1), rounds)
        ens.step_until_cycle(512)
        comps, n, rest = ens.census(max_components=M)
        if rest.any():
            raise SystemExit(f"B {B}: a census of {M} objects a universe is not complete")
        jobs = np.array([(u, int(c["first_cell"])) for u in range(B) for c in comps[u, :n[u]]], dtype=np.uint32).reshape(-1, 2)
        J = len(jobs)
        nursery.configure(J, neighbourhood="moore")
        nursery.isolate(jobs, 0, ens, "centre", True)
        measure(nursery, J, 4, "ash B6/S5-7: every object of a census, isolated (centred) into a nursery", B)
        ens.seed_states(0, np.arange(1, B + 1), 1)
        measure(ens, B, 4, "soups, and_rounds 1 (65 536 cells, box 64^3), B6/S5-7", B)
    for e in (ens, nursery, copy):
        e.close()
    return rows


def damage_rows(args):
    """damage against the two-ensemble step(1) + read_state + numpy loop it replaces and against two plain step launches, the floor:
    one row per (kind, B). -> rows"""
    def masks(s, bits):
        return sum(1 << v for v in host.rules_components_to_values(s)) & ((1 << bits) - 1)

    bits = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)

    def popcounts(a):
        """popcount of every row of a [n, words] array, through a table of the 256 bytes"""
        return bits[np.ascontiguousarray(a).view(np.uint8)].sum(axis=1, dtype=np.uint64)

    a, b = Ensemble(0), Ensemble(0)
    rows = []
    med = statistics.median
    for kind in ("von neumann", "moore", "clustered"):
        clustered = kind == "clustered"
        nb = "moore" if clustered else kind
        if clustered:
            keys = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")
            tables = ([masks(CLUSTERED[keys[2 * i]], n) for i, n in enumerate((27, 13, 9))], [masks(CLUSTERED[keys[2 * i + 1]], n) for i, n in enumerate((27, 13, 9))])
        else:
            tables = (masks(RULES[nb][0], 27 if nb == "moore" else 7), masks(RULES[nb][1], 27 if nb == "moore" else 7))
        for B in args.universes:
            words = fills(B)
            rng = np.random.default_rng(B)
            cells = rng.integers(0, 64, (B, 3))
            flips = [[tuple(int(v) for v in c)] for c in cells]
            twins = words.copy()
            for u, (x, y, z) in enumerate(cells):
                twins[u] ^= host.cells_to_words(G, [(int(x), int(y), int(z))])
            for e in (a, b):
                e.configure(B, neighbourhood=nb, clustered=clustered)
                if clustered:
                    e.set_clustered_tables(0, tables[0], tables[1])
                else:
                    e.set_rule_tables(0, tables[0], tables[1])
            a.upload_state(0, words)
            b.upload_state(0, twins)
            sample = sorted({0, B // 2, B - 1})
            short, short_curve = a.damage(3, flips=flips, curve=True)
            for u in sample:
                curve, rec, _ = host.damage(words[u], kind, tables, 3, flips=flips[u])
                if short[u].tobytes() != rec.tobytes() or short_curve[u].tolist() != curve.tolist():
                    raise SystemExit(f"{kind} B={B}: universe {u} is not host.damage's")
            rec, curve = a.damage(args.steps, flips=flips, curve=True)  # warm-up of the timed shape, and what the loop is held to
            n_loop = min(args.loop_samples, args.steps)
            gpu, wall, loop_wall, loop_gpu, floor = [], [], [], [], []
            for _ in range(args.repeats):
                a.synchronize()
                t0 = time.perf_counter()
                now, now_curve = a.damage(args.steps, flips=flips, curve=True)
                wall.append((time.perf_counter() - t0) * 1e3)
                gpu.append(a.damage_gpu_ms())
                if now.tobytes() != rec.tobytes() or not np.array_equal(now_curve, curve):
                    raise SystemExit(f"{kind} B={B}: two calls differ")
                # the loop: samples 0 .. n_loop of the curve from two ensembles in lock step
                a.synchronize(); b.synchronize()
                t0 = time.perf_counter()
                s_ms = 0.0
                d = [popcounts(a.read_state() ^ b.read_state())]
                for _t in range(n_loop):
                    a.step(1)
                    b.step(1)
                    d.append(popcounts(a.read_state() ^ b.read_state()))
                    s_ms += a.stats().gpu_ms + b.stats().gpu_ms  # (the two launches may overlap: an upper bound of their own time)
                loop_wall.append((time.perf_counter() - t0) * 1e3 * args.steps / n_loop)
                loop_gpu.append(s_ms * args.steps / n_loop)
                if not np.array_equal(np.stack(d, axis=1), curve[:, :n_loop + 1]):
                    raise SystemExit(f"{kind} B={B}: the loop found other distances than the call")
                # the floor: two plain launches of --steps steps
                a.upload_state(0, words)
                b.upload_state(0, twins)
                a.synchronize(); b.synchronize()
                a.step(args.steps)
                a.synchronize()  # one after the other: on two streams at once each launch's events would span the other's work too
                b.step(args.steps)
                b.synchronize()
                floor.append(a.stats().gpu_ms + b.stats().gpu_ms)
                a.upload_state(0, words)
                b.upload_state(0, twins)
            row = {"kernel": kind, "universes": B, "steps": args.steps, "verified_against_host_damage_in": len(sample),
                   "healed": int((rec["flags"] & 1).sum()), "final_distance_median": float(np.median(rec["final_distance"])),
                   "damage_gpu_ms": med(gpu), "damage_gpu_ms_all": gpu, "damage_wall_ms": med(wall), "damage_wall_ms_all": wall,
                   "loop_samples_run": n_loop, "loop_wall_ms_scaled": med(loop_wall), "loop_wall_ms_scaled_all": loop_wall, "loop_step_gpu_ms_scaled": med(loop_gpu),
                   "two_step_launches_gpu_ms": med(floor), "two_step_launches_gpu_ms_all": floor,
                   "wall_ratio_loop_over_damage": med(loop_wall) / med(wall), "gpu_ratio_damage_over_two_step_launches": med(gpu) / med(floor)}
            rows.append(row)
            print(json.dumps(row))
    a.close()
    b.close()
    return rows


def usage_rows(args):
    """usage against the step(1) + read_state + numpy counts + bincount loop it replaces and against one plain step launch, the floor:
    one row per (kind, B). -> rows"""
    def masks(s, bits):
        return sum(1 << v for v in host.rules_components_to_values(s)) & ((1 << bits) - 1)

    a = Ensemble(0)
    rows = []
    med = statistics.median
    for kind in ("von neumann", "moore", "clustered"):
        clustered = kind == "clustered"
        nb = "moore" if clustered else kind
        if clustered:
            keys = ("born", "survive", "born_edges", "survive_edges", "born_corners", "survive_corners")
            tables = ([masks(CLUSTERED[keys[2 * i]], n) for i, n in enumerate((27, 13, 9))], [masks(CLUSTERED[keys[2 * i + 1]], n) for i, n in enumerate((27, 13, 9))])
        else:
            tables = (masks(RULES[nb][0], 27 if nb == "moore" else 7), masks(RULES[nb][1], 27 if nb == "moore" else 7))
        for B in args.universes:
            words = fills(B)
            a.configure(B, neighbourhood=nb, clustered=clustered)
            if clustered:
                a.set_clustered_tables(0, tables[0], tables[1])
            else:
                a.set_rule_tables(0, tables[0], tables[1])
            a.upload_state(0, words)
            sample = sorted({0, B // 2, B - 1})
            short = a.usage(3)
            for u in sample:
                if short[u].tobytes() != host.usage(words[u], kind, tables, 3).tobytes():
                    raise SystemExit(f"{kind} B={B}: universe {u} is not host.usage's")
            rec = a.usage(args.steps)  # warm-up of the timed shape
            n_loop = min(args.loop_samples, args.steps)
            head = a.usage(n_loop)  # what the loop is held to
            gpu, wall, loop_wall, loop_gpu, floor = [], [], [], [], []
            for _ in range(args.repeats):
                a.synchronize()
                t0 = time.perf_counter()
                now = a.usage(args.steps)
                wall.append((time.perf_counter() - t0) * 1e3)
                gpu.append(a.usage_gpu_ms())
                if now.tobytes() != rec.tobytes():
                    raise SystemExit(f"{kind} B={B}: two calls differ")
                # the loop: steps 0 .. n_loop - 1 of every universe, counted on the host
                a.synchronize()
                t0 = time.perf_counter()
                s_ms = 0.0
                seen = [[] for _ in range(B)]
                for _t in range(n_loop):
                    for u, w in enumerate(a.read_state()):
                        seen[u].append(host.usage_of_phases([w], kind))
                    a.step(1)
                    s_ms += a.stats().gpu_ms
                a.synchronize()
                loop_wall.append((time.perf_counter() - t0) * 1e3 * args.steps / n_loop)
                loop_gpu.append(s_ms * args.steps / n_loop)
                for u in range(B):
                    for f in ("dead", "alive"):
                        if not np.array_equal(sum(r[f].astype(np.uint64) for r in seen[u]), head[u][f]):
                            raise SystemExit(f"{kind} B={B}: the loop counted otherwise than the call in universe {u}")
                # the floor: one plain launch of --steps steps
                a.upload_state(0, words)
                a.synchronize()
                a.step(args.steps)
                a.synchronize()
                floor.append(a.stats().gpu_ms)
                a.upload_state(0, words)
            row = {"kernel": kind, "universes": B, "steps": args.steps, "verified_against_host_usage_in": len(sample),
                   "table_bits_read_median": float(np.median([sum(bin(int(v)).count("1") for v in list(r["used_born"]) + list(r["used_survive"])) for r in rec])),
                   "usage_gpu_ms": med(gpu), "usage_gpu_ms_all": gpu, "usage_wall_ms": med(wall), "usage_wall_ms_all": wall,
                   "loop_samples_run": n_loop, "loop_wall_ms_scaled": med(loop_wall), "loop_wall_ms_scaled_all": loop_wall, "loop_step_gpu_ms_scaled": med(loop_gpu),
                   "step_launch_gpu_ms": med(floor), "step_launch_gpu_ms_all": floor,
                   "wall_ratio_loop_over_usage": med(loop_wall) / med(wall), "gpu_ratio_usage_over_step_launch": med(gpu) / med(floor)}
            rows.append(row)
            print(json.dumps(row))
    a.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--universes", type=int, nargs="+", default=None, help="default: 1 256 1024 4096 (--cycle: 256 1024)")
    ap.add_argument("--steps", type=int, default=256, help="steps per launch")
    ap.add_argument("--repeats", type=int, default=5, help="alternating measurements per path; the median is reported")
    ap.add_argument("--min-seconds", type=float, default=0.25, help="work per measurement")
    ap.add_argument("--neighbourhood", choices=sorted(RULES) + ["clustered"], default="von neumann",
                    help="of the ensemble and of the rule both paths run; clustered: a clustered ensemble and bench.py's clustered rule")
    ap.add_argument("--out", default=None, help="JSON file to write (moore: profiles/ensemble_moore_64.json)")
    ap.add_argument("--cycle", action="store_true", help="measure step_until_cycle against step_until instead (both neighbourhoods; default B = 256 1024)")
    ap.add_argument("--moving", action="store_true", help="measure step_until_moving against step_until_cycle instead (von Neumann, Moore, clustered; default B = 256 1024)")
    ap.add_argument("--trace", action="store_true", help="measure step_trace against the step + summaries loop and plain stepping instead (both neighbourhoods; default B = 256 1024)")
    ap.add_argument("--sheet", action="store_true", help="measure render_sheet against the upload + render loop instead (B = 256 1024)")
    ap.add_argument("--census", action="store_true", help="measure census against read_state + labelling on the CPU instead (B = 256 1024)")
    ap.add_argument("--census-torus", action="store_true", help="measure census and isolate under the torus connectivity against the closed one instead (B = 256 1024)")
    ap.add_argument("--isolate", action="store_true", help="measure isolate against the read_state + cut + upload_state loop instead (B = 256)")
    ap.add_argument("--compose", action="store_true", help="measure compose against the read_state + host.compose + upload_state loop instead (B = 256)")
    ap.add_argument("--canon", action="store_true", help="measure canon against the read_state + host.canon loop instead (B = 256)")
    ap.add_argument("--canon-period", action="store_true", help="measure canon_period against canon_phases instead (B = 256)")
    ap.add_argument("--envelope", action="store_true", help="measure envelope against the read_state + step(1) loop with numpy OR / AND / popcount instead (B = 256)")
    ap.add_argument("--damage", action="store_true", help="measure damage against the two-ensemble step(1) + read_state + numpy XOR / popcount loop and against two plain step launches instead (all three kinds; B = 256 1024)")
    ap.add_argument("--usage", action="store_true", help="measure usage against the step(1) + read_state + numpy counts + bincount loop and against one plain step launch instead (all three kinds; B = 256 1024)")
    ap.add_argument("--loop-samples", type=int, default=8, help="--damage, --usage: samples the replaced loop is run on; its time is scaled to --steps")
    ap.add_argument("--boundary", action="store_true", help="measure step under the torus and closed boundaries against the reference boundary instead (all three kinds; B = 256 1024)")
    ap.add_argument("--loop-destinations", type=int, default=1024, help="--compose, --canon: destinations / universes the CPU loop is run on")
    ap.add_argument("--commit", default=None, help="commit the figures belong to (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if args.universes is None:
        args.universes = [256] if args.isolate or args.compose or args.canon or args.canon_period or args.envelope else [256, 1024] if args.cycle or args.trace or args.moving or args.sheet or args.census or args.census_torus or args.boundary or args.damage or args.usage else [1, 256, 1024, 4096]
    nb = args.neighbourhood
    clustered = nb == "clustered"
    if clustered:
        nb, rule = "moore", CLUSTERED
    else:
        rule = dict(neighbourhood=nb, born=RULES[nb][0], survive=RULES[nb][1])
    born, survive = rule["born"], rule["survive"]
    if args.out is None and (clustered or nb == "moore"):
        args.out = os.path.join(ROOT, "profiles", "ensemble_clustered_64.json" if clustered else "ensemble_moore_64.json")
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    if args.usage:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_usage_64.json")
        rows = usage_rows(args)
        result = {
            "what": "B universes of 64^3 (random fills, seeds 1 .. B) followed over --steps steps by ONE Ensemble.usage call — one launch of "
                    "ca_ensemble_usage_<kind>64, records copied to the host — for von Neumann, Moore and clustered ensembles under this tool's rules; vs. the "
                    "loop it replaces (per step read_state, the counts and a bincount per universe in numpy on the host, step(1)) and vs. one plain "
                    "Ensemble.step(--steps) launch of the same ensemble, the floor",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "timing": f"usage_gpu_ms: hipEvent time around the launch; usage_wall_ms: host clock around the call; loop_wall_ms_scaled and "
                      f"loop_step_gpu_ms_scaled: the loop run on loop_samples_run steps, its host clock and the summed hipEvent times of its step launches scaled "
                      f"by steps / loop_samples_run; step_launch_gpu_ms: the hipEvent time of the step launch; medians of {args.repeats} "
                      "alternating measurements, after the records equalled host.usage over 3 steps in the sampled universes; the loop's histograms "
                      "equalled the call's over loop_samples_run steps in every universe",
            "not_measured": "the torus and closed kernels, other step counts, other B, other rules",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.damage:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_damage_64.json")
        rows = damage_rows(args)
        result = {
            "what": "B universes of 64^3 (random fills, seeds 1 .. B) and their twins with one random cell flipped, followed over --steps steps by ONE "
                    "Ensemble.damage call with the curve — one launch of ca_ensemble_damage_<kind>64, records and curve copied to the host — for von Neumann, "
                    "Moore and clustered ensembles under this tool's rules; vs. the loop it replaces (two ensembles in lock step: per sample step(1) on each, "
                    "read_state of both, numpy XOR and byte-table popcounts on the host) and vs. two plain Ensemble.step(--steps) launches, the floor",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "timing": f"damage_gpu_ms: hipEvent time around the launch; damage_wall_ms: host clock around the call; loop_wall_ms_scaled and "
                      f"loop_step_gpu_ms_scaled: the loop run on loop_samples_run samples, its host clock and the summed hipEvent times of its step launches scaled "
                      f"by steps / loop_samples_run; two_step_launches_gpu_ms: the summed hipEvent times of the two step launches, run one after the other; medians of {args.repeats} "
                      "alternating measurements, after records and curves equalled host.damage over 3 steps in the sampled universes; the loop's distances "
                      "equalled the call's curve in every universe",
            "not_measured": "the torus and closed kernels, twins in other universes, the image, other step counts, other B, other rules",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.boundary:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_boundary_64.json")
        rows = boundary_rows(args)
        result = {
            "what": "B universes of 64^3 (random fills, seeds 1 .. B) stepped by ONE Ensemble.step call under each boundary mode (set_boundary): the plain kernels "
                    "ca_ensemble_<kind>64_torus and ca_ensemble_<kind>64_closed against ca_ensemble_<kind>64 on the same universes, for von Neumann, Moore and "
                    "clustered ensembles under this tool's rules",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "timing": f"event_us: hipEvent time around the call's launches (ca3d_ensemble_get_stats); medians of {args.repeats} measurements, the three modes "
                      "alternating in one process, the fills uploaded again before each, after every mode's state equalled host.ensemble_step in the sampled "
                      "universes after 3 steps",
            "not_measured": "the *_cycle, *_trace and *_moving forms, other B, other rules",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.census_torus:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_census_torus_64.json")
        result = {
            "what": "B universes of 64^3 of ash produced under the torus boundary (seed_states, seeds 1 .. B, and_rounds 1, Moore B6/S5-7, set_boundary torus, "
                    "step_until_cycle(512)): Ensemble.census(max_components 1024) and Ensemble.isolate of every census object (centred, with its rule) under "
                    "connectivity torus against the same two launches under connectivity closed on the same universes; each connectivity isolates its own "
                    "census' objects",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"torus": ["ca_ensemble_census64_torus", "ca_ensemble_isolate64_torus"], "closed": ["ca_ensemble_census64", "ca_ensemble_isolate64"]},
            "timing": f"hipEvent time around the launch; medians of {args.repeats} measurements, the two connectivities alternating in one process, after both "
                      "censuses equalled host.census byte for byte and every isolated object host.isolate in the sampled universes",
            "rows": census_torus_rows(args),
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.envelope:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_envelope_64.json")
        rows = envelope_rows(args)
        result = {
            "what": "B universes of 64^3 of ash (seed_states, seeds 1 .. B, and_rounds 1, Moore B6/S5-7, step_until_cycle(512)), a census at max_components 1024, every "
                    "object isolated (centred) into a nursery, then ONE Ensemble.envelope call over the nursery with periods all 4 — one launch of "
                    "ca_ensemble_envelope_moore64, the records copied to the host, no images; and the same call over B dense soups (and_rounds 1) under the same rule "
                    "— vs. the loop it replaces on a copy of the same universes in the same process: per phase read_state + step(1), numpy OR / AND and byte-table "
                    "popcounts on the host",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"envelope": "ca_ensemble_envelope_moore64", "loop_step": "ca_ensemble_moore64"},
            "timing": f"envelope_gpu_ms: hipEvent time around the launch; envelope_wall_ms and loop_wall_ms: host clock around the call and around the loop "
                      f"(the copy uploaded before it, outside the clock); loop_step_gpu_ms_summed: the hipEvent times of the loop's step launches; medians of "
                      f"{args.repeats} alternating measurements, after the records equalled host.envelope in the sampled universes; the loop's heat, envelope and "
                      "stator populations equalled the call's in every universe",
            "not_measured": "von Neumann and clustered ensembles, the torus and closed kernels, images written to a destination, periods other than 4, larger B",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.canon_period:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_canon_period_64.json")
        rows = canon_period_rows(args)
        result = {
            "what": "B universes of 64^3 of ash (seed_states, seeds 1 .. B, and_rounds 1, Moore B6/S5-7, step_until_cycle(512)), a census at max_components 1024, every "
                    "object isolated (centred) into a nursery, then ONE Ensemble.canon_period call over the nursery with periods all 4, and all 1 — one launch of "
                    "ca_ensemble_canon_period_moore64, the records copied to the host; and the same call with periods all 4 over B dense soups (and_rounds 1) under "
                    "the same rule — vs. Ensemble.canon_phases on the same universes, the loop it replaces: per phase one launch of ca_ensemble_canon64 and one "
                    "step launch of ca_ensemble_moore64",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"canon_period": "ca_ensemble_canon_period_moore64", "canon": "ca_ensemble_canon64", "step": "ca_ensemble_moore64"},
            "timing": f"canon_period_gpu_ms: hipEvent time around the launch (without the keys array, and with it); canon_phases_gpu_ms_summed: the hipEvent times of "
                      f"canon_phases' launches, period x (canon + step(1)), from the same loop written out; canon_gpu_ms_one_launch: one plain canon launch on the "
                      f"same universes; *_wall_ms: host clock around the call; medians of {args.repeats} alternating measurements, the universes put back before "
                      "each, after records and keys equalled host.canon_period of the CPU oracle's phases in the sampled universes; canon_phases' results equalled "
                      "the call's everywhere",
            "not_measured": "von Neumann and clustered ensembles, periods above 4, larger B, the kernel's phases one by one (occupancy, leaf reloads, the single "
                            "exchange buffer)",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.canon:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_canon_64.json")
        rows = canon_rows(args)
        result = {
            "what": "B universes of 64^3 of ash (seed_states, seeds 1 .. B, and_rounds 1, Moore B6/S5-7, step_until_cycle(512)), a census at max_components 1024, every "
                    "object isolated (centred) into a nursery, then ONE Ensemble.canon call over the nursery — one launch of ca_ensemble_canon64, the records "
                    "copied to the host; and the same call over B dense soups (and_rounds 1) — vs. the loop it replaces, run on the first loop_universes "
                    "universes only: read_state and host.canon; the census launch on the same universes for scale",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"canon": "ca_ensemble_canon64", "census": "ca_ensemble_census64"},
            "timing": f"canon_gpu_ms / census_gpu_ms_same_universes: hipEvent time around the launch (canon without the digests array, and with it); *_wall_ms: "
                      f"host clock around the call / the loop; medians of {args.repeats} alternating measurements after records and all 48 digests equalled "
                      "host.canon in the sampled universes; every loop's keys equalled the call's",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.compose:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_compose_64.json")
        rows = compose_rows(args)
        result = {
            "what": "B universes of 64^3 of ash (seed_states, seeds 1 .. B, and_rounds 1, Moore B6/S5-7, step_until_cycle(512)), a census at max_components 1024, every "
                    "object isolated (centred) into a nursery, then one destination an object composed of two parts — the object, turned, and a 2 x 2 x 2 block — "
                    "with the object's rule, in ONE Ensemble.compose call — one launch of ca_ensemble_compose64 and the reset launch — vs. the loop it replaces "
                    "on the same layouts, run on the first loop_destinations destinations: read_state of the sources, host.compose, upload_state",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"compose": "ca_ensemble_compose64", "isolate": "ca_ensemble_isolate64"},
            "timing": f"compose_gpu_ms / isolate_gpu_ms_same_objects: hipEvent time around the launch; *_wall_ms: host clock around the call / the loop; medians of "
                      f"{args.repeats} alternating measurements after states and records equalled host.compose in the sampled destinations; after each loop its "
                      "destinations held what the call had left there",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.isolate:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_isolate_64.json")
        rows, cutter = isolate_rows(args)
        result = {
            "what": "B universes of 64^3 of ash (seed_states, seeds 1 .. B, and_rounds 1, Moore B6/S5-7, step_until_cycle(512)), a census at max_components 1024, then "
                    "every object of every universe isolated into a second ensemble, centred, with its source's rule, in ONE Ensemble.isolate call — one launch of "
                    "ca_ensemble_isolate64 and the reset launch — vs. the loop it replaces on the same objects: per universe read_state and a cut on the CPU, per "
                    "object upload_state into the second ensemble",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"isolate": "ca_ensemble_isolate64"}, "cpu_cut": cutter,
            "timing": f"isolate_gpu_ms: hipEvent time around the isolate launch; *_wall_ms: host clock around the call / the loop; medians of {args.repeats} alternating "
                      "measurements after the isolated states, populations and shifts equalled host.isolate for every object of the sampled universes; after "
                      "each loop the second ensemble held what the call had left there",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.census:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_census_64.json")
        rows, labeller = census_rows(args)
        result = {
            "what": "B universes of 64^3: Ensemble.census(max_components 1024) — one launch of ca_ensemble_census64, the records copied to the host — vs. the path "
                    "that exists without it, read_state of the same universes + labelling their connected components on the CPU (the labelling alone: no "
                    "populations, boxes or digests are derived in the timed loop). Ash: seed_states (seeds 1 .. B), then step_until_cycle(512)",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"census": "ca_ensemble_census64"}, "cpu_labelling": labeller,
            "timing": f"census_gpu_ms: hipEvent time around the launch; *_wall_ms: host clock around the call(s); medians of {args.repeats} alternating measurements "
                      "after the census equalled the CPU labelling in every universe (population, first cell, box, order) and host.census byte for byte in sampled ones",
            "rows": rows,
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.sheet:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_sheet_64.json")
        result = {
            "what": "B universes of 64^3 seeded with and_rounds 4 (seeds 1 .. B), camera host.orbit_camera(), square tiles, ceil(sqrt(B)) columns: Ensemble.render_sheet "
                    "(presentation read back) vs. the loop it replaces — one Engine at 64^3, per universe upload_state from a host array + ca3d_render with a host "
                    "presentation pointer, default engine options",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {"render_sheet": "ca_render_sheet64", "loop": "ca3d_render's default launches at 64^3"},
            "timing": f"sheet_gpu_ms: hipEvent time around the sheet's launch; *_wall_ms: host clock around the call(s), presentation on the host; medians of "
                      f"{args.repeats} alternating measurements after sampled tiles equalled the engine's render_skip 0 frames",
            "rows": sheet_rows(args),
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.trace:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_trace_64.json")
        result = {
            "what": "B universes of 64^3, random fills (density 1/2), rules B2,4/S1,3,5 (von Neumann) and B5-7/S4-6 (Moore): (a) Ensemble.step_trace(steps, check_every, "
                    "stop mask 0) vs. (b) K - 1 rounds of ca3d_ensemble_step(check_every) + ca3d_ensemble_summarize collecting the same samples vs. (c) a plain step(steps)",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {nb_: {"step_trace": KERNELS[nb_] + "_trace", "step_summaries_loop": KERNELS[nb_], "plain_step": KERNELS[nb_]} for nb_ in sorted(KERNELS)},
            "timing": f"one call from freshly uploaded states; hipEvent time around the launches ((b): summed over its launches) and host clock around the call; medians of "
                      f"{args.repeats} measurements, the three paths alternating in one process, after (a) and (b) gave identical arrays",
            "rows": trace_rows(args),
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        lost = [(r["neighbourhood"], r["universes"], r["check_every"]) for r in result["rows"] if not r["trace_beats_loop_beyond_spread"]]
        if lost:
            raise SystemExit(f"step_trace does not beat the step + summaries loop by more than the spread at {lost}")
        return
    if args.moving:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_moving_64.json")
        names = {"von neumann": "ca_ensemble_vn64", "moore": "ca_ensemble_moore64", "clustered": "ca_ensemble_clustered64"}
        result = {
            "what": "B universes of 64^3, random fills (density 1/2), rules B2,4/S1,3,5 (von Neumann), B5-7/S4-6 (Moore; the same, side tables silent, in the clustered ensemble): "
                    "Ensemble.step_until_moving(steps, stop mask 15) vs. Ensemble.step_until_cycle(steps, stop mask 7); nothing stops, every check is paid",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {k: [v + "_moving", v + "_cycle"] for k, v in names.items()},
            "timing": f"one call from freshly uploaded states; hipEvent time around the launch and host clock around the call; medians of {args.repeats} alternating measurements",
            "rows": moving_rows(args),
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return
    if args.cycle:
        out = args.out or os.path.join(ROOT, "profiles", "ensemble_cycle_64.json")
        result = {
            "what": "B universes of 64^3, random fills (density 1/2), rules B2,4/S1,3,5 (von Neumann) and B5-7/S4-6 (Moore): Ensemble.step_until_cycle(steps, stop mask 7) "
                    "vs. Ensemble.step_until(steps, stop mask 3); nothing stops, every check is paid",
            "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
            "kernels": {nb_: [KERNELS[nb_] + "_cycle", KERNELS[nb_]] for nb_ in sorted(KERNELS)},
            "timing": f"one call from freshly uploaded states; hipEvent time around the launch and host clock around the call; medians of {args.repeats} alternating measurements",
            "rows": cycle_rows(args),
        }
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
        return

    eng, ens = Engine(0), Ensemble(0)
    eng.configure(G)
    eng.set_rule_strings(**rule)
    eng.set_option("stats", 0)  # no event pair per call: the baseline at its best
    rows = []
    for B in args.universes:
        words = fills(B)
        ens.configure(B, neighbourhood=nb, clustered=clustered)
        ens.set_rule_strings(_capi.ENSEMBLE_ALL, **rule)
        sample = range(B) if B <= 256 else sorted(set(range(0, B, max(1, B // 64))) | {255, 256, B - 1})
        verify(ens, eng, words, args.steps, sample)
        eng.upload_state(words[0])

        def ensemble_launch():
            ens.step(args.steps)

        def engine_sweep():
            for _ in range(B):
                eng.step(args.steps)

        te, tb = [], []
        for _ in range(args.repeats):
            te.append(timed(ensemble_launch, ens.synchronize, args.min_seconds))
            tb.append(timed(engine_sweep, eng.synchronize, args.min_seconds))
        ens.step(args.steps)
        event_ms = ens.stats().gpu_ms
        e, b = statistics.median(te), statistics.median(tb)
        row = {
            "universes": B, "steps_per_launch": args.steps,
            "ensemble": {"us_per_launch": e * 1e6, "us_per_launch_min_max": [min(te) * 1e6, max(te) * 1e6], "event_us_last_launch": event_ms * 1e3,
                         "us_per_step": e * 1e6 / args.steps,
                         "universe_steps_per_s": B * args.steps / e, "tcells_per_s": B * args.steps * CELLS / e / 1e12},
            "baseline_engine_sweep": {"us_per_sweep": b * 1e6, "us_per_sweep_min_max": [min(tb) * 1e6, max(tb) * 1e6],
                                      "us_per_step_per_universe": b * 1e6 / (B * args.steps),
                                      "universe_steps_per_s": B * args.steps / b, "tcells_per_s": B * args.steps * CELLS / b / 1e12},
            "baseline_over_ensemble": b / e,
            "states_verified": len(list(sample)),
        }
        rows.append(row)
        print(json.dumps(row))
    kernel = eng.info().kernel_name.decode()
    eng.close(); ens.close()
    result = {
        "what": f"B universes of 64^3, {'clustered rule Moore ' if clustered else 'Moore ' if nb == 'moore' else ''}rule B{born}/S{survive}"
                f"{', edges B%s/S%s, corners B%s/S%s' % tuple(rule[k] for k in ('born_edges', 'survive_edges', 'born_corners', 'survive_corners')) if clustered else ''}, random fills (density 1/2): one Ensemble.step(steps) launch vs. B Engine.step(steps) calls",
        "date": datetime.date.today().isoformat(), "commit": commit, "device": "MI355X (gfx950)",
        "ensemble_kernel": f"{'ca_ensemble_clustered64' if clustered else KERNELS[nb]} (rule as data)", "baseline_kernel": kernel,
        "timing": f"host clock around >= {args.min_seconds} s of calls ending in a synchronise; median of {args.repeats} alternating measurements",
        "rows": rows,
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))
    slower = [r["universes"] for r in rows if r["universes"] >= 256 and r["baseline_over_ensemble"] <= 1.0]
    if slower:
        raise SystemExit(f"the ensemble is no faster than the engine sweep at B = {slower}: it has no reason to exist")


if __name__ == "__main__":
    main()
