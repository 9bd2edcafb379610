"""Windows on the device against the loops they replace: ca3d_cut_windows / ca3d_stamp_windows (Engine.cut_windows / stamp_windows)
between a packed engine of 512^3 and 1024^3 and an ensemble, against read_state + numpy + upload_state over the bus.

  cut    tiling     every window of host.window_tiling(G) — 512 / 4096 of them — into as many universes
         scattered  256 windows at random origins (they wrap and lie across word seams)
         loop       Engine.read_state, per window numpy slicing (whole words for the tiling, host.cut_window for the scattered ones),
                    one Ensemble.upload_state
  stamp  ash        256 isolated ash objects of Moore B6/S5-7 soups (census + isolate, centred), at random origins, each mode
         soups      256 dense soups at origins drawn from a 192^3 corner, so that they overlap heavily, each mode
         loop       Engine.read_state, host.stamp_windows, Engine.upload_state
Reported per case: the hipEvent time around the launches (median, min, max of --repeats calls after a warm-up call), the host clock around
the call (median), and the loop's host clock (--loop-repeats runs, 1 by default: it takes seconds). At 512^3 every device result is compared
with the loop's before anything is timed. No speed is claimed in advance and nothing is required of the ratios.

    python tools/bench_windows.py --out profiles/windows.json

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

from cellularautomatons3d_amd import Engine, Ensemble, host  # noqa: E402

SHIP = ("6", "5-7")


def med(xs, scale=1.0):
    return {"median_ms": statistics.median(xs) * scale, "min_ms": min(xs) * scale, "max_ms": max(xs) * scale, "repeats": len(xs)}


def measure(call, gpu_ms, repeats):
    call()  # warm: the staging array and the events exist afterwards
    gpu, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
        gpu.append(gpu_ms())
    return {"gpu": med(gpu), "host_clock": med(wall, 1e3)}


def timed_loop(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return med(out, 1e3)


def cut_rows(eng, G, args, rng):
    rows = []
    eng.configure(G)
    eng.seed_state(5, 1)
    tiling = [tuple(int(v) for v in o) for o in host.window_tiling(G)]
    scattered = [tuple(int(v) for v in rng.integers(0, G, 3)) for _ in range(256)]
    for name, origins in (("tiling", tiling), ("scattered", scattered)):
        windows = host.window_records(list(enumerate(origins)))
        with Ensemble(0) as ens:
            ens.configure(len(origins))

            def loop():
                grid = eng.read_state().reshape(G, G, G // 32)
                if name == "tiling":
                    cut = np.stack([grid[z:z + 64, y:y + 64, x // 32:x // 32 + 2].reshape(-1) for x, y, z in origins])
                else:
                    cut = np.stack([host.cut_window(G, grid, o) for o in origins])
                ens.upload_state(0, cut)
                return cut

            if G <= 512:
                eng.cut_windows(ens, windows)
                got = ens.read_state()
                if not np.array_equal(got, loop()):
                    raise SystemExit(f"cut {name} at {G}^3: the device's universes differ from the loop's")
            row = {"case": f"cut {name} {G}^3", "windows": len(origins), "universe_mib": len(origins) * 32768 / 2 ** 20}
            row.update(measure(lambda: eng.cut_windows(ens, windows), eng.windows_gpu_ms, args.repeats))
            row["loop_host_clock"] = timed_loop(loop, args.loop_repeats)
            row["loop_over_call"] = row["loop_host_clock"]["median_ms"] / row["host_clock"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def ash_objects(n):
    """`n` universes holding one centred ash object each (or nothing, where a soup died out): soups, stepped to ash, census, isolate."""
    soups, nursery = Ensemble(0), Ensemble(0)
    soups.configure(n, neighbourhood="moore")
    soups.set_rule_strings(0xFFFFFFFF, born=SHIP[0], survive=SHIP[1], neighbourhood="moore")
    soups.seed_states(0, 1 + np.arange(n), 1)
    soups.step(400)
    comps, counts, _ = soups.census(0, n, 64)
    jobs = [(u, int(comps[u][0]["first_cell"]) if counts[u] else 0) for u in range(n)]
    nursery.configure(n, neighbourhood="moore")
    nursery.isolate(np.array(jobs, dtype=np.uint32), src=soups)
    soups.close()
    return nursery, int((counts > 0).sum())


def stamp_rows(eng, G, args, rng):
    rows = []
    eng.configure(G)
    ash, n_objects = ash_objects(256)
    dense = Ensemble(0)
    dense.configure(256)
    dense.seed_states(0, 100 + np.arange(256), 0)
    cases = (("ash", ash, [tuple(int(v) for v in rng.integers(0, G, 3)) for _ in range(256)]),
             ("soups", dense, [tuple(int(v) for v in rng.integers(0, 192, 3)) for _ in range(256)]))
    for name, ens, origins in cases:
        windows = host.window_records(list(enumerate(origins)))
        universes = ens.read_state()
        for mode in host.STAMP_MODES:
            eng.seed_state(5, 3)

            def loop():
                after = host.stamp_windows(G, eng.read_state(), [(universes[k], o) for k, o in enumerate(origins)], mode)
                eng.upload_state(after)
                return after

            if G <= 512:
                eng.stamp_windows(ens, windows, mode)
                got = eng.read_state()
                eng.seed_state(5, 3)
                if not np.array_equal(got, loop()):
                    raise SystemExit(f"stamp {name} {mode} at {G}^3: the device's state differs from the loop's")
                eng.seed_state(5, 3)
            row = {"case": f"stamp {name} {mode} {G}^3", "windows": 256, "live_cells": int(sum(host.state_summary(64, u)["population"] for u in universes))}
            if name == "ash":
                row["universes_with_an_object"] = n_objects
            row.update(measure(lambda: eng.stamp_windows(ens, windows, mode), eng.windows_gpu_ms, args.repeats))
            row["loop_host_clock"] = timed_loop(loop, args.loop_repeats)
            row["loop_over_call"] = row["loop_host_clock"]["median_ms"] / row["host_clock"]["median_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    ash.close()
    dense.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--repeats", type=int, default=5, help="timed calls per case; the median is reported")
    ap.add_argument("--loop-repeats", type=int, default=1, help="runs of the loop a call replaces")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    rng = np.random.default_rng(64)
    rows = []
    with Engine(0) as eng:
        for G in args.grids:
            rows += cut_rows(eng, G, args, rng)
            rows += stamp_rows(eng, G, args, rng)
    result = {"what": "cut_windows / stamp_windows on the device against read_state + numpy + upload_state", "date": datetime.date.today().isoformat(),
              "commit": commit, "device": "MI355X (gfx950)", "kernels": "ca_window_cut / ca_window_stamp / ca_window_clear (csrc/ca_window.hip)",
              "timing": f"gpu: hipEvent around the launches of one call; host_clock: around the call; medians of {args.repeats} calls after a warm-up, "
                        f"min / max given; loop: host clock, {args.loop_repeats} run(s)", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


if __name__ == "__main__":
    main()
