#!/usr/bin/env python3
"""Times ca3d_summarize (csrc/ca_summary.hip) against a device copy of the same bytes, and prices the alternatives.

Per grid (packed, density 1/2, one step taken so that both ping-pong buffers are read):
  * hipEvent time of the summary's clear + kernel (Engine.summary_gpu_ms: without the copy back and the host's wait), summed over
    enough calls for a window of a few tenths of a second, in rounds ALTERNATING with ca3d_measure_copy of n_bytes = the bytes the
    summary reads (the copy figure counts read + written bytes, so a read-only stream is compared at equal total bytes);
  * the wall clock of summary() as a host sees it next to read_state() + a host popcount — what there was before;
and at 512^3 the wall clock of step_until(1024, check_every = 8 | 32 | 128) on a rule that never settles next to step(1024).
One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellularautomatons3d_amd import Engine, host  # noqa: E402

NEVER_SETTLES = dict(neighbourhood="von neumann", born="2,4", survive="1,3,5")


def time_grid(e, G, window_s, rounds):
    e.configure(G)
    e.set_rule_strings()
    st = host.random_fill(host.words_per_buffer(G), seed=21)
    e.upload_state(st)
    e.step(1)
    n_bytes = 2 * st.nbytes  # current + previous buffer
    for _ in range(3):
        s = e.summary()
    per_call = max(e.summary_gpu_ms() * 1e-3, 2e-6)
    calls = max(50 if G >= 2048 else 200, int(window_s / rounds / per_call))
    copy_bytes = max(n_bytes, 1 << 20)
    copy_reps = max(4, min(4096, int(window_s / rounds / (2 * per_call))))  # a copy of n_bytes moves twice the bytes
    e.measure_copy(copy_bytes, 4)
    gpu_ms, copy_gbs, wall = [], [], []
    for _ in range(rounds):
        ms = 0.0
        t0 = time.perf_counter()
        for _ in range(calls):
            e.summary()
            ms += e.summary_gpu_ms()
        wall.append((time.perf_counter() - t0) / calls)
        gpu_ms.append(ms / calls)
        copy_gbs.append(e.measure_copy(copy_bytes, copy_reps))
    t0 = time.perf_counter()
    reps_rb = 3
    for _ in range(reps_rb):
        back = e.read_state()
        pop = int(np.bitwise_count(back).sum(dtype=np.uint64)) if hasattr(np, "bitwise_count") else int(np.unpackbits(back.view(np.uint8)).sum(dtype=np.uint64))
    readback_s = (time.perf_counter() - t0) / reps_rb
    assert pop == s.population, (pop, s.population)
    us = float(np.median(gpu_ms)) * 1e3
    rate = n_bytes / (us * 1e-6) / 1e9
    copy = float(np.median(copy_gbs))
    return {"grid": G, "bytes_read": n_bytes, "calls_per_round": calls, "rounds": rounds,
            "summary_gpu_us": round(us, 3), "summary_gpu_us_rounds": [round(x * 1e3, 3) for x in gpu_ms],
            "summary_gb_per_s": round(rate, 1), "copy_gb_per_s": round(copy, 1), "copy_gb_per_s_rounds": [round(x, 1) for x in copy_gbs],
            "fraction_of_copy": round(rate / copy, 3) if copy > 0 else None,
            "summary_wall_us": round(float(np.median(wall)) * 1e6, 2), "read_state_plus_popcount_wall_us": round(readback_s * 1e6, 1),
            "population": s.population, "births": s.births, "deaths": s.deaths}


def time_step_until(e, G=512, steps=1024, reps=5):
    e.configure(G)
    e.set_rule_strings(**NEVER_SETTLES)
    st = host.random_fill(host.words_per_buffer(G), seed=21)
    out = {"grid": G, "steps": steps, "kernel": None}
    rows = {}
    for every in (0, 8, 32, 128):  # 0: plain step(steps)
        walls = []
        for rep in range(reps + 1):  # the first one warms up
            e.upload_state(st)
            e.synchronize()
            t0 = time.perf_counter()
            if every:
                done, reason, _ = e.step_until(steps, check_every=every)
                assert (done, reason) == (steps, 0), (done, reason)
            else:
                e.step(steps)
                e.synchronize()
            if rep:
                walls.append(time.perf_counter() - t0)
        rows["step" if not every else f"check_every_{every}"] = round(float(np.median(walls)) * 1e3, 3)
    out["kernel"] = e.info().kernel_name.decode()
    out["wall_ms"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="256,512,1024,2048")
    ap.add_argument("--window", type=float, default=0.6, help="seconds of summary kernel time per grid, over all rounds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step-until", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = Engine(0)
    doc = {"tool": "tools/run_summary.py", "device": "MI355X (gfx950)", "grids": []}
    for G in [int(x) for x in a.grids.split(",")]:
        row = time_grid(e, G, a.window, a.rounds)
        doc["grids"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if not a.no_step_until:
        doc["step_until"] = time_step_until(e)
    e.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
