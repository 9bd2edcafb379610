"""Seeding on the device against the path that existed before it: host.random_fill on the CPU + upload_state over the bus.

Packed 512^3 / 1024^3 / 2048^3 for and_rounds 0 and 5, unpacked 512^3, ensembles of 256 and 4096 universes (seed_states, and
set_rule_tables against B set_rule_strings calls). Per case, in one process, the two paths alternating, medians of `--repeats`
measurements with their spread:
  seed        ms per seed call: host clock around >= 20 calls ending in ONE synchronise, after a warm-up call
  parent      host generation (numpy; a CPU figure), the H2D copy ALONE (a pageable host array into an existing device tensor: the bar a
              seed has to beat), and the whole upload_state call (H2D + the device copy into the second buffer + the wait)
  bound       the seed writes 2 x the state bytes and reads nothing: bytes / time against the engine's own ca3d_measure_copy figure of
              the same run (bytes read + written per second) and against the 8 TB/s HBM peak
The kernels use plain stores; non-temporal stores on grids past the Infinity Cache are not built and not measured here.

    python tools/bench_seed.py --out profiles/seed.json

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

import ctypes as C  # noqa: E402

from cellularautomatons3d_amd import LAYOUT_UNPACKED, Engine, Ensemble, _capi, host  # noqa: E402
from cellularautomatons3d_amd.engine import _seed_spec  # noqa: E402

W = 8192
RULES = [("1,3", "0-6"), ("2,4", "1,3,5"), ("", ""), ("", "0-6"), ("3", "2,3"), ("1", ""), ("4-6", "3-6"), ("5,6", "4-6"), ("0", "0-6"), ("2", "1-3")]


def med(xs):
    return {"median_ms": statistics.median(xs) * 1e3, "min_ms": min(xs) * 1e3, "max_ms": max(xs) * 1e3, "repeats": len(xs)}


def per_call(fn, sync, calls):
    fn(); sync()  # warm
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls


def h2d_alone(words):
    """Seconds of one copy of the pageable host array into an existing device tensor, waited for."""
    import torch

    src = torch.from_numpy(words.view(np.int32))
    dst = torch.empty(src.numel(), dtype=torch.int32, device="cuda:0")
    dst.copy_(src); torch.cuda.synchronize()  # warm

    def once():
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    return once, dst


def mask_of(text):
    m = 0
    for v in host.rules_components_to_values(text):
        m |= 1 << v
    return m


def engine_case(eng, G, layout, and_rounds, args, copy_gbs, gen_repeats, modes):
    eng.configure(G, layout)
    packed = layout == 0

    def generate():
        w = host.random_fill(G ** 3 // 32, seed=7, and_rounds=and_rounds)
        return w if packed else ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint32).ravel()

    t_gen = []
    for _ in range(gen_repeats):
        t0 = time.perf_counter(); words = generate(); t_gen.append(time.perf_counter() - t0)
    eng.seed_state(7, and_rounds)
    if G <= 1024 and not np.array_equal(eng.read_state(), words):
        raise SystemExit(f"{G}^3: the seeded state differs from the host's")
    once, keep = h2d_alone(words)
    t_seed, t_h2d, t_up, digests = {m: [] for m in modes}, [], [], {host.state_summary(G, words, layout=layout)["digest"]} if G <= 1024 else set()
    for _ in range(args.repeats):
        for m in modes:
            t_seed[m].append(per_call(lambda: eng.seed_state(7, and_rounds), eng.synchronize, args.calls))
            digests.add(eng.summary().digest)
        t_h2d.append(once())
        t0 = time.perf_counter(); eng.upload_state(words); t_up.append(time.perf_counter() - t0)
    del keep
    if len(digests) != 1:
        raise SystemExit(f"{G}^3: repeated seeds left different states (digests {digests})")
    state_bytes = words.nbytes
    s = statistics.median(t_seed["default"])
    row = {"case": f"{'packed' if packed else 'unpacked'} {G}^3", "and_rounds": and_rounds, "state_mib": state_bytes / 2 ** 20,
           "seed": {m: med(t) for m, t in t_seed.items()}, "seed_calls_per_measurement": args.calls,
           "parent": {"host_generation": med(t_gen), "h2d_copy_alone": med(t_h2d), "upload_state_call": med(t_up)},
           "h2d_alone_over_seed": statistics.median(t_h2d) / s,
           "seed_written_gb_per_s": 2 * state_bytes / s / 1e9, "measure_copy_gb_per_s": copy_gbs,
           "share_of_measured_copy": 2 * state_bytes / s / 1e9 / copy_gbs, "share_of_8_tb_per_s": 2 * state_bytes / s / 8e12}
    print(json.dumps(row), flush=True)
    return row


def ensemble_case(B, args):
    ens = Ensemble(0)
    ens.configure(B)
    seeds, rounds = 1 + np.arange(B), np.array([(0, 2, 5)[u % 3] for u in range(B)])
    born, survive = [mask_of(RULES[u % 10][0]) for u in range(B)], [mask_of(RULES[u % 10][1]) for u in range(B)]

    def generate():
        return np.stack([host.random_fill(W, seed=1 + u, and_rounds=(0, 2, 5)[u % 3]) for u in range(B)])

    def rules_one_by_one():
        for u in range(B):
            ens.set_rule_strings(u, born=RULES[u % 10][0], survive=RULES[u % 10][1])

    # the C calls themselves, their arguments built once: what a host that keeps its spec array pays per sweep
    lib, u32p = _capi.load(), C.POINTER(C.c_uint32)
    specs = (_capi.SeedStruct * B)(*[_seed_spec(64, int(a), int(b)) for a, b in zip(seeds, rounds)])
    born_a, survive_a = np.array(born, dtype=np.uint32), np.array(survive, dtype=np.uint32)

    def seed_call():
        _capi.check(lib.ca3d_ensemble_seed_state(ens._h, 0, B, specs, B))

    def tables_call():
        _capi.check(lib.ca3d_ensemble_set_rule_tables(ens._h, 0, B, born_a.ctypes.data_as(u32p), survive_a.ctypes.data_as(u32p), B))

    words = generate()
    ens.seed_states(0, seeds, rounds)
    if not np.array_equal(ens.read_state(), words):
        raise SystemExit(f"B = {B}: the seeded universes differ from the host's")
    once, keep = h2d_alone(words.reshape(-1))
    t_gen, t_seed, t_h2d, t_up, t_tab, t_str = [], [], [], [], [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter(); generate(); t_gen.append(time.perf_counter() - t0)
        t_seed.append(per_call(seed_call, ens.synchronize, args.calls))
        t_h2d.append(once())
        t0 = time.perf_counter(); ens.upload_state(0, words); t_up.append(time.perf_counter() - t0)
        t_tab.append(per_call(tables_call, ens.synchronize, args.calls))
        t0 = time.perf_counter(); rules_one_by_one(); t_str.append(time.perf_counter() - t0)
    del keep
    ens.close()
    s = statistics.median(t_seed)
    row = {"case": f"ensemble of {B}", "state_mib": words.nbytes / 2 ** 20, "seed": {"default": med(t_seed)}, "seed_calls_per_measurement": args.calls,
           "seed_includes": "ca3d_ensemble_seed_state with one spec per universe: the spec copy, the fill and the zero-step record launch",
           "parent": {"host_generation": med(t_gen), "h2d_copy_alone": med(t_h2d), "upload_state_call": med(t_up)},
           "h2d_alone_over_seed": statistics.median(t_h2d) / s,
           "rules": {"set_rule_tables_one_call": med(t_tab), "set_rule_strings_B_calls": med(t_str), "ratio": statistics.median(t_str) / statistics.median(t_tab)}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--universes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--repeats", type=int, default=5, help="alternating measurements per path; the median is reported")
    ap.add_argument("--calls", type=int, default=20, help="seed calls per measurement (one synchronise at the end)")
    ap.add_argument("--gen-repeats-large", type=int, default=1, help="host generations timed on grids of 1024 and up (numpy needs seconds per call there)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    eng = Engine(0)
    eng.configure(64)
    copy_gbs = eng.measure_copy(1 << 30, 8)
    rows = []
    for G in args.grids:
        for and_rounds in (0, 5):
            large = G >= 1024
            if large and and_rounds:
                gen = 0  # the copy does not depend on the density; six rounds of numpy hashing at this size are not worth the wait
            else:
                gen = args.gen_repeats_large if large else args.repeats
            modes = ["default"]
            if gen == 0:
                # reuse the and_rounds 0 words as the copy's payload
                rows.append(engine_case_no_generation(eng, G, and_rounds, args, copy_gbs, modes))
            else:
                rows.append(engine_case(eng, G, 0, and_rounds, args, copy_gbs, gen, modes))
    rows.append(engine_case(eng, 512, LAYOUT_UNPACKED, 0, args, copy_gbs, args.gen_repeats_large, ["default"]))
    eng.configure(32)
    eng.close()
    for B in args.universes:
        rows.append(ensemble_case(B, args))
    result = {"what": "seed_state on the device against host.random_fill + upload_state (the parent commit's path)", "date": datetime.date.today().isoformat(),
              "commit": commit, "device": "MI355X (gfx950)", "kernels": "ca_seed_packed / ca_seed_unpacked / ca_seed_ensemble (csrc/ca_seed.hip)",
              "timing": f"host clock; seed: {args.calls} calls + one synchronise per measurement; medians of {args.repeats} alternating measurements, min / max given",
              "bar": "parent.h2d_copy_alone: the host-to-device copy of the state without generation and without the second buffer's copy",
              "measure_copy_gb_per_s": copy_gbs, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


def engine_case_no_generation(eng, G, and_rounds, args, copy_gbs, modes):
    """A packed case whose host generation is not timed: the seed alone (its time depends on and_rounds, the copy's does not)."""
    eng.configure(G)
    t_seed, digests = {m: [] for m in modes}, set()
    for _ in range(args.repeats):
        for m in modes:
            t_seed[m].append(per_call(lambda: eng.seed_state(7, and_rounds), eng.synchronize, args.calls))
            digests.add(eng.summary().digest)
    if len(digests) != 1:
        raise SystemExit(f"{G}^3: repeated seeds left different states (digests {digests})")
    state_bytes = G ** 3 // 8
    s = statistics.median(t_seed["default"])
    row = {"case": f"packed {G}^3", "and_rounds": and_rounds, "state_mib": state_bytes / 2 ** 20, "seed": {m: med(t) for m, t in t_seed.items()},
           "seed_calls_per_measurement": args.calls, "parent": "as the and_rounds 0 row of this grid (the copy does not depend on the density; generation not timed)",
           "seed_written_gb_per_s": 2 * state_bytes / s / 1e9, "measure_copy_gb_per_s": copy_gbs,
           "share_of_measured_copy": 2 * state_bytes / s / 1e9 / copy_gbs, "share_of_8_tb_per_s": 2 * state_bytes / s / 8e12}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
