#!/bin/bash
# Round-3 evidence on an MI355X box (from the repo root):  tools/profile_round3.sh r3_a [stats|pmc|all]
# Bench lines, rocprofv3 kernel stats, and PMC passes — one counter group per pass, never combined with --stats
# (MI355X_MICROARCH.md). The SQ passes of the resident kernels record how many steps their launches held
# (steps_per_launch): bench.py turns SQ_INSTS_VALU per step into the VALU-issue roofline of those kernels.
set -e -o pipefail
tag=${1:-r3_x}
what=${2:-all}
out=$PWD/gpurun_out
mkdir -p "$out"
export TMPDIR=/tmp
Q="--no-cpu-baseline --no-render --no-scaling-base --no-per-step-leg --no-per-call-leg --no-grid-256 --min-seconds 0.2"
DRV="bench.py --steps 20 --warmup 5"          # the driver's own command
SQ="SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY"
stats() { rocprofv3 --output-format csv --kernel-trace --stats -d "$out/${tag}_stats_$1" -o s -- python3 ${@:2} > "$out/${tag}_bench_$1_under_rocprof.json"; cp "$out/${tag}_stats_$1"/*/s_kernel_stats.csv "$out/${tag}_$1_kernel_stats.csv" 2>/dev/null || cp "$out/${tag}_stats_$1"/s_kernel_stats.csv "$out/${tag}_$1_kernel_stats.csv"; }
pmc() { rocprofv3 --output-format csv --pmc $2 --kernel-trace -d "$out/${tag}_pmc_$1" -o p -- python3 ${@:3} > /dev/null; }
if [ "$what" = stats ] || [ "$what" = all ]; then
  python3 $DRV > "$out/${tag}_bench512_driver_cmd.json"
  stats 512_driver_cmd $DRV $Q
  stats 512_perstep bench.py $Q --resident 0 --steps 512 --warmup 64
  stats 256_driver_cmd $DRV $Q --grid 256
  stats 1024 bench.py $Q --grid 1024 --steps 128 --warmup 32
  stats 512_clustered bench.py $Q --rule clustered --steps 256 --warmup 32
  stats 1024_clustered bench.py $Q --grid 1024 --rule clustered --steps 64 --warmup 16
  stats render bench.py --full --no-cpu-baseline --no-scaling-base --no-per-step-leg --no-per-call-leg --no-grid-256 --min-seconds 0.2 --steps 64 --warmup 8
  python3 bench.py --full --config 5 --steps 16 --warmup 4 --no-cpu-baseline --min-seconds 0.3 > "$out/${tag}_bench_config5_1gpu.json"
fi
if [ "$what" = pmc ] || [ "$what" = all ]; then
  pmc sq512res "$SQ" $DRV $Q
  python3 tools/pmc_sq_reduce.py "$out/${tag}_pmc_sq512res" ca_resident_vn 2060 > "$out/${tag}_pmc_sq_resident512.json"
  pmc sq256res "$SQ" $DRV $Q --grid 256
  python3 tools/pmc_sq_reduce.py "$out/${tag}_pmc_sq256res" ca_resident_vn256 2060 > "$out/${tag}_pmc_sq_resident256.json"
  pmc sq512cl "$SQ" bench.py $Q --rule clustered --steps 128 --warmup 16 --queue 1024
  python3 tools/pmc_sq_reduce.py "$out/${tag}_pmc_sq512cl" ca3d_jit_resident_class 1024 > "$out/${tag}_pmc_sq_clustered512.json"
  pmc sq1024cl "$SQ" bench.py $Q --grid 1024 --rule clustered --steps 32 --warmup 8
  python3 tools/pmc_sq_reduce.py "$out/${tag}_pmc_sq1024cl" ca3d_jit_ > "$out/${tag}_pmc_sq_clustered1024.json"
  pmc fetch512res FETCH_SIZE $DRV $Q
  pmc write512res WRITE_SIZE $DRV $Q
  python3 tools/pmc_reduce.py "ca_resident_vn@512" ca_resident_vn "$out/${tag}_pmc_fetch512res" "$out/${tag}_pmc_write512res" "$out/${tag}_pmc_traffic.json"
  pmc fetch512 FETCH_SIZE bench.py $Q --resident 0 --steps 256 --warmup 32
  pmc write512 WRITE_SIZE bench.py $Q --resident 0 --steps 256 --warmup 32
  python3 tools/pmc_reduce.py "ca_packed_vn@512" ca_packed_vn "$out/${tag}_pmc_fetch512" "$out/${tag}_pmc_write512" "$out/${tag}_pmc_traffic.json"
  pmc fetch1024cl FETCH_SIZE bench.py $Q --grid 1024 --rule clustered --steps 32 --warmup 8
  pmc write1024cl WRITE_SIZE bench.py $Q --grid 1024 --rule clustered --steps 32 --warmup 8
  python3 tools/pmc_reduce.py "ca3d_jit_tile@1024" ca3d_jit_ "$out/${tag}_pmc_fetch1024cl" "$out/${tag}_pmc_write1024cl" "$out/${tag}_pmc_traffic.json"
  bash tools/pmc_render.sh ${tag}_render > "$out/${tag}_pmc_render.json" 2>/dev/null
  rm -rf "$out"/${tag}_render_pmc_*
fi
find "$out" -name "*kernel_trace.csv" -delete; find "$out" -name "*counter_collection.csv" -delete; find "$out" -name "*agent_info.csv" -delete
echo done
