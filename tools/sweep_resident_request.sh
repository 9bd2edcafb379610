#!/bin/bash
# Where the 512^3 row-pair kernel asks for the next faces: builds tools/ubench/resident_probe.hip once per point of the sweep and runs
# mode 33 with launches of 4 096 steps (us per step; with the counter build, stale first polls per 1 000 steps of every wave of tile 37).
#   tools/sweep_resident_request.sh build      (needs hipcc only; binaries under tools/ubench/_build/, git-ignored)
#   tools/sweep_resident_request.sh run [OUT]  (on an MI355X; default OUT = build/resident_request_sweep.txt)
# Points: the order up to round 5 (pin0: request at the head of the pass) and planes 5 / 9 / 12 / 14 / 15 (= behind the pass) with the
# pin, each with CA3D_RES_PAIR_PRE0 = 2 / 0 / 1, each with and without -DCA3D_RES_COUNT_STALE; the general forms and the 512^3 class
# form with and without their pins. Every run has its own time limit and the script stops at the first run that fails.
set -o pipefail
cd "$(dirname "$0")/.."
B=tools/ubench/_build
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
POINTS="pin0_pre12 pin1_pre5 pin1_pre9 pin1_pre12 pin1_pre14 pin1_pre15"
if [ "$1" = build ]; then
	mkdir -p $B
	cc() { $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -I $B -I cellularautomatons3d_amd/csrc -I include "$@" || exit 1; }
	for pt in $POINTS; do
		pin=${pt#pin}; pin=${pin%%_*}; pre=${pt##*pre}
		for g in 0 1 2; do
			cc -DCA3D_RES_PAIR_PIN=$pin -DCA3D_RES_PAIR_PRE=$pre -DCA3D_RES_PAIR_PRE0=$g tools/ubench/resident_probe.hip -o $B/pair_${pt}_g${g}_c0 &
			cc -DCA3D_RES_PAIR_PIN=$pin -DCA3D_RES_PAIR_PRE=$pre -DCA3D_RES_PAIR_PRE0=$g -DCA3D_RES_COUNT_STALE=1 tools/ubench/resident_probe.hip -o $B/pair_${pt}_g${g}_c1 &
		done
		wait
	done
	for pin in 0 1; do cc -DCA3D_RES_PIN_PASS=$pin tools/ubench/resident_probe.hip -o $B/general_pin$pin & done
	python3 tools/run_class_probe.py --build-only # writes $B/ca_jit_rule.inc
	D=$(python3 - <<'PY'
t = (0x000000F0, 0x000000E0, 0x0038, 0x0010, 0x0014, 0x0008)
print("-DCA3D_JIT=1 -DCA3D_JIT_MAIN=2 -DCA3D_JIT_E=true -DCA3D_JIT_C=true " + " ".join(f"-DCA3D_JIT_{n}={v}u" for n, v in zip(["TS0", "TB0", "TS1", "TB1", "TS2", "TB2"], t)))
PY
)
	for pin in 0 1; do cc $D -DCA3D_RC_PIN_SWEEP=$pin tools/ubench/resident_class_probe.hip -o $B/class_pin$pin & done
	wait
	exit 0
fi
[ "$1" = run ] || { echo "usage: $0 build | run [OUT]"; exit 2; }
out=${2:-build/resident_request_sweep.txt}
mkdir -p "$(dirname "$out")"
: > "$out"
one() { # name, time limit, arguments
	echo "== $1 ${*:3}" >> "$out"
	timeout -k 10 "$2" $B/$1 "${@:3}" >> "$out" 2>&1
	rc=$?
	if [ $rc -ne 0 ]; then echo "FAILED rc=$rc $1" | tee -a "$out"; exit $rc; fi
}
for pt in $POINTS; do for g in 2 0 1; do for c in 0 1; do one pair_${pt}_g${g}_c${c} 60 4096 6 33; done; done; done
for n in general_pin0 general_pin1; do one $n 60 4096 4 32; one $n 60 4096 4 16; one $n 60 4096 4 32 2; one $n 60 4096 4 16 2; done
for n in class_pin0 class_pin1; do one $n 90 2048 4 512 1; done
echo "done: $out"
