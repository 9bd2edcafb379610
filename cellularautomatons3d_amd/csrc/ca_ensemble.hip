// Ensemble kernel behind ca3d_ensemble_* (include/ca3d.h): B independent 64^3 universes, ONE workgroup each, in one launch.
//
// A universe is stepped exactly as resident64_run (ca_resident_kernel.inc) steps the lone 64^3 grid: 1024 threads hold its 32 KiB in
// eight registers each — lane = row y, wave w = planes 4 w .. 4 w + 3, a row's two words in one thread; x neighbours by v_alignbit,
// y neighbours by wave-wide DPP, z neighbours through a double-buffered LDS exchange with one barrier per step; - faces dead, + faces
// wrap. A workgroup waits for nobody outside itself, so a grid of B of them is B universes whatever part of it is resident at once.
// What differs from the lone-grid kernel:
//   * the RULE IS DATA. A universe's von Neumann table pair (7 + 7 bits) is read once per workgroup with a wave-uniform load and
//     expanded into 14 registers of all-zeros / all-ones (`leaf`); a word's update is then a multiplexer tree of v_bitop3 selects over
//     (alive, count planes 0, 1, 2): 7 selects on the alive word pick born / survive per count, 3 on plane 0, 2 on plane 1, 1 on
//     plane 2 (count 7 does not exist, so count 6's leaf needs no select on plane 0) — 13 instructions where the compiled rule needs 1
//     to 3, after the same 8 of the carry-save count and the same 4 neighbour shifts: 25 per word instead of ~12. No per-cell
//     extraction, no LDS table, and every select has ONE operand that is not a plain register.
//   * the SUMMARY comes out of the registers: at the end of a launch every workgroup reduces population, births / deaths against the
//     state one step earlier (held in registers across the last step), digest and bounding box — registers -> wave -> LDS -> thread 0,
//     which writes the universe's ca3d_summary with plain stores.
//   * STOPPING is decided per universe in the kernel: on entry from the stored record, then every check_every steps from a workgroup
//     reduction of two bits — any cell alive, any cell changed in the last step — at the price of one extra barrier per check. A
//     universe whose condition holds writes its state and record and leaves; the CU takes the next workgroup.
// There are no waits on other workgroups, no spins, and nothing but vector stores.
//
// Three kernels share everything but the step: ca_ensemble_vn64 (above), ca_ensemble_moore64, whose rule is a Moore table pair (27 + 27
// bits, two words per universe), and ca_ensemble_clustered64, whose rule is three pairs — main (Moore), edges, corners — ORed (six words).
// The body — entry check from the stored record, check points, record reduction, write-back — is ensemble_run<Step, Cycle, Trace>; a Step
// policy (VnStep, MooreStep, ClusteredStep) owns the rule's registers, the size of the LDS exchange and one step.
// The *_cycle kernels watch CA3D_STOP_PERIODIC as well, the *_moving kernels CA3D_STOP_MOVING on top of that; the *_trace kernels leave a
// sample (population, births, deaths) per check point.
// The body and the policies are ca_ensemble_run.inc and ca_ensemble_step.inc. This unit holds the twelve kernels of the reference boundary
// (- faces dead, + faces wrap); the *_torus and *_closed forms (ca3d_ensemble_set_boundary) are ca_ensemble_boundary.hip's, a unit of its
// own so that the two compile side by side. kernel_of below picks from both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
#include "ca_bitops.inc"
#include "ca_wave_ops.inc"
#include "ca_digest.h"
#include "ca_ensemble_run.inc"

// Four waves per SIMD = up to 128 registers = one workgroup per CU: cut for 64 registers (two per CU) the step loop spills
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_vn64(EnsembleArgs a) { ensemble_run<VnStep, false, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_moore64(EnsembleArgs a) { ensemble_run<MooreStep, false, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_vn64_cycle(EnsembleArgs a) { ensemble_run<VnStep, true, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_moore64_cycle(EnsembleArgs a) { ensemble_run<MooreStep, true, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_vn64_trace(EnsembleArgs a) { ensemble_run<VnStep, false, true>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_moore64_trace(EnsembleArgs a) { ensemble_run<MooreStep, false, true>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_clustered64(EnsembleArgs a) { ensemble_run<ClusteredStep, false, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_clustered64_cycle(EnsembleArgs a) { ensemble_run<ClusteredStep, true, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_clustered64_trace(EnsembleArgs a) { ensemble_run<ClusteredStep, false, true>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_vn64_moving(EnsembleArgs a) { ensemble_run<VnStep, true, false, true>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_moore64_moving(EnsembleArgs a) { ensemble_run<MooreStep, true, false, true>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_clustered64_moving(EnsembleArgs a) { ensemble_run<ClusteredStep, true, false, true>(a); }

// the one place that maps an ensemble's kind and boundary (and whether CA3D_STOP_PERIODIC or CA3D_STOP_MOVING is watched, or samples are
// recorded) to its kernel, a function of one EnsembleArgs; null for a boundary nobody knows
const void *kernel_of(int neighbourhood, bool clustered, int boundary, bool cycle, bool trace, bool moving = false)
{
	typedef void (*Kernel)(EnsembleArgs);
	static const Kernel reference[3][4] = {
		{ca_ensemble_vn64, ca_ensemble_vn64_cycle, ca_ensemble_vn64_trace, ca_ensemble_vn64_moving},
		{ca_ensemble_moore64, ca_ensemble_moore64_cycle, ca_ensemble_moore64_trace, ca_ensemble_moore64_moving},
		{ca_ensemble_clustered64, ca_ensemble_clustered64_cycle, ca_ensemble_clustered64_trace, ca_ensemble_clustered64_moving}};
	const int kind = clustered ? 2 : neighbourhood == CA3D_ENSEMBLE_MOORE ? 1 : 0;
	const int form = moving ? 3 : trace ? 2 : cycle ? 1 : 0; // (moving and cycle never with trace: launch_ensemble)
	if (boundary == CA3D_ENSEMBLE_BOUNDARY_REFERENCE) return (const void *)reference[kind][form];
	return ensemble_boundary_kernel(boundary, kind, form);
}

} // namespace

hipError_t launch_ensemble(const EnsembleLaunch &l, hipStream_t stream)
{
	// the *_moving kernels watch CA3D_STOP_PERIODIC too when the mask holds it: they are *_cycle kernels with one more condition
	const bool moving = (l.stop_mask & (uint32_t)CA3D_STOP_MOVING) != 0u;
	const bool cycle = moving || (l.stop_mask & (uint32_t)CA3D_STOP_PERIODIC) != 0u, trace = l.samples != nullptr;
	const bool checks = l.stop_mask || trace; // the launch has check points
	if (l.count == 0 || (l.clustered && l.neighbourhood != CA3D_ENSEMBLE_MOORE) || l.steps > kEnsembleMaxSteps || (checks && l.check_every == 0)) return hipErrorInvalidValue;
	if (cycle && (!l.anchor || !l.cycle || trace)) return hipErrorInvalidValue;
	// the last sample a universe can write is number ceil((base + steps) / check_every): inside its sample_stride slots, or no launch
	if (trace && ((uint64_t)l.base + l.steps + l.check_every - 1u) / l.check_every >= l.sample_stride) return hipErrorInvalidValue;
	const void *kernel = kernel_of(l.neighbourhood, l.clustered, l.boundary, cycle, trace, moving);
	if (!kernel) return hipErrorInvalidValue;
	EnsembleArgs a;
	a.state = l.state; a.prev = l.prev;
	a.rules = l.rules;
	a.records = l.records;
	a.steps_done = l.steps_done; a.reason = l.reason;
	a.first = l.first; a.steps = l.steps; a.base = l.base;
	a.check_every = l.check_every;
	a.stop_mask = l.stop_mask;
	const uint32_t into = checks ? l.base % l.check_every : 0u; // steps since the call's last check point
	a.first_check = into ? l.check_every - into : 0u;
	a.final = l.final ? 1u : 0u;
	a.reset = l.reset ? 1u : 0u;
	a.anchor = l.anchor;
	a.cycle = l.cycle;
	a.next_check = l.stop_mask ? l.base / l.check_every + (into ? 1u : 0u) : 0u; // launches are cut ON check points: one that ends a launch and opens the next counts once
	a.samples = l.samples;
	a.sample_stride = l.sample_stride;
	void *args[] = {&a};
	return hipLaunchKernel(kernel, dim3(l.count), dim3(kThreads), args, 0, stream);
}

int ensemble_workgroups_per_cu(int neighbourhood, bool clustered)
{
	int per_cu = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_of(neighbourhood, clustered, CA3D_ENSEMBLE_BOUNDARY_REFERENCE, false, false), (int)kThreads, 0) != hipSuccess)
	{
		(void)hipGetLastError();
		return 0;
	}
	return per_cu;
}

} // namespace ca3d
