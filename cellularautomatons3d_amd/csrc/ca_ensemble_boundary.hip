// The ensemble kernels of the two boundaries ca_ensemble.hip does not hold (include/ca3d.h, ca3d_ensemble_set_boundary): *_torus, all
// six faces wrap, and *_closed, all six faces dead. They are ca_ensemble.hip's kernels word for word — ensemble_run of
// ca_ensemble_run.inc, the Step policies of ca_ensemble_step.inc — with the policy's boundary parameter set: three kinds (von Neumann,
// Moore, clustered) x four forms (plain, *_cycle, *_trace, *_moving) x two boundaries, 24 kernels. A unit of its own, so that the build
// compiles it beside ca_ensemble.hip and that unit's twelve kernels stay what they were.
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

static_assert(kBoundaryTorus == CA3D_ENSEMBLE_BOUNDARY_TORUS && kBoundaryClosed == CA3D_ENSEMBLE_BOUNDARY_CLOSED, "the policies' boundary is the ABI's");

// a kind's four forms under one boundary; four waves per SIMD as in ca_ensemble.hip
#define CA3D_ENSEMBLE_FORMS(kind, name, Step)                                                                                                     \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_##kind##64_##name(EnsembleArgs a) { ensemble_run<Step, false, false>(a); }          \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_##kind##64_cycle_##name(EnsembleArgs a) { ensemble_run<Step, true, false>(a); }     \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_##kind##64_trace_##name(EnsembleArgs a) { ensemble_run<Step, false, true>(a); }     \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_##kind##64_moving_##name(EnsembleArgs a) { ensemble_run<Step, true, false, true>(a); }
CA3D_ENSEMBLE_FORMS(vn, torus, VnStepT<kBoundaryTorus>)
CA3D_ENSEMBLE_FORMS(moore, torus, MooreStepT<kBoundaryTorus>)
CA3D_ENSEMBLE_FORMS(clustered, torus, ClusteredStepT<kBoundaryTorus>)
CA3D_ENSEMBLE_FORMS(vn, closed, VnStepT<kBoundaryClosed>)
CA3D_ENSEMBLE_FORMS(moore, closed, MooreStepT<kBoundaryClosed>)
CA3D_ENSEMBLE_FORMS(clustered, closed, ClusteredStepT<kBoundaryClosed>)
#undef CA3D_ENSEMBLE_FORMS

} // namespace

const void *ensemble_boundary_kernel(int boundary, int kind, int form)
{
	typedef void (*Kernel)(EnsembleArgs);
#define CA3D_ENSEMBLE_ROW(kind, name) {ca_ensemble_##kind##64_##name, ca_ensemble_##kind##64_cycle_##name, ca_ensemble_##kind##64_trace_##name, ca_ensemble_##kind##64_moving_##name}
	static const Kernel kernels[2][3][4] = {{CA3D_ENSEMBLE_ROW(vn, torus), CA3D_ENSEMBLE_ROW(moore, torus), CA3D_ENSEMBLE_ROW(clustered, torus)},
	                                        {CA3D_ENSEMBLE_ROW(vn, closed), CA3D_ENSEMBLE_ROW(moore, closed), CA3D_ENSEMBLE_ROW(clustered, closed)}};
#undef CA3D_ENSEMBLE_ROW
	if ((boundary != CA3D_ENSEMBLE_BOUNDARY_TORUS && boundary != CA3D_ENSEMBLE_BOUNDARY_CLOSED) || kind < 0 || kind > 2 || form < 0 || form > 3) return nullptr;
	return (const void *)kernels[boundary - CA3D_ENSEMBLE_BOUNDARY_TORUS][kind][form];
}

} // namespace ca3d
