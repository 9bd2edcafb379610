// Isolate kernel behind ca3d_ensemble_isolate (include/ca3d.h): one connected object of a 64^3 universe, cut out and made the only thing
// in a universe of its own, ONE workgroup a job, every job of a call in one launch.
//
// Layout, flood fill, extent join and the invariants they keep (every barrier reached by all 1024 threads, every loop exit read from LDS
// behind a barrier, no waits on other workgroups, no atomics) are ca_flood.inc's. R[4][2] is the source universe, F[4][2] the object: F
// starts as the job's cell, if it is live, and grows by the flood; an empty F ends it in iteration 1. From the extent follows the shift
// (DESIGN.md 12.8).
//
// The write: F goes into LDS as a [z][y][2] image — into the exchange buffer, which is dead once the flood has ended — behind ONE barrier
// (the extent join's) a thread assembles ITS destination rows (y, 4 w + p) from image rows (y - dy, z - dz), zero where that row lies
// outside the cube, shifts the row's 64 bits by dx and stores the two words to both ping-pong buffers of the destination universe.
// Every destination word is written exactly once, by one thread. Thread 0 stores the 16-byte result and copies the rule words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
#include "ca_bitops.inc"
#include "ca_wave_ops.inc"
#include "ca_flood.inc"

struct IsolateArgs
{
	const u32 *src_state;         // [Bs][8192], the source ensemble's current states
	u32 *dst_state, *dst_prev;    // [Bd][8192], both buffers of the destination ensemble
	const u32 *src_rules;         // [Bs][rule_words]
	u32 *dst_rules;               // [Bd][rule_words]
	const ca3d_isolate_job *jobs; // [n_jobs]
	ca3d_isolated *out;           // [n_jobs]
	u32 dst_first, placement, rule_words; // rule_words 0: rules stay
};

// after the flood the exchange buffer's words hold the image
static_assert(kXchWords == kEnsembleWords, "the image of a universe fits the exchange buffer exactly");

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_isolate64(IsolateArgs a)
{
	__shared__ __attribute__((aligned(16))) u32 xch[kXchWords];
	__shared__ __attribute__((aligned(16))) u32 flg[kFlgWords];
	__shared__ __attribute__((aligned(16))) u32 part[kPartWords];
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const ca3d_isolate_job job = a.jobs[blockIdx.x]; // the host has checked universe and cell
	const u32 *mine = a.src_state + (size_t)job.universe * kEnsembleWords;

	u32 R[kPT][2], F[kPT][2];
	load_universe(mine, wave, row, R);
	seed_cell(F, job.cell, wave, row);
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
#pragma unroll
		for (u32 h = 0; h < 2u; h++) F[p][h] &= R[p][h]; // a dead cell: F is empty

	flood(R, F, xch, flg, wave, row);

	// ---- the image (the exchange buffer is dead: see flood)
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
		*reinterpret_cast<uint2 *>(xch + ((wave * kPT + p) * 64u + row) * 2u) = make_uint2(F[p][0], F[p][1]);

	// ---- population and box. The barrier inside extent is also the image's: behind it every thread may read every image row.
	const Extent e = extent(F, part, wave, row);
	const u32 cpop = e.pop;
	int dx = 0, dy = 0, dz = 0; // workgroup-uniform, as e is
	if (cpop && a.placement != CA3D_ISOLATE_KEEP) // (an empty F has no box: the shift stays zero)
	{
		const u64 xm = (u64)e.x1 << 32 | e.x0;
		const int lo[3] = {(int)__builtin_ctzll(xm), (int)__builtin_ctzll(e.ym), (int)__builtin_ctzll(e.zm)};
		const int hi[3] = {63 - (int)__builtin_clzll(xm), 63 - (int)__builtin_clzll(e.ym), 63 - (int)__builtin_clzll(e.zm)};
		int d[3];
		for (int i = 0; i < 3; i++) d[i] = (a.placement == CA3D_ISOLATE_CENTRE ? (64 - (hi[i] - lo[i] + 1)) / 2 : 0) - lo[i];
		dx = d[0]; dy = d[1]; dz = d[2];
	}

	// ---- the write: destination row (y, z) is image row (y - dy, z - dz) shifted by dx. The translated box lies inside the cube, so
	// no live bit leaves the row's 64.
	const size_t dst_off = (size_t)(a.dst_first + blockIdx.x) * kEnsembleWords;
	const u32 sy = row - (u32)dy; // in 0 .. 63, or wrapped far above
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const u32 z = wave * kPT + p, sz = z - (u32)dz;
		u64 r64 = 0;
		if (sy < 64u && sz < 64u)
		{
			const uint2 v = *reinterpret_cast<const uint2 *>(xch + (sz * 64u + sy) * 2u);
			r64 = (u64)v.y << 32 | v.x;
		}
		r64 = dx >= 0 ? r64 << (u32)dx : r64 >> (u32)-dx; // |dx| <= 63
		const uint2 o = make_uint2((u32)r64, (u32)(r64 >> 32));
		const size_t at = dst_off + (size_t)(z * 64u + row) * 2u; // inside universe dst_first + job of the destination
		*reinterpret_cast<uint2 *>(a.dst_state + at) = o;
		*reinterpret_cast<uint2 *>(a.dst_prev + at) = o;
	}
	if (tid == 0u)
	{
		*reinterpret_cast<uint4 *>(a.out + blockIdx.x) = make_uint4(cpop, (u32)dx, (u32)dy, (u32)dz);
		const u32 *rs = a.src_rules + (size_t)job.universe * a.rule_words;
		u32 *rd = a.dst_rules + (size_t)(a.dst_first + blockIdx.x) * a.rule_words;
#pragma nounroll
		for (u32 i = 0; i < a.rule_words; i++) rd[i] = rs[i];
	}
}

} // namespace

hipError_t launch_isolate(const IsolateLaunch &l, hipStream_t stream)
{
	if (l.connectivity == CA3D_CONNECT_TORUS) return launch_isolate_torus(l, stream);
	if (l.connectivity != CA3D_CONNECT_CLOSED) return hipErrorInvalidValue;
	if (l.n_jobs == 0 || l.placement > CA3D_ISOLATE_ORIGIN || l.rule_words > 6u) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_isolated) == 16 && sizeof(ca3d_isolate_job) == 8, "a result is one 16-byte store");
	IsolateArgs a;
	a.src_state = l.src_state;
	a.dst_state = l.dst_state;
	a.dst_prev = l.dst_prev;
	a.src_rules = l.src_rules;
	a.dst_rules = l.dst_rules;
	a.jobs = l.jobs;
	a.out = l.out;
	a.dst_first = l.dst_first;
	a.placement = l.placement;
	a.rule_words = l.rule_words;
	hipLaunchKernelGGL(ca_ensemble_isolate64, dim3(l.n_jobs), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
