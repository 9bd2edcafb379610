// The torus forms of the census and isolate kernels, behind ca3d_ensemble_census_connected and ca3d_ensemble_isolate_connected with
// CA3D_CONNECT_TORUS (include/ca3d.h): objects join across the faces of the 64^3 universe, adjacency being the
// 26-neighbourhood of Z_64^3. A unit of its own, so that ca_census.hip and ca_isolate.hip hold the one kernel each they held and their
// listings stay what they were.
//
// Layout, flood fill, extent join and the invariants they keep (every barrier reached by all 1024 threads, every loop exit read from LDS
// behind a barrier, no waits on other workgroups, no atomics) are ca_flood.inc's: both kernels CALL load_universe, seed_cell,
// flood<true> and extent, and read the cyclic box of an object from extent's masks with torus_span. What differs from the closed
// kernels besides the flood's three operands: the census' digest ROTATES a row where the closed form shifts it and takes the word's
// index modulo 64, box_max is box_min + e - 1 unreduced, and isolate's write reads its image rows modulo 64 and rotates them, so the
// object arrives in one piece.
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
#include "ca_digest.h"

constexpr u32 kNone = 0xFFFFFFFFu; // "no live cell" among first-cell keys (a key is below 2^18)

__device__ __forceinline__ u64 rotl64(u64 v, u32 s) { return v << (s & 63u) | v >> ((64u - s) & 63u); } // s = 0: v | v
__device__ __forceinline__ u64 rotr64(u64 v, u32 s) { return rotl64(v, 64u - s); }

struct CensusTorusArgs
{
	const u32 *state;    // [B][8192], the ensemble's current states
	ca3d_component *out; // [count][max_components]
	u32 *n_components, *remaining; // [count]
	u32 first, max_components;
};

// ca_ensemble_census64's rounds — SEED, FLOOD, RECORD, REMOVE (ca_census.hip) — on the torus.
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_census64_torus(CensusTorusArgs a)
{
	__shared__ __attribute__((aligned(16))) u32 xch[kXchWords];
	__shared__ __attribute__((aligned(16))) u32 flg[kFlgWords];
	__shared__ __attribute__((aligned(16))) u32 sed[kWaves];      // a wave's lowest first-cell key
	__shared__ __attribute__((aligned(16))) u32 part[kPartWords];  // the extent join's partials; at the end, a wave's rest of R
	__shared__ u64 dig[kWaves];
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const u32 *mine = a.state + (size_t)(a.first + blockIdx.x) * kEnsembleWords;
	ca3d_component *out = a.out + (size_t)blockIdx.x * a.max_components;

	u32 R[kPT][2], F[kPT][2];
	load_universe(mine, wave, row, R);

	u32 n = 0; // components listed so far: counted alike by every thread
	for (; n < a.max_components; n++)
	{
		// ---- seed: the lowest live cell of R, key = x + 64 y + 4096 z, the thread's own taken from the top down
		u32 key = kNone;
#pragma unroll
		for (int p = (int)kPT - 1; p >= 0; p--)
#pragma unroll
			for (int h = 1; h >= 0; h--)
				if (R[p][h]) key = ((wave * kPT + (u32)p) * 64u + row) * 64u + (u32)h * 32u + (u32)__builtin_ctz(R[p][h]);
		key = wave_min(key);
		// (sed is read behind the barrier below and rewritten a round later: the flood's barriers lie in between)
		if (row == 0u) sed[wave] = key;
		__syncthreads();
		const uint4 *s4 = reinterpret_cast<const uint4 *>(sed);
		u32 first_cell = kNone;
#pragma unroll
		for (u32 i = 0; i < kWaves / 4u; i++) { const uint4 v = s4[i]; first_cell = min(min(first_cell, v.x), min(min(v.y, v.z), v.w)); }
		first_cell = (u32)__builtin_amdgcn_readfirstlane((int)first_cell);
		if (first_cell == kNone) break; // R is empty — read from LDS behind the barrier: every thread leaves here, or none
		seed_cell(F, first_cell, wave, row);

		flood<true>(R, F, xch, flg, wave, row);

		// ---- record: population and the cyclic box (F holds its seed: no mask is empty) ...
		const Extent e = extent(F, part, wave, row);
		const TorusSpan sx = torus_span((u64)e.x1 << 32 | e.x0), sy = torus_span(e.ym), sz = torus_span(e.zm);
		const u32 cmin = sx.lo | sy.lo << 8 | sz.lo << 16;
		const u32 cmax = (sx.lo + sx.e - 1u) | (sy.lo + sy.e - 1u) << 8 | (sz.lo + sz.e - 1u) << 16; // not reduced: >= 64 through a seam, 126 at most
		// ... then the digest of the component translated cyclically by -box_min: the row's 64 bits rotated right by x0, the word's
		// index taken from ((y - y0) & 63, (z - z0) & 63).
		u64 d = 0;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
		{
			const u64 r64 = rotr64((u64)F[p][1] << 32 | F[p][0], sx.lo);
			const u32 idx = (((wave * kPT + p - sz.lo) & 63u) * 64u + ((row - sy.lo) & 63u)) * 2u;
			if ((u32)r64) d += digest_mix((u64)idx, (u32)r64);
			if ((u32)(r64 >> 32)) d += digest_mix((u64)(idx + 1u), (u32)(r64 >> 32));
		}
		d = wave_add(d);
		// (dig and part are rewritten a round later: the next round's seed barrier and flood barriers lie in between)
		if (row == 0u) dig[wave] = d;
		__syncthreads();
		if (tid == 0u)
		{
			u64 sum = 0;
#pragma nounroll
			for (u32 w = 0; w < kWaves; w++) sum += dig[w];
			uint4 *o4 = reinterpret_cast<uint4 *>(out + n); // 32 bytes: population, first_cell, box_min, box_max | digest, reserved[2]
			o4[0] = make_uint4(e.pop, first_cell, cmin, cmax);
			o4[1] = make_uint4((u32)sum, (u32)(sum >> 32), 0u, 0u);
		}

		// ---- remove
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++) R[p][h] &= ~F[p][h];
	}

	// ---- the slots behind the list are zero; remaining = what R still holds
	{
		uint4 *z4 = reinterpret_cast<uint4 *>(out);
		for (u32 i = 2u * n + tid; i < 2u * a.max_components; i += kThreads) z4[i] = make_uint4(0u, 0u, 0u, 0u); // inside the universe's max_components records
	}
	u32 rest = 0;
#pragma unroll
	for (u32 p = 0; p < kPT; p++) rest += (u32)__popc(R[p][0]) + (u32)__popc(R[p][1]);
	rest = wave_add(rest);
	__syncthreads(); // (thread 0 may be reading dig for the last record)
	if (row == 0u) part[wave] = rest;
	__syncthreads();
	if (tid == 0u)
	{
		u32 sum = 0;
#pragma nounroll
		for (u32 w = 0; w < kWaves; w++) sum += part[w];
		a.remaining[blockIdx.x] = sum;
		a.n_components[blockIdx.x] = n;
	}
}

struct IsolateTorusArgs
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

// ca_ensemble_isolate64 (ca_isolate.hip) on the torus: the object is the torus component, the shift is applied modulo 64.
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_isolate64_torus(IsolateTorusArgs a)
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

	flood<true>(R, F, xch, flg, wave, row);

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
		const TorusSpan s[3] = {torus_span((u64)e.x1 << 32 | e.x0), torus_span(e.ym), torus_span(e.zm)};
		int d[3];
		for (int i = 0; i < 3; i++) d[i] = (a.placement == CA3D_ISOLATE_CENTRE ? (64 - (int)s[i].e) / 2 : 0) - (int)s[i].lo; // -63 .. 31
		dx = d[0]; dy = d[1]; dz = d[2];
	}

	// ---- the write: destination row (y, z) is image row ((y - dy) & 63, (z - dz) & 63) rotated left by dx & 63: every row has a
	// source, nothing is clipped.
	const size_t dst_off = (size_t)(a.dst_first + blockIdx.x) * kEnsembleWords;
	const u32 sy = (row - (u32)dy) & 63u;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const u32 z = wave * kPT + p, sz = (z - (u32)dz) & 63u;
		const uint2 v = *reinterpret_cast<const uint2 *>(xch + (sz * 64u + sy) * 2u); // sy, sz < 64: inside the image
		const u64 r64 = rotl64((u64)v.y << 32 | v.x, (u32)dx & 63u);
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

hipError_t launch_census_torus(const CensusLaunch &l, hipStream_t stream)
{
	if (l.count == 0 || l.max_components == 0 || l.max_components > kCensusMaxComponents) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_component) == 32, "ca3d_component is two 16-byte stores");
	CensusTorusArgs a;
	a.state = l.state;
	a.out = l.out;
	a.n_components = l.n_components;
	a.remaining = l.remaining;
	a.first = l.first;
	a.max_components = l.max_components;
	hipLaunchKernelGGL(ca_ensemble_census64_torus, dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_isolate_torus(const IsolateLaunch &l, hipStream_t stream)
{
	if (l.n_jobs == 0 || l.placement > CA3D_ISOLATE_ORIGIN || l.rule_words > 6u) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_isolated) == 16 && sizeof(ca3d_isolate_job) == 8, "a result is one 16-byte store");
	IsolateTorusArgs a;
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
	hipLaunchKernelGGL(ca_ensemble_isolate64_torus, dim3(l.n_jobs), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
