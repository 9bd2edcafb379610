// Census kernel behind ca3d_ensemble_census (include/ca3d.h): the connected objects of a 64^3 universe, one by one, ONE workgroup a
// universe, in one launch.
//
// Layout, extent join and the invariants (every barrier reached by all 1024 threads, every loop exit read from LDS behind a barrier, no
// waits on other workgroups, no atomics) are ca_flood.inc's. R[4][2] holds the cells no listed component has taken yet, F[4][2] the
// component being filled.
//
// The row loads, the seed and the flood loop are TEXT in this kernel, not calls. Called, ca_flood.inc's load_universe, seed_cell and
// flood compute the same, but the compiler allocates this kernel's registers differently and the census measured 1.3 to 4.5 % slower on
// an MI355X. The flood loop, the long one, exists once all the same: it is the fragment ca_flood_loop.inc, flood's
// body, included below under Torus = false, and the kernel's listing is the measured one line for line. The six lines of load_universe
// and the seven of seed_cell stay written out: even one of them as a call moves this listing (21 and 24 lines of it).
//
// One round of the loop: SEED (the lowest live cell of R in the order z, y, x: thread -> wave -> LDS -> workgroup), FLOOD, RECORD
// (population and box, then — the box known — the digest of the component translated to the origin; thread 0 stores the 32 bytes),
// REMOVE (R &= ~F). The round count n is counted alike by every thread, the empty-R exit is read from LDS behind the seed's barrier;
// there are max_components rounds at most, each with a flood of population + 1 iterations at most.
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

struct CensusArgs
{
	const u32 *state;    // [B][8192], the ensemble's current states
	ca3d_component *out; // [count][max_components]
	u32 *n_components, *remaining; // [count]
	u32 first, max_components;
};

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_census64(CensusArgs a)
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
#pragma unroll
	for (u32 p = 0; p < kPT; p++) // (load_universe)
	{
		const uint2 v = *reinterpret_cast<const uint2 *>(mine + ((size_t)((wave * kPT + p) * 64u + row)) * 2u);
		R[p][0] = v.x; R[p][1] = v.y;
	}

	u32 n = 0; // components listed so far: counted alike by every thread
	for (; n < a.max_components; n++)
	{
		// ---- seed: the lowest live cell of R, key = x + 64 y + 4096 z (the bit order of the packed state). The thread's own lowest
		// is in its lowest plane, then word, then bit — taken from the top down, so that the lowest is assigned last.
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
		{ // (seed_cell)
			const u32 sz = first_cell >> 12, sy = (first_cell >> 6) & 63u, sx = first_cell & 63u;
			const bool own = wave == (sz >> 2) && row == sy;
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
#pragma unroll
				for (u32 h = 0; h < 2u; h++) F[p][h] = own && p == (sz & 3u) && h == (sx >> 5) ? 1u << (sx & 31u) : 0u;
		}

		// ---- flood (flood's body, the closed form): F <- R & dilate(F) until an iteration changes nothing anywhere. Iteration k carries the waves' "changed in
		// iteration k - 1" bits in the exchange buffer of its parity, so the barrier of the exchange is the barrier of the test.
		{
			constexpr bool Torus = false;
#include "ca_flood_loop.inc"
		}

		// ---- record: population and box first (F holds its seed: nothing below is taken of an empty word pair) ...
		const Extent e = extent(F, part, wave, row);
		const u32 cpop = e.pop;
		const u32 cmin = (e.x0 ? (u32)__builtin_ctz(e.x0) : 32u + (u32)__builtin_ctz(e.x1)) | (u32)__builtin_ctzll(e.ym) << 8 | (u32)__builtin_ctzll(e.zm) << 16;
		const u32 cmax = (e.x1 ? 63u - (u32)__builtin_clz(e.x1) : 31u - (u32)__builtin_clz(e.x0)) | (63u - (u32)__builtin_clzll(e.ym)) << 8 |
		                 (63u - (u32)__builtin_clzll(e.zm)) << 16;
		// ... then the digest of the component translated by -box_min: the row's 64 bits shifted right by x0, the word's index taken
		// from (y - y0, z - z0). A word outside the box is zero and adds nothing.
		u64 d = 0;
		{
			const u32 bx = cmin & 0xFFu, by = (cmin >> 8) & 0xFFu, bz = cmin >> 16;
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const u64 r64 = ((u64)F[p][1] << 32 | F[p][0]) >> bx;
				const u32 idx = ((wave * kPT + p - bz) * 64u + (row - by)) * 2u;
				if ((u32)r64) d += digest_mix((u64)idx, (u32)r64);
				if ((u32)(r64 >> 32)) d += digest_mix((u64)(idx + 1u), (u32)(r64 >> 32));
			}
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
			o4[0] = make_uint4(cpop, first_cell, cmin, cmax);
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

} // namespace

hipError_t launch_census(const CensusLaunch &l, hipStream_t stream)
{
	if (l.connectivity == CA3D_CONNECT_TORUS) return launch_census_torus(l, stream);
	if (l.connectivity != CA3D_CONNECT_CLOSED) return hipErrorInvalidValue;
	if (l.count == 0 || l.max_components == 0 || l.max_components > kCensusMaxComponents) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_component) == 32, "ca3d_component is two 16-byte stores");
	CensusArgs a;
	a.state = l.state;
	a.out = l.out;
	a.n_components = l.n_components;
	a.remaining = l.remaining;
	a.first = l.first;
	a.max_components = l.max_components;
	hipLaunchKernelGGL(ca_ensemble_census64, dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
