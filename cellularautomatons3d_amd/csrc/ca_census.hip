// Census kernel behind ca3d_ensemble_census (include/ca3d.h): the connected objects of a 64^3 universe, one by one, ONE workgroup a
// universe, in one launch.
//
// The universe lies in registers as the ensemble kernels hold it (ca_ensemble.hip): 1024 threads, lane = row y, wave w = planes 4 w ..
// 4 w + 3, a row's two words in one thread. A thread holds R[4][2], the cells no listed component has taken yet, and F[4][2], the
// component being filled. A component is found by a flood fill, F <- R & dilate(F) until nothing changes; the 3 x 3 x 3 dilation is
// the step's neighbour access with ORs in place of the count: v_alignbit along x, wave-wide DPP along y, the double-buffered LDS
// exchange (laid out like VnStep's) along z. ALL SIX FACES ARE CLOSED — not the step's boundary: word 1's right neighbour, row 63's
// y + 1 and plane 63's z + 1 shift in zero where the step wraps.
//
// One round of the loop: SEED (the lowest live cell of R in the order z, y, x: thread -> wave -> LDS -> workgroup), FLOOD (one barrier
// an iteration; a wave's "anything changed" bit rides the exchange), RECORD (population and box, then — the box known — the digest
// of the component translated to the origin; thread 0 stores the 32 bytes), REMOVE (R &= ~F).
//
// Every condition that ends a loop is read from LDS behind a barrier, or counted alike by every thread: all 1024 threads reach every
// __syncthreads(). An iteration that does not end a flood adds a cell, so a flood takes population + 1 iterations at most, and there
// are max_components rounds at most. No waits on other workgroups, no spins, no atomics, nothing but vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
#include "ca_bitops.inc"
#include "ca_digest.h"

typedef unsigned long long u64;

constexpr u32 kThreads = 1024, kWaves = 16, kPT = 4; // threads, waves, planes per wave
constexpr u32 kNone = 0xFFFFFFFFu;                   // "no live cell" among first-cell keys (a key is below 2^18)

struct CensusArgs
{
	const u32 *state;    // [B][8192], the ensemble's current states
	ca3d_component *out; // [count][max_components]
	u32 *n_components, *remaining; // [count]
	u32 first, max_components;
};

template <typename T>
__device__ __forceinline__ T wave_add(T v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ u32 wave_or(u32 v)
{
	for (int o = 32; o > 0; o >>= 1) v |= (u32)__shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ u32 wave_min(u32 v)
{
	for (int o = 32; o > 0; o >>= 1) v = min(v, (u32)__shfl_xor(v, o));
	return v;
}
// sum / OR over a row of 16 lanes, left in every lane of the row (ca_ensemble.hip's)
__device__ __forceinline__ u32 row16_sum(u32 v)
{
	v += dpp_mov<1 | (0 << 2) | (3 << 4) | (2 << 6)>(v); // quad_perm:[1,0,3,2]
	v += dpp_mov<2 | (3 << 2) | (0 << 4) | (1 << 6)>(v); // quad_perm:[2,3,0,1]
	v += dpp_mov<0x141>(v);                              // row_half_mirror
	v += dpp_mov<0x140>(v);                              // row_mirror
	return v;
}
__device__ __forceinline__ u32 row16_or(u32 v)
{
	v |= dpp_mov<1 | (0 << 2) | (3 << 4) | (2 << 6)>(v);
	v |= dpp_mov<2 | (3 << 2) | (0 << 4) | (1 << 6)>(v);
	v |= dpp_mov<0x141>(v);
	v |= dpp_mov<0x140>(v);
	return v;
}

// the exchange: [iteration parity][wave][first / last plane][word][row], VnStep's
constexpr u32 kXchWords = 2u * kWaves * 2u * 2u * 64u; // 32 KiB
__device__ __forceinline__ u32 slot(u32 buf, u32 w, u32 which, u32 h, u32 row) { return (((buf * kWaves + w) * 2u + which) * 2u + h) * 64u + row; }

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_census64(CensusArgs a)
{
	__shared__ __attribute__((aligned(16))) u32 xch[kXchWords];
	__shared__ __attribute__((aligned(16))) u32 flg[2u * kWaves]; // [iteration parity][wave]: the wave changed a cell in the iteration before
	__shared__ __attribute__((aligned(16))) u32 sed[kWaves];      // a wave's lowest first-cell key
	__shared__ __attribute__((aligned(16))) u32 part[kWaves * 8u]; // a wave's population, x-occupancy 0 and 1, y ballot low and high, z bits low and high
	__shared__ u64 dig[kWaves];
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const u32 *mine = a.state + (size_t)(a.first + blockIdx.x) * kEnsembleWords;
	ca3d_component *out = a.out + (size_t)blockIdx.x * a.max_components;

	u32 R[kPT][2], F[kPT][2];
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
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
		{
			const u32 sz = first_cell >> 12, sy = (first_cell >> 6) & 63u, sx = first_cell & 63u;
			const bool own = wave == (sz >> 2) && row == sy;
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
#pragma unroll
				for (u32 h = 0; h < 2u; h++) F[p][h] = own && p == (sz & 3u) && h == (sx >> 5) ? 1u << (sx & 31u) : 0u;
		}

		// ---- flood: F <- R & dilate(F) until an iteration changes nothing anywhere. Iteration k carries the waves' "changed in
		// iteration k - 1" bits in the exchange buffer of its parity, so the barrier of the exchange is the barrier of the test.
		u32 changed = 1u; // wave-uniform
		for (u32 it = 0;; it++)
		{
			const u32 buf = it & 1u;
			u32 Y[kPT][2]; // x and y of the dilation
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
#pragma unroll
				for (u32 h = 0; h < 2u; h++)
				{
					const u32 w = F[p][h], other = F[p][h ^ 1u];
					const u32 l = from_left(w, h ? other : 0u);  // cell x - 1: word 0's comes from nowhere, word 1's from word 0
					const u32 r = from_right(h ? 0u : other, w); // cell x + 1: word 0's from word 1, word 1's from nowhere (closed: no wrap)
					const u32 x = w | l | r;
					// row y - 1 (zero into row 0), row y + 1 (zero into row 63: wave_shl, not the step's wave_rol)
					Y[p][h] = x | dpp_mov<kDppWaveShr1>(x) | dpp_mov<kDppWaveShl1>(x);
				}
			xch[slot(buf, wave, 0u, 0u, row)] = Y[0][0];
			xch[slot(buf, wave, 0u, 1u, row)] = Y[0][1];
			xch[slot(buf, wave, 1u, 0u, row)] = Y[kPT - 1][0];
			xch[slot(buf, wave, 1u, 1u, row)] = Y[kPT - 1][1];
			if (row == 0u) flg[buf * kWaves + wave] = changed;
			// (a wave writes this parity's buffer again two iterations on, behind the next iteration's barrier, which no wave passes
			// before it has read this one's)
			__syncthreads();
			const uint4 *f4 = reinterpret_cast<const uint4 *>(flg + buf * kWaves);
			uint4 m = f4[0];
#pragma unroll
			for (u32 i = 1; i < kWaves / 4u; i++) { const uint4 v = f4[i]; m.x |= v.x; m.y |= v.y; m.z |= v.z; m.w |= v.w; }
			if (__builtin_amdgcn_readfirstlane((int)(m.x | m.y | m.z | m.w)) == 0) break; // from LDS behind the barrier: workgroup-uniform
			u32 below[2], above[2];
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				below[h] = wave ? xch[slot(buf, wave - 1u, 1u, h, row)] : 0u;                        // z == -1: closed
				above[h] = wave + 1u < kWaves ? xch[slot(buf, (wave + 1u) & (kWaves - 1u), 0u, h, row)] : 0u; // z == 64: closed (the step wraps here)
			}
			u32 ch = 0;
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
#pragma unroll
				for (u32 h = 0; h < 2u; h++)
				{
					const u32 z = Y[p][h] | (p ? Y[p ? p - 1u : 0u][h] : below[h]) | (p + 1u < kPT ? Y[p + 1u < kPT ? p + 1u : p][h] : above[h]);
					const u32 f = R[p][h] & z; // F is part of R and of its own dilation: f holds F
					ch |= f ^ F[p][h];
					F[p][h] = f;
				}
			changed = __ballot(ch != 0u) ? 1u : 0u;
		}

		// ---- record: population and box first ...
		u32 pop = 0, o0 = 0, o1 = 0, zb = 0;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
		{
			pop += (u32)__popc(F[p][0]) + (u32)__popc(F[p][1]); // (a thread's 256 cells, a wave's 16 384, the universe's 262 144: one word each)
			o0 |= F[p][0];
			o1 |= F[p][1];
			if (__ballot((F[p][0] | F[p][1]) != 0u)) zb |= 1u << p;
		}
		const u64 ymw = __ballot((o0 | o1) != 0u); // bit y: row y of one of the wave's planes holds a cell of F
		pop = wave_add(pop);
		o0 = wave_or(o0);
		o1 = wave_or(o1);
		if (row == 0u)
		{
			const u64 zmw = (u64)zb << (wave * kPT);
			uint4 *pw = reinterpret_cast<uint4 *>(part) + 2u * wave;
			pw[0] = make_uint4(pop, o0, o1, (u32)ymw);
			pw[1] = make_uint4((u32)(ymw >> 32), (u32)zmw, (u32)(zmw >> 32), 0u);
		}
		__syncthreads();
		// every wave joins the 16 partials for itself: lanes 0 .. 15 of every row of 16 take one wave's each, four DPP steps leave the
		// row's lanes with the whole, lane 0 is read (the *_moving kernels' join)
		u32 cpop, cmin, cmax;
		{
			const uint4 *pr = reinterpret_cast<const uint4 *>(part) + 2u * (row & 15u);
			const uint4 pa = pr[0], pb = pr[1];
			auto lane0 = [](u32 v) { return (u32)__builtin_amdgcn_readlane((int)v, 0); };
			cpop = lane0(row16_sum(pa.x));
			const u32 x0 = lane0(row16_or(pa.y)), x1 = lane0(row16_or(pa.z));
			const u64 ym = (u64)lane0(row16_or(pb.x)) << 32 | lane0(row16_or(pa.w));
			const u64 zm = (u64)lane0(row16_or(pb.z)) << 32 | lane0(row16_or(pb.y));
			// (F holds its seed: nothing below is taken of an empty word pair)
			cmin = (x0 ? (u32)__builtin_ctz(x0) : 32u + (u32)__builtin_ctz(x1)) | (u32)__builtin_ctzll(ym) << 8 | (u32)__builtin_ctzll(zm) << 16;
			cmax = (x1 ? 63u - (u32)__builtin_clz(x1) : 31u - (u32)__builtin_clz(x0)) | (63u - (u32)__builtin_clzll(ym)) << 8 |
			       (63u - (u32)__builtin_clzll(zm)) << 16;
		}
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
