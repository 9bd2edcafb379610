// Isolate kernel behind ca3d_ensemble_isolate (include/ca3d.h): one connected object of a 64^3 universe, cut out and made the only thing
// in a universe of its own, ONE workgroup a job, every job of a call in one launch.
//
// The source universe lies in registers as the census holds it (ca_census.hip): 1024 threads, lane = row y, wave w = planes 4 w ..
// 4 w + 3, a row's two words in one thread. R[4][2] is the source, F[4][2] the object: F starts as the job's cell, if it is live, and
// grows by the census' flood fill, F <- R & dilate(F) until nothing changes — v_alignbit along x, wave-wide DPP along y with zero
// shifted in at both ends, the double-buffered LDS exchange along z, ALL SIX FACES CLOSED, one barrier an iteration with the waves'
// "changed" bits riding the exchange. Population and box follow by the census' two-step join, and from the box the shift.
//
// The write: F goes into LDS as a [z][y][2] image — into the exchange buffer, which is dead once the flood has ended: no thread reads it
// in the iteration that ends the flood, and every read of the iteration before lies in front of that iteration's barrier — behind ONE
// barrier (the join's) a thread assembles ITS destination rows (y, 4 w + p) from image rows (y - dy, z - dz), zero where that row lies
// outside the cube, shifts the row's 64 bits by dx and stores the two words to both ping-pong buffers of the destination universe.
// Every destination word is written exactly once, by one thread. Thread 0 stores the 16-byte result and copies the rule words.
//
// Every condition that ends the loop is read from LDS behind a barrier: all 1024 threads reach every __syncthreads(). An iteration
// that does not end the flood adds a cell, so it takes population + 2 iterations at most. No waits on other
// workgroups, no spins, no atomics, nothing but vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
#include "ca_bitops.inc"

typedef unsigned long long u64;

constexpr u32 kThreads = 1024, kWaves = 16, kPT = 4; // threads, waves, planes per wave

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

// the census' (ca_census.hip)
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

// the exchange: [iteration parity][wave][first / last plane][word][row], the census'; after the flood the same words hold the image
constexpr u32 kXchWords = 2u * kWaves * 2u * 2u * 64u; // 32 KiB
static_assert(kXchWords == kEnsembleWords, "the image of a universe fits the exchange buffer exactly");
__device__ __forceinline__ u32 slot(u32 buf, u32 w, u32 which, u32 h, u32 row) { return (((buf * kWaves + w) * 2u + which) * 2u + h) * 64u + row; }

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_isolate64(IsolateArgs a)
{
	__shared__ __attribute__((aligned(16))) u32 xch[kXchWords];
	__shared__ __attribute__((aligned(16))) u32 flg[2u * kWaves]; // [iteration parity][wave]: the wave changed a cell in the iteration before
	__shared__ __attribute__((aligned(16))) u32 part[kWaves * 8u]; // a wave's population, x-occupancy 0 and 1, y ballot low and high, z bits low and high
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const ca3d_isolate_job job = a.jobs[blockIdx.x]; // the host has checked universe and cell
	const u32 *mine = a.src_state + (size_t)job.universe * kEnsembleWords;

	u32 R[kPT][2], F[kPT][2];
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const uint2 v = *reinterpret_cast<const uint2 *>(mine + ((size_t)((wave * kPT + p) * 64u + row)) * 2u);
		R[p][0] = v.x; R[p][1] = v.y;
	}
	{
		const u32 sz = job.cell >> 12, sy = (job.cell >> 6) & 63u, sx = job.cell & 63u;
		const bool own = wave == (sz >> 2) && row == sy;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++) F[p][h] = own && p == (sz & 3u) && h == (sx >> 5) ? R[p][h] & 1u << (sx & 31u) : 0u; // a dead cell: F is empty
	}

	// ---- flood: F <- R & dilate(F) until an iteration changes nothing anywhere. Iteration k carries the waves' "changed in iteration
	// k - 1" bits in the exchange buffer of its parity, so the barrier of the exchange is the barrier of the test. An empty F changes
	// nothing in iteration 0 and ends the loop in iteration 1.
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
				// row y - 1 (zero into row 0), row y + 1 (zero into row 63)
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
			below[h] = wave ? xch[slot(buf, wave - 1u, 1u, h, row)] : 0u;                                    // z == -1: closed
			above[h] = wave + 1u < kWaves ? xch[slot(buf, (wave + 1u) & (kWaves - 1u), 0u, h, row)] : 0u; // z == 64: closed
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

	// ---- the image: the exchange buffer is dead — the iteration that ended the flood read none of it, and every wave has passed that
	// iteration's barrier only after all had finished the reads of the one before
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
		*reinterpret_cast<uint2 *>(xch + ((wave * kPT + p) * 64u + row) * 2u) = make_uint2(F[p][0], F[p][1]);

	// ---- population and box (the census' join); its barrier is the image's
	u32 pop = 0, o0 = 0, o1 = 0, zb = 0;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		pop += (u32)__popc(F[p][0]) + (u32)__popc(F[p][1]);
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
	u32 cpop;
	int dx = 0, dy = 0, dz = 0; // workgroup-uniform: read from lane 0 of what every wave joined for itself
	{
		const uint4 *pr = reinterpret_cast<const uint4 *>(part) + 2u * (row & 15u);
		const uint4 pa = pr[0], pb = pr[1];
		auto lane0 = [](u32 v) { return (u32)__builtin_amdgcn_readlane((int)v, 0); };
		cpop = lane0(row16_sum(pa.x));
		const u32 x0 = lane0(row16_or(pa.y)), x1 = lane0(row16_or(pa.z));
		const u64 ym = (u64)lane0(row16_or(pb.x)) << 32 | lane0(row16_or(pa.w));
		const u64 zm = (u64)lane0(row16_or(pb.z)) << 32 | lane0(row16_or(pb.y));
		if (cpop && a.placement != CA3D_ISOLATE_KEEP) // (an empty F has no box: the shift stays zero)
		{
			const u64 xm = (u64)x1 << 32 | x0;
			const int lo[3] = {(int)__builtin_ctzll(xm), (int)__builtin_ctzll(ym), (int)__builtin_ctzll(zm)};
			const int hi[3] = {63 - (int)__builtin_clzll(xm), 63 - (int)__builtin_clzll(ym), 63 - (int)__builtin_clzll(zm)};
			int d[3];
			for (int i = 0; i < 3; i++) d[i] = (a.placement == CA3D_ISOLATE_CENTRE ? (64 - (hi[i] - lo[i] + 1)) / 2 : 0) - lo[i];
			dx = d[0]; dy = d[1]; dz = d[2];
		}
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
