// State summary behind ca3d_summarize (include/ca3d.h): population, births / deaths against the state one step earlier, the
// bounding box of the live cells, the per-plane populations and the order-independent digest — ONE pass over the owned planes of
// the current buffer (and of the other ping-pong buffer when it holds the state one step earlier), nothing state-sized written.
//
// Decomposition: a plane is cut into tiles of kThreads * kPer uint4 (16 KiB); the tiles of all planes, in memory order, are dealt
// out in CONTIGUOUS runs to a bounded number of workgroups (a few per CU), so that a workgroup mostly stays inside one plane and
// the plane count costs one workgroup reduction per plane change instead of one per tile. Every lane issues its kPer 16-byte
// loads of both buffers before the first use. Rows need not be whole uint4 (G = 96, 160, 288 ...: 3, 5, 9 words): the row / word
// column of a lane's first word come from one division per uint4 (a shift on power-of-two rows), the other three by carry.
// Reduction: registers -> wave (__shfl_xor) -> workgroup (LDS) -> one set of integer atomics per workgroup. Integer sums, minima
// and maxima are exact and independent of the order workgroups finish in: two runs give the same numbers, the digest included.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
#include "ca_bitops.inc"
#include "ca_wave_ops.inc"

typedef unsigned long long u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4; // uint4 per lane and tile, per buffer
constexpr u32 kTileVecs = kThreads * kPer;

struct SummaryArgs
{
	const u32x4 *cur, *prev; // first owned plane of the current buffer / of the buffer holding the state one step earlier
	u32 *result;             // kSummaryHeaderWords + nz words, zeroed
	u64 base_word;           // index of the first owned word in the FULL grid's state array (z0 * words per plane)
	u32 plane_vecs;          // uint4 per plane
	u32 cols;                // words per row
	int cols_shift;          // log2(cols) when cols is a power of two, else -1
	u32 chunks;              // tiles per plane
	u32 tiles;               // nz * chunks
	u32 z0;
};

#include "ca_digest.h"

// the workgroup's live cells of plane `plane` -> its slot (called by all threads, at a workgroup-uniform point)
__device__ __forceinline__ void flush_plane(u32 *result, u32 plane, u32 count, u32 *lds)
{
	const u32 s = wave_add(count);
	if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0u)
	{
		u32 t = 0;
		for (int w = 0; w < kWaves; w++) t += lds[w];
		if (t) atomicAdd(result + kSummaryHeaderWords + plane, t);
	}
	__syncthreads();
}

template <bool PACKED, bool PREV>
__global__ __launch_bounds__(kThreads) void ca_summary(SummaryArgs a)
{
	__shared__ u32 lds_plane[kWaves];
	__shared__ u64 lds64[kWaves][4];
	__shared__ u32 lds32[kWaves][6];
	const u32 tid = threadIdx.x;
	const u32 t0 = (u32)((u64)a.tiles * blockIdx.x / gridDim.x), t1 = (u32)((u64)a.tiles * (blockIdx.x + 1u) / gridDim.x);
	u32 pop = 0, births = 0, deaths = 0;
	u64 dig = 0;
	u32 xmin = 0xFFFFFFFFu, ymin = 0xFFFFFFFFu, zmin = 0xFFFFFFFFu, xmax = 0, ymax = 0, zmax = 0; // z: plane of the slab
	u32 plane = t0 < t1 ? t0 / a.chunks : 0u, plane_pop = 0;
	for (u32 t = t0; t < t1; t++)
	{
		const u32 z = t / a.chunks, c = t - z * a.chunks;
		if (z != plane) // workgroup-uniform
		{
			flush_plane(a.result, plane, plane_pop, lds_plane);
			plane = z;
			plane_pop = 0;
		}
		const u32 pv0 = c * kTileVecs + tid;
		const size_t vbase = (size_t)z * a.plane_vecs;
		u32x4 v[kPer], p[kPer];
#pragma unroll
		for (int k = 0; k < kPer; k++)
		{
			const u32 pv = pv0 + (u32)k * kThreads;
			const bool in = pv < a.plane_vecs;
			v[k] = in ? a.cur[vbase + pv] : (u32x4){0u, 0u, 0u, 0u};
			if (PREV) p[k] = in ? a.prev[vbase + pv] : (u32x4){0u, 0u, 0u, 0u};
		}
		const u32 pop_before = pop;
#pragma unroll
		for (int k = 0; k < kPer; k++)
		{
			// (a uint4 beyond the plane was read as zeros: zero words contribute to nothing)
			const u32 pv = pv0 + (u32)k * kThreads;
			const u32 wl = pv * 4u; // word index inside the plane
			u32 y, xc;
			if (a.cols_shift >= 0) { y = wl >> a.cols_shift; xc = wl & (a.cols - 1u); }
			else { y = wl / a.cols; xc = wl - y * a.cols; }
			const u64 gi = a.base_word + (u64)(vbase + pv) * 4u;
#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				const u32 w = v[k][j];
				if (w) dig += digest_mix(gi + (u64)j, w);
				if (PACKED)
				{
					pop += (u32)__popc(w);
					if (PREV)
					{
						const u32 q = p[k][j];
						births += (u32)__popc(w & ~q);
						deaths += (u32)__popc(q & ~w);
					}
					if (w)
					{
						xmin = min(xmin, xc * 32u + (u32)__builtin_ctz(w));
						xmax = max(xmax, xc * 32u + 31u - (u32)__builtin_clz(w));
						ymin = min(ymin, y);
						ymax = max(ymax, y);
					}
				}
				else
				{
					// a cell is alive exactly when its word == 1 (ca_unpacked.hip, ca_unpacked_literal: `st == 1u`; render_device.inc: `== 1u`)
					const u32 alive = w == 1u ? 1u : 0u;
					pop += alive;
					if (PREV)
					{
						const u32 was = p[k][j] == 1u ? 1u : 0u;
						births += alive & (was ^ 1u);
						deaths += was & (alive ^ 1u);
					}
					if (alive)
					{
						xmin = min(xmin, xc);
						xmax = max(xmax, xc);
						ymin = min(ymin, y);
						ymax = max(ymax, y);
					}
				}
				if (++xc == a.cols) { xc = 0; y++; }
			}
		}
		if (pop != pop_before)
		{
			zmin = min(zmin, z);
			zmax = max(zmax, z);
			plane_pop += pop - pop_before;
		}
	}
	if (t0 < t1) flush_plane(a.result, plane, plane_pop, lds_plane);

	// registers -> wave -> workgroup -> one set of atomics (the counts are widened first: every sum from here on is a 64-bit one)
	const u64 s_pop = wave_add((u64)pop), s_b = wave_add((u64)births), s_d = wave_add((u64)deaths), s_dig = wave_add(dig);
	const u32 m[6] = {wave_min(xmin), wave_min(ymin), wave_min(zmin), wave_max(xmax), wave_max(ymax), wave_max(zmax)};
	const u32 wave = tid >> 6;
	if ((tid & 63u) == 0u)
	{
		lds64[wave][0] = s_pop; lds64[wave][1] = s_b; lds64[wave][2] = s_d; lds64[wave][3] = s_dig;
		for (int i = 0; i < 6; i++) lds32[wave][i] = m[i];
	}
	__syncthreads();
	if (tid == 0u)
	{
		u64 r64[4] = {0, 0, 0, 0};
		u32 lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
		for (int w = 0; w < kWaves; w++)
		{
			for (int i = 0; i < 4; i++) r64[i] += lds64[w][i];
			for (int i = 0; i < 3; i++) { lo[i] = min(lo[i], lds32[w][i]); hi[i] = max(hi[i], lds32[w][3 + i]); }
		}
		u64 *res64 = (u64 *)a.result;
		if (r64[0]) atomicAdd(res64 + 0, r64[0]);
		if (r64[1]) atomicAdd(res64 + 1, r64[1]);
		if (r64[2]) atomicAdd(res64 + 2, r64[2]);
		if (r64[3]) atomicAdd(res64 + 3, r64[3]);
		if (r64[0])
		{
			// minima are kept as the maximum of the complement: the block starts out as zeros, one memset clears all of it
			atomicMax(a.result + 8, ~lo[0]);
			atomicMax(a.result + 9, ~lo[1]);
			atomicMax(a.result + 10, ~(lo[2] + a.z0));
			atomicMax(a.result + 11, hi[0]);
			atomicMax(a.result + 12, hi[1]);
			atomicMax(a.result + 13, hi[2] + a.z0);
		}
	}
}

// ca3d_step_until_cycle's comparison of the state with the anchor: 16-byte loads over both arrays, every lane its kPer of both before the
// first use; a workgroup that saw a difference ORs 1 into the flag word (one atomic per workgroup at most)
__global__ __launch_bounds__(kThreads) void ca_state_equal(const u32x4 *a, const u32x4 *b, u64 n_vecs, u32 *flag)
{
	__shared__ u32 lds[kWaves];
	u32 diff = 0;
	for (u64 base = (u64)blockIdx.x * kTileVecs; base < n_vecs; base += (u64)gridDim.x * kTileVecs)
	{
		u32x4 x[kPer], y[kPer];
#pragma unroll
		for (int k = 0; k < kPer; k++)
		{
			const u64 i = base + threadIdx.x + (u64)k * kThreads;
			const bool in = i < n_vecs;
			x[k] = in ? a[i] : (u32x4){0u, 0u, 0u, 0u};
			y[k] = in ? b[i] : (u32x4){0u, 0u, 0u, 0u};
		}
#pragma unroll
		for (int k = 0; k < kPer; k++)
		{
			const u32x4 d = x[k] ^ y[k];
			diff |= d[0] | d[1] | d[2] | d[3];
		}
	}
	const u32 any = __ballot(diff != 0u) ? 1u : 0u;
	if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = any;
	__syncthreads();
	if (threadIdx.x == 0u)
	{
		u32 t = 0;
		for (int w = 0; w < kWaves; w++) t |= lds[w];
		if (t) atomicOr(flag, 1u);
	}
}

} // namespace

hipError_t launch_state_equal(const uint32_t *a, const uint32_t *b, size_t n_words, uint32_t *flag, hipStream_t stream)
{
	if (!a || !b || !flag || n_words == 0 || n_words % 4u) return hipErrorInvalidValue;
	const u64 n_vecs = n_words / 4u, tiles = (n_vecs + kTileVecs - 1u) / kTileVecs;
	int dev = 0, cus = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	if (e != hipSuccess) return e;
	const u64 cap = (u64)(cus > 0 ? cus : 256) * 8u;
	hipLaunchKernelGGL(ca_state_equal, dim3((u32)(tiles < cap ? tiles : cap)), dim3(kThreads), 0, stream, (const u32x4 *)a, (const u32x4 *)b, n_vecs, flag);
	return hipGetLastError();
}

hipError_t launch_summary(const SummaryLaunch &l, hipStream_t stream)
{
	SummaryArgs a;
	const bool packed = l.layout == CA3D_LAYOUT_PACKED32;
	a.cols = packed ? l.G / 32u : l.G;
	const size_t plane_words = (size_t)a.cols * l.G; // a multiple of 16 in both layouts
	a.cur = (const u32x4 *)l.cur;
	a.prev = (const u32x4 *)l.prev;
	a.result = l.result;
	a.base_word = (u64)l.z0 * plane_words;
	a.plane_vecs = (u32)(plane_words / 4u);
	a.cols_shift = -1;
	if ((a.cols & (a.cols - 1u)) == 0u)
		for (a.cols_shift = 0; (1u << a.cols_shift) < a.cols;) a.cols_shift++;
	a.chunks = (a.plane_vecs + kTileVecs - 1u) / kTileVecs;
	a.tiles = l.nz * a.chunks;
	a.z0 = l.z0;
	if (a.tiles == 0) return hipErrorInvalidValue;
	int dev = 0, cus = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	if (e != hipSuccess) return e;
	const u32 cap = (u32)(cus > 0 ? cus : 256) * 4u; // four 256-thread workgroups per CU
	const u32 blocks = a.tiles < cap ? a.tiles : cap;
	if (packed)
	{
		if (l.prev) hipLaunchKernelGGL((ca_summary<true, true>), dim3(blocks), dim3(kThreads), 0, stream, a);
		else hipLaunchKernelGGL((ca_summary<true, false>), dim3(blocks), dim3(kThreads), 0, stream, a);
	}
	else
	{
		if (l.prev) hipLaunchKernelGGL((ca_summary<false, true>), dim3(blocks), dim3(kThreads), 0, stream, a);
		else hipLaunchKernelGGL((ca_summary<false, false>), dim3(blocks), dim3(kThreads), 0, stream, a);
	}
	return hipGetLastError();
}

} // namespace ca3d
