// Seed kernels behind ca3d_seed_state / ca3d_group_seed_state / ca3d_ensemble_seed_state (include/ca3d.h): the counter-based fill the
// hosts share (host.random_fill / host.seeded_state) produced where the state lives. A word is a pure function of (seed, its index in the
// FULL grid), so every lane computes what it stores and nobody waits for anybody: no LDS, no atomics, no inter-workgroup traffic, and
// nothing is read from memory but the kernel arguments (the ensemble form: one wave-uniform load of the universe's spec).
//   * ONE pass writes BOTH ping-pong buffers (an upload copies host -> buffer 0 -> buffer 1): 16-byte stores, consecutive lanes on
//     consecutive 16 bytes, the same register quad stored twice.
//   * blockIdx.y is the array plane: the z test of the box and the "is this a ghost plane" test are uniform over the workgroup, and a
//     plane outside the box (or a ghost plane of a slab) costs its stores only. The y test and the x mask are per word: a uint4 of a
//     narrow grid (32^3: one word per row) spans four rows.
//   * the hash is 32-bit throughout: the index term i * 0x9E3779B9 is computed once per lane and advanced by ADDITION from word to word,
//     the round term by addition from round to round; a round is two multiplies, three shift-xors and the AND.
//   * stores are plain. Whether grids whose two buffers exceed the Infinity Cache gain from non-temporal stores has NOT been measured
//     (DESIGN.md 13): until it has, there is one store flavour and no knob.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
typedef uint32_t u32;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

constexpr u32 kSeedThreads = 256;
constexpr u32 kGolden = 0x9E3779B9u, kRound = 0x85EBCA6Bu;

__device__ __forceinline__ u32 mix_final(u32 x)
{
	x ^= x >> 16;
	x *= 0x7FEB352Du;
	x ^= x >> 15;
	x *= 0x846CA68Bu;
	x ^= x >> 16;
	return x;
}

// AND over r = 0 .. rounds of mix32(seed, i, r), with t = i * kGolden + seed (modulo 2^32)
__device__ __forceinline__ u32 fill_word(u32 t, u32 rounds)
{
	u32 w = mix_final(t);
	for (u32 r = 0; r < rounds; r++)
	{
		t += kRound;
		w &= mix_final(t);
	}
	return w;
}

struct Box
{
	u32 lo[3], hi[3];
};

// bits of word column xw (cells 32 xw .. 32 xw + 31) whose x lies in [x0, x1]
__device__ __forceinline__ u32 x_mask(u32 xw, u32 x0, u32 x1)
{
	const u32 base = xw << 5;
	const u32 lo = x0 > base ? x0 : base, hi = x1 < base + 31u ? x1 : base + 31u;
	return lo > hi ? 0u : (~0u << (lo & 31u)) & (~0u >> (31u - (hi & 31u)));
}

// Four consecutive words of a PACKED32 plane from word r (a multiple of 4) of global plane gz, which is inside the box in z
__device__ __forceinline__ u32x4 packed_quad(u32 r, u32 gz, u32 G, u32 cols, int cshift, u32 seed, u32 rounds, const Box &b)
{
	u32 y = cshift >= 0 ? r >> cshift : r / cols;
	u32 xw = r - y * cols;
	u32 t = (gz * (cols * G) + r) * kGolden + seed; // the index enters modulo 2^32
	u32x4 out;
#pragma unroll
	for (int k = 0; k < 4; k++)
	{
		const u32 m = (y >= b.lo[1] && y <= b.hi[1]) ? x_mask(xw, b.lo[0], b.hi[0]) : 0u;
		out[k] = fill_word(t, rounds) & m;
		t += kGolden;
		if (++xw == cols) { xw = 0u; y++; }
	}
	return out;
}

__device__ __forceinline__ void store2(u32 *b0, u32 *b1, size_t v4, u32x4 v)
{
	reinterpret_cast<u32x4 *>(b0)[v4] = v;
	reinterpret_cast<u32x4 *>(b1)[v4] = v;
}

struct SeedArgs
{
	u32 *b0, *b1;
	u32 G, cols; // cols: words per row (packed: G / 32; unpacked: words per row of the PACKED form the cells are cut from, ceil(G / 32))
	int cshift;  // packed: log2(cols), or -1 when cols is not a power of two
	u32 plane_v4; // uint4 per plane
	u32 z0, nz, ghost;
	u32 seed, rounds;
	Box box;
};

__global__ __launch_bounds__(kSeedThreads) void ca_seed_packed(SeedArgs a)
{
	const u32 v = blockIdx.x * kSeedThreads + threadIdx.x;
	if (v >= a.plane_v4) return;
	const u32 owned = blockIdx.y - a.ghost; // (wraps on the low ghost planes: >= nz)
	const u32 gz = a.z0 + owned;
	u32x4 out = 0u;
	if (owned < a.nz && gz >= a.box.lo[2] && gz <= a.box.hi[2]) // uniform over the workgroup
		out = packed_quad(v * 4u, gz, a.G, a.cols, a.cshift, a.seed, a.rounds, a.box);
	store2(a.b0, a.b1, (size_t)blockIdx.y * a.plane_v4 + v, out);
}

// One u32 (0 / 1) per cell: a lane owns four x-adjacent cells (G is a multiple of 4: one row, one packed word), hashes that word itself
// and stores its four cells as 16 bytes
__global__ __launch_bounds__(kSeedThreads) void ca_seed_unpacked(SeedArgs a)
{
	const u32 v = blockIdx.x * kSeedThreads + threadIdx.x;
	if (v >= a.plane_v4) return;
	const u32 owned = blockIdx.y - a.ghost;
	const u32 gz = a.z0 + owned;
	u32x4 out = 0u;
	if (owned < a.nz && gz >= a.box.lo[2] && gz <= a.box.hi[2])
	{
		const u32 r = v * 4u, y = r / a.G, x = r - y * a.G;
		if (y >= a.box.lo[1] && y <= a.box.hi[1])
		{
			const u32 i = (x >> 5) + y * a.cols + gz * (a.cols * a.G);
			const u32 w = fill_word(i * kGolden + a.seed, a.rounds) >> (x & 31u);
#pragma unroll
			for (u32 k = 0; k < 4u; k++) out[k] = (x + k >= a.box.lo[0] && x + k <= a.box.hi[0]) ? (w >> k) & 1u : 0u;
		}
	}
	store2(a.b0, a.b1, (size_t)blockIdx.y * a.plane_v4 + v, out);
}

// Ensemble: workgroup k seeds universe first + k — 8192 words, 2048 uint4, eight per lane — into both of its buffers
__global__ __launch_bounds__(kSeedThreads) void ca_seed_ensemble(u32 *state, u32 *prev, u32 first, const ca3d_seed *specs, ca3d_seed one)
{
	const ca3d_seed s = specs ? specs[blockIdx.x] : one; // the address is uniform: one load for the wave
	Box b;
	for (int i = 0; i < 3; i++) { b.lo[i] = s.box_min[i]; b.hi[i] = s.box_max[i]; }
	const size_t base = (size_t)(first + blockIdx.x) * kEnsembleWords;
	for (u32 v = threadIdx.x; v < kEnsembleWords / 4u; v += kSeedThreads)
	{
		const u32 r = v * 4u, z = r >> 7; // 128 words per plane
		u32x4 out = 0u;
		if (z >= b.lo[2] && z <= b.hi[2]) out = packed_quad(r & 127u, z, 64u, 2u, 1, s.seed, s.and_rounds, b);
		store2(state + base, prev + base, v, out);
	}
}

} // namespace

hipError_t launch_seed(const SeedLaunch &l, hipStream_t stream)
{
	const bool packed = l.layout == CA3D_LAYOUT_PACKED32;
	if (!l.buf0 || !l.buf1 || l.G == 0 || l.nz == 0 || (packed ? l.G % 32u : l.G % 4u)) return hipErrorInvalidValue;
	SeedArgs a;
	a.b0 = l.buf0; a.b1 = l.buf1;
	a.G = l.G;
	a.cols = (l.G + 31u) / 32u;
	a.cshift = (a.cols & (a.cols - 1u)) ? -1 : __builtin_ctz(a.cols);
	const size_t plane_words = packed ? (size_t)a.cols * l.G : (size_t)l.G * l.G; // a multiple of 4 in both layouts
	a.plane_v4 = (u32)(plane_words / 4u);
	a.z0 = l.z0; a.nz = l.nz; a.ghost = l.ghost;
	a.seed = l.spec.seed; a.rounds = l.spec.and_rounds;
	for (int i = 0; i < 3; i++) { a.box.lo[i] = l.spec.box_min[i]; a.box.hi[i] = l.spec.box_max[i]; }
	const u32 nplanes = l.nz + 2u * l.ghost;
	const dim3 grid((a.plane_v4 + kSeedThreads - 1u) / kSeedThreads, nplanes);
	if (packed) hipLaunchKernelGGL(ca_seed_packed, grid, dim3(kSeedThreads), 0, stream, a);
	else hipLaunchKernelGGL(ca_seed_unpacked, grid, dim3(kSeedThreads), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_seed_ensemble(uint32_t *state, uint32_t *prev, uint32_t first, uint32_t count, const ca3d_seed *specs, const ca3d_seed &one, hipStream_t stream)
{
	if (!state || !prev || count == 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL(ca_seed_ensemble, dim3(count), dim3(kSeedThreads), 0, stream, state, prev, first, specs, one);
	return hipGetLastError();
}

} // namespace ca3d
