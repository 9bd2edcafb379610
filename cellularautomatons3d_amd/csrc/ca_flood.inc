// The closed-cube flood fill on the ensemble's register layout, and the population-and-extent join that follows it: shared by the
// object-level kernels on a 64^3 universe (ca_census.hip, ca_isolate.hip; DESIGN.md 12.7, 12.8). Device code only; include inside
// namespace ca3d { namespace { ... } }, after ca_bitops.inc and ca_wave_ops.inc.
//
// The universe lies in registers as the ensemble kernels hold it (ca_ensemble.hip): ONE workgroup of 1024 threads a universe, lane = row
// y, wave w = planes 4 w .. 4 w + 3, a row's two words in one thread. A thread holds R[4][2], the cells an object may take, and
// F[4][2], the object being filled. An object is found by F <- R & dilate(F) until nothing changes; the 3 x 3 x 3 dilation is the
// step's neighbour access with ORs in place of the count: v_alignbit along x, wave-wide DPP along y, the double-buffered LDS exchange
// (laid out like VnStep's) along z. ALL SIX FACES ARE CLOSED — not the step's boundary: word 1's right neighbour, row 63's y + 1 and
// plane 63's z + 1 shift in zero where the step wraps.
// flood<true> is the same fill on the torus Z_64^3 (ca_objects_torus.hip; DESIGN.md 12.13): it differs in three operands — word 0's x - 1
// and word 1's x + 1 take the row's other word, the y shifts are wave rotations, and wave 0 / 15 read the planes of wave 15 / 0 — and in
// nothing else; extent serves both, and torus_span reads a cyclic box from its masks.
//
// What every kernel built on this may rely on, and must keep:
//  - all 1024 threads reach every __syncthreads(): flood and extent hold barriers, so a kernel must call them from all 1024 threads,
//    never under a condition that differs within the workgroup;
//  - every condition that ends a loop is read from LDS behind a barrier, so every thread leaves, or none;
//  - an iteration that does not end a flood adds a cell: a flood takes population + 1 iterations at most, population + 2 (that is, 2)
//    from an empty seed, whose iteration 0 changes nothing and whose iteration 1 reads that;
//  - no waits on other workgroups, no spins, no atomics, nothing but vector stores.
// ca_isolate.hip calls everything here. ca_census.hip calls extent, and takes the flood as text, not as a call, because the called form
// measured slower there (its header, DESIGN.md 12.7): the loop is ca_flood_loop.inc, a fragment that is flood's whole body here and is
// included once more in the census kernel.
// The LDS arrays are declared by the kernels (kXchWords, kFlgWords, kPartWords) and passed in: a kernel's LDS stays visible in one place.
#pragma once

typedef unsigned long long u64;

constexpr u32 kThreads = 1024, kWaves = 16, kPT = 4; // threads, waves, planes per wave

// the exchange: [iteration parity][wave][first / last plane][word][row], VnStep's
constexpr u32 kXchWords = 2u * kWaves * 2u * 2u * 64u; // 32 KiB
constexpr u32 kFlgWords = 2u * kWaves;                 // [iteration parity][wave]: the wave changed a cell in the iteration before
constexpr u32 kPartWords = kWaves * 8u; // a wave's population, x-occupancy 0 and 1, y ballot low and high, z bits low and high, unused
__device__ __forceinline__ u32 slot(u32 buf, u32 w, u32 which, u32 h, u32 row) { return (((buf * kWaves + w) * 2u + which) * 2u + h) * 64u + row; }

// R <- the thread's four rows of the universe at `mine` ([8192] words)
__device__ __forceinline__ void load_universe(const u32 *mine, u32 wave, u32 row, u32 (&R)[kPT][2])
{
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const uint2 v = *reinterpret_cast<const uint2 *>(mine + ((size_t)((wave * kPT + p) * 64u + row)) * 2u);
		R[p][0] = v.x; R[p][1] = v.y;
	}
}

// F <- the one bit of `cell` = x + 64 y + 4096 z (the bit order of the packed state), workgroup-uniform
__device__ __forceinline__ void seed_cell(u32 (&F)[kPT][2], u32 cell, u32 wave, u32 row)
{
	const u32 sz = cell >> 12, sy = (cell >> 6) & 63u, sx = cell & 63u;
	const bool own = wave == (sz >> 2) && row == sy;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
#pragma unroll
		for (u32 h = 0; h < 2u; h++) F[p][h] = own && p == (sz & 3u) && h == (sx >> 5) ? 1u << (sx & 31u) : 0u;
}

// F <- the connected part of R that holds F (F a part of R): F <- R & dilate(F) until an iteration changes nothing anywhere. Iteration
// k carries the waves' "changed in iteration k - 1" bits in the exchange buffer of its parity, so the barrier of the exchange is the
// barrier of the test: ONE barrier an iteration. xch and flg are dead on return: the iteration that ends the flood reads none of xch,
// and every wave has passed that iteration's barrier only after all had finished the reads of the one before.
// Torus: every face joins the opposite one (see the head of this file); the closed form is flood(...), the default.
// The body is the fragment ca_flood_loop.inc (its head has the contract): the parameters here are the names it reads.
template <bool Torus = false>
__device__ __forceinline__ void flood(const u32 (&R)[kPT][2], u32 (&F)[kPT][2], u32 *xch, u32 *flg, u32 wave, u32 row)
{
#include "ca_flood_loop.inc"
}

// Population and extent of F, workgroup-uniform: x0 / x1 the OR of every row's word 0 / 1, bit y of ym and bit z of zm set where that
// row / plane holds a cell. Of an empty F all five are zero.
struct Extent
{
	u32 pop, x0, x1;
	u64 ym, zm;
};
// thread -> wave (ballots, butterflies) -> part -> ONE barrier -> every wave joins the 16 partials for itself: lanes 0 .. 15 of every
// row of 16 take one wave's each, four DPP steps leave the row's lanes with the whole, lane 0 is read (the *_moving kernels' join).
// The reads of part follow the barrier in here: the caller rewrites part — by the next call, or by stores of its own — only behind a later barrier.
__device__ __forceinline__ Extent extent(const u32 (&F)[kPT][2], u32 *part, u32 wave, u32 row)
{
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
	const uint4 *pr = reinterpret_cast<const uint4 *>(part) + 2u * (row & 15u);
	const uint4 pa = pr[0], pb = pr[1];
	auto lane0 = [](u32 v) { return (u32)__builtin_amdgcn_readlane((int)v, 0); };
	Extent e;
	e.pop = lane0(row16_sum(pa.x));
	e.x0 = lane0(row16_or(pa.y));
	e.x1 = lane0(row16_or(pa.z));
	e.ym = (u64)lane0(row16_or(pb.x)) << 32 | lane0(row16_or(pa.w));
	e.zm = (u64)lane0(row16_or(pb.z)) << 32 | lane0(row16_or(pb.y));
	return e;
}

// The torus box of one axis from its occupancy mask m (bit c: coordinate c holds a cell; m != 0): the shortest cyclic interval that
// covers the set. A connected component's coordinates form ONE cyclic run, so the start is the one set bit whose predecessor is clear
// and the length the number of set bits; a full ring starts at 0.
struct TorusSpan
{
	u32 lo, e; // start 0 .. 63, length 1 .. 64: the interval is lo .. lo + e - 1 modulo 64
};
__device__ __forceinline__ TorusSpan torus_span(u64 m)
{
	const u64 pred = m << 1 | m >> 63; // rotl64(m, 1): bit c = coordinate c - 1 is occupied
	TorusSpan s;
	s.lo = m == ~0ull ? 0u : (u32)__builtin_ctzll(m & ~pred);
	s.e = (u32)__popcll(m);
	return s;
}
