// Canon kernel behind ca3d_ensemble_canon (include/ca3d.h): a universe's name up to the 48 symmetries of the cube and any translation.
// For every orientation o the state is turned by o with the turned box's minimum at the origin — T_o, compose with at = 0 — and T_o's
// ca3d_summary digest is formed; the key is the smallest digest, the orientation the first o that reaches it, and bit o of the symmetry
// mask says that T_o equals T_0 word for word. ONE workgroup a universe, every universe of a call in one launch. The kernel only reads
// the states.
//
// Layout, load_universe, extent and the invariants they keep (every barrier reached by all 1024 threads, every loop bound
// workgroup-uniform, no waits on other workgroups, no atomics, nothing but vector stores) are ca_flood.inc's; nothing is flooded here.
// The universe goes into LDS as compose's image (ca_compose.hip: two planes of words, [word][z][y] with 65 words a plane of rows), its
// population and box come from extent, whose barrier is also the image's. From there on the image is only read: the loop over the 48
// orientations holds NO barrier. In it every thread assembles ITS four rows of T_o under compose's map with at = 0, adds digest_mix of
// the non-zero words to a sum that the wave joins into dig[o][wave], and compares the rows with its rows of T_0, kept in registers
// from o = 0; the wave's ballot of "a row differs" sets bit o of a scalar mask. In the loop wave w owns planes w, w + 16, w + 32 and
// w + 48 of T_o — not load_universe's 4 w .. 4 w + 3: the rows come out of the image, and a thin object is spread over the SIMDs that
// way. A plane above the turned box has nothing to assemble: its row of T_o is zero. One barrier behind the loop, then threads 0 .. 47
// sum the 16 partials of their o, wave 0 takes the 64-bit minimum and thread 0 writes the record.
//
// THE MAP AND THE ROW ASSEMBLY ARE ca_compose.hip's (its header), written out here with at = 0, so that the intervals
// are [0, e'[i] - 1] and nothing is clipped: change that text with this one. ca_canon_period.hip (canon over a period)
// carries the image, the orientation loop and the join of THIS file written out inside its loop over the phases: change it with this one.
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

struct CanonArgs
{
	const u32 *state; // [B][8192], the ensemble's current states
	ca3d_canon *out;  // [count]
	u64 *digests;     // [count][48] or null
	u32 first;
};

constexpr u32 kOrientations = 48u;
constexpr u32 kImgPlane = 65u;            // compose's image: words from one plane of rows to the next
constexpr u32 kImgHalf = 64u * kImgPlane; // words of one of the two word planes
constexpr u32 kImgWords = 2u * kImgHalf;  // 33 280 B
constexpr u32 kPerm0 = 0u | 0u << 2 | 1u << 4 | 1u << 6 | 2u << 8 | 2u << 10; // PERMS[m][i], two bits an m
constexpr u32 kPerm1 = 1u | 2u << 2 | 0u << 4 | 2u << 6 | 0u << 8 | 1u << 10;
constexpr u32 kPerm2 = 2u | 1u << 2 | 2u << 4 | 0u << 6 | 1u << 8 | 0u << 10;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int pick(u32 j, int a, int b, int c) { return j == 0u ? a : j == 1u ? b : c; }
// v shifted left by t (right by -t), zero from |t| >= 64 on
__device__ __forceinline__ u64 shifted(u64 v, int t) { return t >= 64 || t <= -64 ? 0ull : t >= 0 ? v << (u32)t : v >> (u32)-t; }

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_canon64(CanonArgs a)
{
	__shared__ __attribute__((aligned(16))) u32 img[kImgWords];
	__shared__ __attribute__((aligned(16))) u32 part[kPartWords];
	__shared__ __attribute__((aligned(16))) u64 dig[kOrientations * kWaves]; // [o][wave]: the wave's share of T_o's digest
	__shared__ __attribute__((aligned(16))) u64 dif[kWaves];                 // [wave]: bit o: one of the wave's rows of T_o differs from T_0's
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)uni((int)(tid >> 6));

	u32 R[kPT][2];
	load_universe(a.state + (size_t)(a.first + blockIdx.x) * kEnsembleWords, wave, row, R);
	// ---- the image
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const u32 w = (wave * kPT + p) * kImgPlane + row;
		img[w] = R[p][0];
		img[kImgHalf + w] = R[p][1];
	}
	// ---- population and box. The barrier inside extent is also the image's: behind it every thread may read every image row, and
	// nothing writes the image again.
	const Extent e = extent(R, part, wave, row);
	int mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}; // an empty universe: a box of one dead cell, every T_o empty
	if (e.pop != 0u)
	{
		const u64 xm = (u64)e.x1 << 32 | e.x0;
		mn[0] = (int)__builtin_ctzll(xm); mn[1] = (int)__builtin_ctzll(e.ym); mn[2] = (int)__builtin_ctzll(e.zm);
		mx[0] = 63 - (int)__builtin_clzll(xm); mx[1] = 63 - (int)__builtin_clzll(e.ym); mx[2] = 63 - (int)__builtin_clzll(e.zm);
	}

	u32 T0[kPT][2]; // the thread's rows of T_0, from o = 0
#pragma unroll
	for (u32 p = 0; p < kPT; p++) T0[p][0] = T0[p][1] = 0u;
	bool t0_any = false; // wave-uniform: the wave holds a cell of T_0
	u64 differs = 0;     // wave-uniform

	// WHICH ROWS OF T_o A THREAD ASSEMBLES is free, since they come out of the image: not planes 4 w .. 4 w + 3, load_universe's, but
	// planes w, w + 16, w + 32, w + 48. An ash object, two or three planes thick, then lies in two or three waves on different SIMDs
	// with ONE plane each, where the other layout would give all of it to wave 0: the launch is bound by that one wave's digest_mix.
	// A wave whose planes lie above the LARGEST extent of the box lies above every turned box: all its rows of every T_o are zero. It
	// writes its 48 zeros at once and leaves the loop to the others (wave-uniform, and no barrier inside either branch).
	const int reach = max(mx[0] - mn[0], max(mx[1] - mn[1], mx[2] - mn[2]));
	if ((int)wave > reach)
	{
		if (row < kOrientations) dig[row * kWaves + wave] = 0ull;
	}
	else
	{
#pragma nounroll
	for (u32 o = 0; o < kOrientations; o++) // compile-time bounds, the same for every thread; no barrier inside
	{
		// ---- the map, workgroup-uniform: compose's with at = 0
		const u32 m = o % 6u, f = o / 6u;
		const u32 pj[3] = {(kPerm0 >> 2u * m) & 3u, (kPerm1 >> 2u * m) & 3u, (kPerm2 >> 2u * m) & 3u};
		int s[3], k[3], hi[3];
#pragma unroll
		for (int d = 0; d < 3; d++)
		{
			const int lo_c = pick(pj[d], mn[0], mn[1], mn[2]), ext = pick(pj[d], mx[0], mx[1], mx[2]) - lo_c + 1;
			const bool flip = (f >> d) & 1u;
			s[d] = flip ? -1 : 1;
			k[d] = lo_c + (flip ? ext - 1 : 0);
			hi[d] = ext - 1; // the turned box is [0, hi] on every axis: inside the cube
		}
		u64 sum = 0;
		bool row_differs;
		if ((int)wave > hi[2]) // wave-uniform: the wave's planes lie above the turned box, its rows of T_o are zero
			row_differs = t0_any;
		else
		{
			u32 ch = 0;
			// this thread's row y, clamped into the turned box: the address stays inside the image, the result is dropped below
			const int y = (int)row, yc = min(y, hi[1]);
			const int cy_from = s[1] * yc + k[1]; // the universe's coordinate on axis pj[1]
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const int z = (int)(p * kWaves + wave);
				if (z > hi[2]) // wave-uniform: this plane lies above the turned box, its row of T_o is zero (and so is T_0's at o = 0)
				{
					ch |= T0[p][0] | T0[p][1];
					continue;
				}
				const int cz_from = s[2] * z + k[2]; // the universe's coordinate on axis pj[2]
				const bool inside = y == yc;
				u64 r64;
				if (pj[0] == 0u)
				{
					// pj[1], pj[2] are 1 and 2 in some order: an image row
					const u32 w = (u32)(pj[1] == 1u ? cz_from * (int)kImgPlane + cy_from : cy_from * (int)kImgPlane + cz_from);
					u64 v = (u64)img[kImgHalf + w] << 32 | img[w];
					// mirrored: bit x of the row is bit k0 - x of the image row, bit 63 - k0 + x of the reversed one
					if (s[0] < 0) v = (u64)__brev((u32)v) << 32 | __brev((u32)(v >> 32));
					r64 = shifted(v, s[0] < 0 ? k[0] - 63 : -k[0]);
				}
				else
				{
					// the universe's x comes from y or z: one bit of one word plane; its other coordinate, and pj[0]'s, which x walks
					const int cx = pj[1] == 0u ? cy_from : cz_from;
					const int other = pj[1] == 0u ? cz_from * (pj[2] == 1u ? 1 : (int)kImgPlane) : cy_from * (pj[1] == 1u ? 1 : (int)kImgPlane);
					const int step = pj[0] == 1u ? 1 : (int)kImgPlane;
					const u32 bit = (u32)cx & 31u;
					const int w0 = (cx >> 5) * (int)kImgHalf + other + k[0] * step, dw = s[0] * step;
					u32 r0 = 0, r1 = 0;
#pragma unroll 8
					for (int x = 0; x <= min(hi[0], 31); x++) r0 |= ((img[w0 + x * dw] >> bit) & 1u) << x;
#pragma unroll 8
					for (int x = 32; x <= hi[0]; x++) r1 |= ((img[w0 + x * dw] >> bit) & 1u) << (x - 32);
					r64 = (u64)r1 << 32 | r0;
				}
				if (!inside) r64 = 0;
				const u32 w0r = (u32)r64, w1r = (u32)(r64 >> 32);
				const u64 index = (u64)(((u32)z * 64u + row) * 2u); // the word's index in the packed state
				if (w0r) sum += digest_mix(index, w0r);
				if (w1r) sum += digest_mix(index + 1u, w1r);
				if (o == 0u) { T0[p][0] = w0r; T0[p][1] = w1r; }
				ch |= (w0r ^ T0[p][0]) | (w1r ^ T0[p][1]);
			}
			if (o == 0u) t0_any = __ballot((T0[0][0] | T0[0][1] | T0[1][0] | T0[1][1] | T0[2][0] | T0[2][1] | T0[3][0] | T0[3][1]) != 0u) != 0ull;
			row_differs = __ballot(ch != 0u) != 0ull;
			// the wave's sum, in lane 0: rows above the turned box hold zero, so the butterfly's steps across more than hi[1] lanes would
			// add nothing there (a wave-uniform bound: an ash object takes two or three of the six steps)
#pragma unroll
			for (int off = 32; off > 0; off >>= 1)
				if (off <= hi[1]) sum += __shfl_xor(sum, off);
		}
		if (row == 0u) dig[o * kWaves + wave] = sum;
		if (row_differs) differs |= 1ull << o;
	}
	}

	// ---- the join: wave -> dig, dif -> ONE barrier -> threads 0 .. 47 -> wave 0 -> thread 0
	if (row == 0u) dif[wave] = differs;
	__syncthreads();
	if (wave == 0u) // wave-uniform, and no barrier inside
	{
		const bool valid = tid < kOrientations;
		u64 d = 0;
		if (valid)
		{
#pragma unroll
			for (u32 w = 0; w < kWaves; w++) d += dig[tid * kWaves + w];
			if (a.digests) a.digests[(size_t)blockIdx.x * kOrientations + tid] = d;
		}
		// the smallest digest as an unsigned 64-bit number, and the smallest o that holds it: high words, then the low words of the
		// lanes that hold that high word, then o
		const u32 dh = (u32)(d >> 32), dl = (u32)d;
		const u32 mh = wave_min(valid ? dh : 0xFFFFFFFFu);
		const u32 ml = wave_min(valid && dh == mh ? dl : 0xFFFFFFFFu);
		const u32 mo = wave_min(valid && dh == mh && dl == ml ? tid : 0xFFFFFFFFu);
		if (tid == 0u)
		{
			u64 any = 0;
#pragma unroll
			for (u32 w = 0; w < kWaves; w++) any |= dif[w];
			const u64 sym = ~any & ((1ull << kOrientations) - 1ull);
			uint4 *rec = reinterpret_cast<uint4 *>(a.out + blockIdx.x);
			rec[0] = make_uint4(ml, mh, (u32)sym, (u32)(sym >> 32));
			rec[1] = make_uint4(mo, e.pop, (u32)(mn[0] | mn[1] << 8 | mn[2] << 16), (u32)(mx[0] | mx[1] << 8 | mx[2] << 16));
		}
	}
}

} // namespace

hipError_t launch_canon(const CanonLaunch &l, hipStream_t stream)
{
	if (l.count == 0) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_canon) == 32, "a record is two 16-byte stores");
	static_assert(kImgWords * 4u + kPartWords * 4u + kOrientations * kWaves * 8u + kWaves * 8u <= 65536u, "the image, the digests and the partials fit 64 KiB of LDS");
	CanonArgs a;
	a.state = l.state;
	a.out = l.out;
	a.digests = reinterpret_cast<u64 *>(l.digests);
	a.first = l.first;
	hipLaunchKernelGGL(ca_ensemble_canon64, dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
