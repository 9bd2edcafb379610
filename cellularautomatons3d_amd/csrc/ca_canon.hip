// Canon kernel behind ca3d_ensemble_canon (include/ca3d.h): a universe's name up to the 48 symmetries of the cube and any translation.
// For every orientation o the state is turned by o with the turned box's minimum at the origin — T_o, compose with at = 0 — and T_o's
// ca3d_summary digest is formed; the key is the smallest digest, the orientation the first o that reaches it, and bit o of the symmetry
// mask says that T_o equals T_0 word for word. ONE workgroup a universe, every universe of a call in one launch. The kernel only reads
// the states.
//
// Layout, load_universe, extent and the invariants they keep (every barrier reached by all 1024 threads, every loop bound
// workgroup-uniform, no waits on other workgroups, no atomics, nothing but vector stores) are ca_flood.inc's; nothing is flooded here.
// The universe goes into LDS as the turn image (ca_turn_image.inc: two planes of words, [word][z][y] with 65 words a plane of rows), its
// population and box come from extent, whose barrier is also the image's. From there on the image is only read: the loop over the 48
// orientations holds NO barrier. In it every thread assembles ITS four rows of T_o under compose's map with at = 0, adds digest_mix of
// the non-zero words to a sum that the wave joins into dig[o][wave], and compares the rows with its rows of T_0, kept in registers
// from o = 0; the wave's ballot of "a row differs" sets bit o of a scalar mask. In the loop wave w owns planes w, w + 16, w + 32 and
// w + 48 of T_o — not load_universe's 4 w .. 4 w + 3: the rows come out of the image, and a thin object is spread over the SIMDs that
// way. A plane above the turned box has nothing to assemble: its row of T_o is zero. One barrier behind the loop, then threads 0 .. 47
// sum the 16 partials of their o, wave 0 takes the 64-bit minimum and thread 0 writes the record.
//
// THE LOOP OVER THE ORIENTATIONS is ca_canon_pass.inc, a fragment included below where its text stood (its head has the contract;
// DESIGN.md 12.10): ca_canon_period.hip (canon over a period) includes the same text inside its loop over the phases.
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
#include "ca_turn_image.inc"

struct CanonArgs
{
	const u32 *state; // [B][8192], the ensemble's current states
	ca3d_canon *out;  // [count]
	u64 *digests;     // [count][48] or null
	u32 first;
};

constexpr u32 kOrientations = 48u;

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

	// ---- the pass over the orientations, no barrier inside: it leaves T0 (the thread's rows of T_0), t0_any and differs
#include "ca_canon_pass.inc"

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
