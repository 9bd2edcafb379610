// Compose kernel behind ca3d_ensemble_compose (include/ca3d.h): a destination universe becomes the union of several pieces, each the
// whole state of a source universe, turned by one of the 48 symmetries of the cube and put where the caller says. ONE workgroup a
// destination, every destination of a call in one launch. The inverse of ca_isolate.hip.
//
// Layout, load_universe, extent and the invariants they keep (every barrier reached by all 1024 threads, every loop bound
// workgroup-uniform, no waits on other workgroups, no atomics, nothing but vector stores) are ca_flood.inc's; nothing is flooded here.
// A[4][2] is the destination being built: zero, or its current state under CA3D_COMPOSE_OVER. For each part — the bounds of that loop
// are read by every thread from part_begin, the same words for all — the source universe R[4][2] goes into LDS as an image, its
// population and box come from extent (whose barrier is also the image's), and every thread assembles ITS four destination rows from
// the image under the part's map and ORs them into A. A second barrier ends the part: the image and `part` are rewritten only behind it.
//
// The map. A destination cell d is live when the piece holds c with c[perm[i]] = s_i d[i] + k_i, s_i = -1 where output
// axis i is mirrored, and d[i] lies in [at[i], at[i] + e[perm[i]] - 1] — the turned box — cut to 0 .. 63. Inside those intervals c lies
// inside the piece's box, so inside the image: no address is formed from a coordinate outside them (rows and planes outside are clamped
// to the interval and their result dropped).
//  - perm[0] == 0, 8 of the 48: a destination row is ONE image row, bit-reversed when x is mirrored, shifted by a scalar.
//  - the other 40: the 64 bits of a destination row lie in 64 image rows. One ds_read_b32 and a bit extract a cell, over the x interval
//    of the turned box only, so a small object costs a few reads a row.
// The image is two planes of words, [word][z][y] with 65 words a plane of rows: lanes that run along the piece's y are 1 word apart,
// lanes that run along its z 65 — both reach 32 different banks; with the natural [z][y][2] they would be 128 words apart, one bank.
// Its constants, the permutation tables and uni, pick and shifted are ca_turn_image.inc's, shared with the canon kernels.
//
// THE MAP AND THE ROW ASSEMBLY BELOW ARE THIS KERNEL'S OWN. The canon kernels' (ca_canon_pass.inc) are the case at = 0, where the
// intervals are [0, e'[i] - 1] and nothing is clipped; here every axis is clipped by `at` (lo and hi, rows and planes clamped into
// them), and the result is ORed into A, not digested. That is another text, not a copy: as functions shared by both kernels the common
// pieces changed this kernel's register allocation and instruction count, so each keeps its own.
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
#include "ca_turn_image.inc"

struct ComposeArgs
{
	const u32 *src_state;            // [Bs][8192], the source ensemble's current states
	u32 *dst_state, *dst_prev;       // [Bd][8192], both buffers of the destination ensemble
	const u32 *src_rules;            // [Bs][rule_words]
	u32 *dst_rules;                  // [Bd][rule_words]
	const ca3d_compose_part *parts;  // [part_begin[n_dst]]
	const u32 *part_begin;           // [n_dst + 1]
	ca3d_composed *out;              // [n_dst]
	u32 dst_first, over, rule_words; // rule_words 0: rules stay
};

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_compose64(ComposeArgs a)
{
	__shared__ __attribute__((aligned(16))) u32 img[kImgWords];
	__shared__ __attribute__((aligned(16))) u32 part[kPartWords];
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)uni((int)(tid >> 6));
	const size_t dst_off = (size_t)(a.dst_first + blockIdx.x) * kEnsembleWords;

	u32 A[kPT][2];
	if (a.over) load_universe(a.dst_state + dst_off, wave, row, A);
	else
	{
#pragma unroll
		for (u32 p = 0; p < kPT; p++) A[p][0] = A[p][1] = 0u;
	}
	u32 base_pop = 0, placed = 0; // the thread's share
#pragma unroll
	for (u32 p = 0; p < kPT; p++) base_pop += (u32)__popc(A[p][0]) + (u32)__popc(A[p][1]);
	u32 pieces_pop = 0; // workgroup-uniform: the populations of the parts, summed

	const u32 begin = (u32)uni((int)a.part_begin[blockIdx.x]), end = (u32)uni((int)a.part_begin[blockIdx.x + 1u]);
	for (u32 i = begin; i < end; i++)
	{
		const ca3d_compose_part *pp = a.parts + i; // the host has checked universe, orientation and at
		const u32 universe = (u32)uni((int)pp->universe), o = (u32)uni((int)pp->orientation);
		const int at[3] = {uni(pp->at[0]), uni(pp->at[1]), uni(pp->at[2])};

		u32 R[kPT][2];
		load_universe(a.src_state + (size_t)universe * kEnsembleWords, wave, row, R);
		// ---- the image (behind the barrier that ended the part before)
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
		{
			const u32 w = (wave * kPT + p) * kImgPlane + row;
			img[w] = R[p][0];
			img[kImgHalf + w] = R[p][1];
		}
		// ---- population and box. The barrier inside extent is also the image's: behind it every thread may read every image row.
		const Extent e = extent(R, part, wave, row);
		pieces_pop += e.pop;

		// ---- the map, workgroup-uniform
		const u32 m = o % 6u, f = o / 6u;
		const u32 pj[3] = {(kPerm0 >> 2u * m) & 3u, (kPerm1 >> 2u * m) & 3u, (kPerm2 >> 2u * m) & 3u};
		int s[3], k[3], lo[3], hi[3];
		bool active = e.pop != 0u; // (an empty piece has no box)
		if (active)
		{
			const u64 xm = (u64)e.x1 << 32 | e.x0;
			const int mn[3] = {(int)__builtin_ctzll(xm), (int)__builtin_ctzll(e.ym), (int)__builtin_ctzll(e.zm)};
			const int mx[3] = {63 - (int)__builtin_clzll(xm), 63 - (int)__builtin_clzll(e.ym), 63 - (int)__builtin_clzll(e.zm)};
#pragma unroll
			for (int d = 0; d < 3; d++)
			{
				const int lo_c = pick(pj[d], mn[0], mn[1], mn[2]), ext = pick(pj[d], mx[0], mx[1], mx[2]) - lo_c + 1;
				const bool flip = (f >> d) & 1u;
				s[d] = flip ? -1 : 1;
				k[d] = lo_c + (flip ? ext - 1 + at[d] : -at[d]);
				lo[d] = max(at[d], 0);
				hi[d] = min(at[d] + ext - 1, 63);
				active = active && lo[d] <= hi[d];
			}
		}
		if (active) // workgroup-uniform, and no barrier inside
		{
			// this thread's row y, clamped into the turned box: the address stays inside the image, the result is dropped below
			const int y = (int)row, yc = min(max(y, lo[1]), hi[1]);
			const int cy_from = s[1] * yc + k[1]; // the piece's coordinate on axis pj[1]
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const int z = (int)(wave * kPT + p), zc = min(max(z, lo[2]), hi[2]);
				const int cz_from = s[2] * zc + k[2]; // the piece's coordinate on axis pj[2]
				const bool inside = y == yc && z == zc;
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
					// the piece's x comes from y or z: one bit of one word plane; its other coordinate, and pj[0]'s, which x walks
					const int cx = pj[1] == 0u ? cy_from : cz_from;
					const int other = pj[1] == 0u ? cz_from * (pj[2] == 1u ? 1 : (int)kImgPlane) : cy_from * (pj[1] == 1u ? 1 : (int)kImgPlane);
					const int step = pj[0] == 1u ? 1 : (int)kImgPlane;
					const u32 bit = (u32)cx & 31u;
					const int w0 = (cx >> 5) * (int)kImgHalf + other + k[0] * step, dw = s[0] * step;
					u32 r0 = 0, r1 = 0;
#pragma unroll 8
					for (int x = lo[0]; x <= min(hi[0], 31); x++) r0 |= ((img[w0 + x * dw] >> bit) & 1u) << x;
#pragma unroll 8
					for (int x = max(lo[0], 32); x <= hi[0]; x++) r1 |= ((img[w0 + x * dw] >> bit) & 1u) << (x - 32);
					r64 = (u64)r1 << 32 | r0;
				}
				if (!inside) r64 = 0;
				placed += (u32)__popcll(r64);
				A[p][0] |= (u32)r64;
				A[p][1] |= (u32)(r64 >> 32);
			}
		}
		__syncthreads(); // every reader of the image and of `part` has passed: the next part may write them
	}

	// ---- the write: both buffers, every destination word once
	u32 pop = 0;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const uint2 v = make_uint2(A[p][0], A[p][1]);
		const size_t w = dst_off + (size_t)((wave * kPT + p) * 64u + row) * 2u; // inside universe dst_first + blockIdx.x of the destination
		*reinterpret_cast<uint2 *>(a.dst_state + w) = v;
		*reinterpret_cast<uint2 *>(a.dst_prev + w) = v;
		pop += (u32)__popc(v.x) + (u32)__popc(v.y);
	}
	// ---- the counters: thread -> wave -> part -> ONE barrier -> thread 0 (part is free: the last reads lie behind the loop's barrier)
	pop = wave_add(pop);
	placed = wave_add(placed);
	base_pop = wave_add(base_pop);
	if (row == 0u) reinterpret_cast<uint4 *>(part)[wave] = make_uint4(pop, placed, base_pop, 0u);
	__syncthreads();
	if (tid == 0u)
	{
		uint4 t = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
		for (u32 w = 0; w < kWaves; w++)
		{
			const uint4 v = reinterpret_cast<const uint4 *>(part)[w];
			t.x += v.x; t.y += v.y; t.z += v.z;
		}
		*reinterpret_cast<uint4 *>(a.out + blockIdx.x) = make_uint4(t.x, t.y, t.z + t.y - t.x, pieces_pop - t.y);
		if (begin < end)
		{
			const u32 *rs = a.src_rules + (size_t)a.parts[begin].universe * a.rule_words;
			u32 *rd = a.dst_rules + (size_t)(a.dst_first + blockIdx.x) * a.rule_words;
#pragma nounroll
			for (u32 i = 0; i < a.rule_words; i++) rd[i] = rs[i];
		}
	}
}

} // namespace

hipError_t launch_compose(const ComposeLaunch &l, hipStream_t stream)
{
	if (l.n_dst == 0 || l.rule_words > 6u) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_composed) == 16 && sizeof(ca3d_compose_part) == 24, "a record is one 16-byte store");
	static_assert(kImgWords * 4u + kPartWords * 4u <= 65536u, "the image and the partials fit 64 KiB of LDS");
	ComposeArgs a;
	a.src_state = l.src_state;
	a.dst_state = l.dst_state;
	a.dst_prev = l.dst_prev;
	a.src_rules = l.src_rules;
	a.dst_rules = l.dst_rules;
	a.parts = l.parts;
	a.part_begin = l.part_begin;
	a.out = l.out;
	a.dst_first = l.dst_first;
	a.over = l.over ? 1u : 0u;
	a.rule_words = l.rule_words;
	hipLaunchKernelGGL(ca_ensemble_compose64, dim3(l.n_dst), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
