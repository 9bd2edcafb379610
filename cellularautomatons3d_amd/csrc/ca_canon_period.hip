// Canon-over-a-period kernels behind ca3d_ensemble_canon_period (include/ca3d.h): a universe's name up to the 48 symmetries of the cube
// and any translation, taken over the phases t = 0 .. period - 1 of its own evolution, with the proof that the period closes — in ONE
// launch that only reads the ensemble. ONE workgroup a universe; three kernels, one per ensemble kind, share the body
// canon_period_run<Step> and differ in the step policy (ca_ensemble_step.inc: VnStep, MooreStep, ClusteredStep).
//
// The universe is loaded once into the ensemble's register layout (ca_flood.inc's load_universe) and never stored. Round t of the loop,
// t = 0 .. period - 1, a workgroup-uniform bound read once:
//   1. the state S_t goes from the registers into LDS as the turn image (ca_turn_image.inc), as in ca_canon.hip;
//   2. extent gives its population and box; its barrier (B1) is also the image's;
//   3. the pass over the 48 orientations (ca_canon_pass.inc), no barrier inside, then the join behind ONE barrier (B2): wave 0 forms k_t's key,
//      orientation and symmetry, stores keys[u][t] and keeps the running minimum — a strict <, so the first t wins;
//   4. t == 0: the thread's rows of T_0(S_0) are kept (in LDS, a slot of its own for every thread), and the box minimum;
//   5. the thread reads its own eight words back out of the image (it wrote them itself in 1), loads the rule's leaves (Step::load on
//      one to six wave-uniform words, again in every round, so that no leaf is alive across the orientation pass) and takes one
//      Step::step, whose barrier is B3.
// Behind the loop S_period is laid out as in 1 and 2; the thread's rows of T_0(S_period) alone are assembled and compared with the kept
// ones; the waves' ballots meet behind one barrier, thread 0 forms CLOSED and the shift and writes the record.
//
// REGISTERS. The orientation pass takes about 68 vector and 93 scalar registers, the Moore and the clustered step all 128 vector
// registers with their leaves. So nothing but the state's eight words, t and the period lives from one round to the next: the running
// minimum and the kept rows lie in LDS, the kernel's arguments are read where they are used, and row and wave are worked out again
// (whoami) so that no address derived from them is carried along.
//
// LDS. A step policy's exchange is double-buffered for a loop of ONE barrier a step. Here a step is separated from the next by B1 and
// B2, so ONE parity (half of Step::kXchWords, buffer 0 always) suffices: the last read of the exchange follows B3 of round t, its next
// write follows B1 and B2 of round t + 1, which no wave passes before every wave has finished those reads. The image is an array of
// its own, not aliased: its last read in round t lies in front of B2 (the orientation pass) or, for the thread's own words, in front
// of B3; its next write follows B3. part is written in front of B1 and read behind it, and written again behind B2 and B3; dig and dif
// are written in front of B2, read behind it by wave 0, and written again behind B3 and B1. best is wave 0's alone, a word of kept
// one thread's alone. Moore: 65 536 (exchange) + 40 064 (canon's arrays) + 32 768 (kept) + 48 = 138 416 B of the 163 840 a workgroup
// may hold; von Neumann and clustered: 89 264 B.
//
// Layout, load_universe, extent and the invariants (every barrier reached by all 1024 threads, every loop bound a constant or uniform
// over the workgroup or the wave, no waits on other workgroups, no spins, no atomics, nothing but vector stores) are ca_flood.inc's.
//
// THE ORIENTATION PASS is ca_canon.hip's, the same text: ca_canon_pass.inc, a fragment included here inside the loop over the phases
// (its head has the contract). The join behind it is this file's own: it keeps a running minimum where ca_canon.hip
// writes a record.
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
#include "ca_ensemble_step.inc"
#include "ca_turn_image.inc"

struct CanonPeriodArgs
{
	const u32 *state;   // [B][8192], the ensemble's current states
	const u32 *rules;   // [B][rule words of the kind]
	const u32 *periods; // [count]
	ca3d_canon_period *out; // [count]
	u64 *keys;          // [count][keys_stride] or null
	u32 keys_stride;
	u32 first;
};

constexpr u32 kOrientations = 48u;
// static LDS of a kernel beside its exchange: the image, the partials, the digests' shares, the waves' masks
constexpr u32 kCanonBytes = kImgWords * 4u + kPartWords * 4u + kOrientations * kWaves * 8u + kWaves * 8u;

template <typename Step>
__device__ __forceinline__ void canon_period_run(const CanonPeriodArgs &a)
{
	__shared__ __attribute__((aligned(16))) u32 xch[Step::kXchWords / 2u]; // ONE parity of the step's exchange (the header)
	__shared__ __attribute__((aligned(16))) u32 img[kImgWords];
	__shared__ __attribute__((aligned(16))) u32 part[kPartWords];
	__shared__ __attribute__((aligned(16))) u64 dig[kOrientations * kWaves]; // [o][wave]: the wave's share of T_o's digest
	__shared__ __attribute__((aligned(16))) u64 dif[kWaves];                 // [wave]: bit o: one of the wave's rows of T_o differs from T_0's
	// wave 0's running minimum — key low and high, symmetry low and high, orientation, phase, population, unused: the record's first
	// seven words — and behind it S_0's packed box minimum and population. Written by lane 0 of wave 0 and read by wave 0 itself (LDS
	// order within a wave, no barrier): in LDS, because the Moore and the clustered step have no registers to spare across the rounds
	__shared__ __attribute__((aligned(16))) u32 best[12];
	// [word][thread]: the thread's rows of T_0(S_0) — planes wave, wave + 16, wave + 32, wave + 48 —, written in round 0 and read behind
	// the loop by the thread itself: in LDS for the same reason
	__shared__ __attribute__((aligned(16))) u32 kept[2u * kPT * kThreads];

	u32 R[kPT][2];
	load_universe(a.state + (size_t)(a.first + blockIdx.x) * kEnsembleWords, (u32)uni((int)(threadIdx.x >> 6)), threadIdx.x & 63u, R);
	const u32 period = (u32)uni((int)a.periods[blockIdx.x]); // workgroup-uniform, read once

	// What only the join, the step or the end needs is read from the kernel's arguments there and then, not held in scalar registers
	// across the orientation pass, which has none to spare (ca_ensemble.hip's ka)
	const volatile CanonPeriodArgs *ka = (const volatile CanonPeriodArgs *)__builtin_amdgcn_kernarg_segment_ptr();
	// The thread's row and wave are worked out again in every round, once more in front of the step and behind the loop: nothing derived
	// from them — image addresses, digest indices, exchange slots — may stay in registers from one round to the next, or across the
	// orientation pass (ca_ensemble.hip's own())
	auto whoami = [](u32 &row, u32 &wave) __attribute__((always_inline)) {
		u32 v = threadIdx.x;
		asm volatile("" : "+v"(v));
		wave = (u32)uni((int)(v >> 6));
		row = v & 63u;
	};
	// The state in R goes into LDS as the image; its population and box. The barrier inside extent (B1) is also the image's: behind it
	// every thread may read every image row, and nothing writes the image again before the step's barrier.
	auto lay_out = [&](u32 row, u32 wave, int (&mn)[3], int (&mx)[3]) __attribute__((always_inline)) -> u32 {
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
		{
			const u32 w = (wave * kPT + p) * kImgPlane + row;
			img[w] = R[p][0];
			img[kImgHalf + w] = R[p][1];
		}
		const Extent e = extent(R, part, wave, row);
#pragma unroll
		for (int i = 0; i < 3; i++) mn[i] = mx[i] = 0; // an empty universe: a box of one dead cell, every T_o empty
		if (e.pop != 0u)
		{
			const u64 xm = (u64)e.x1 << 32 | e.x0;
			mn[0] = (int)__builtin_ctzll(xm); mn[1] = (int)__builtin_ctzll(e.ym); mn[2] = (int)__builtin_ctzll(e.zm);
			mx[0] = 63 - (int)__builtin_clzll(xm); mx[1] = 63 - (int)__builtin_clzll(e.ym); mx[2] = 63 - (int)__builtin_clzll(e.zm);
		}
		return e.pop;
	};

#pragma nounroll
	for (u32 t = 0; t < period; t++) // a workgroup-uniform bound
	{
		u32 row, wave;
		whoami(row, wave);
		int mn[3], mx[3];
		const u32 pop = lay_out(row, wave, mn, mx);

		// ---- the pass over the orientations of S_t, no barrier inside: it leaves T0 (the thread's rows of T_0(S_t)) and differs
#include "ca_canon_pass.inc"

		// ---- t == 0: what CLOSED and the shift are measured against
		if (t == 0u)
		{
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				kept[(2u * p) * kThreads + wave * 64u + row] = T0[p][0];
				kept[(2u * p + 1u) * kThreads + wave * 64u + row] = T0[p][1];
			}
		}

		// ---- the join of phase t: wave -> dig, dif -> ONE barrier (B2) -> threads 0 .. 47 -> wave 0
		if (row == 0u) dif[wave] = differs;
		__syncthreads();
		if (wave == 0u) // wave-uniform, and no barrier inside
		{
			const u32 tid = row; // wave 0
			const bool valid = tid < kOrientations;
			u64 d = 0;
			if (valid)
			{
#pragma unroll
				for (u32 w = 0; w < kWaves; w++) d += dig[tid * kWaves + w];
			}
			// the smallest digest as an unsigned 64-bit number, and the smallest o that holds it: high words, then the low words of the
			// lanes that hold that high word, then o
			const u32 dh = (u32)(d >> 32), dl = (u32)d;
			const u32 mh = (u32)uni((int)wave_min(valid ? dh : 0xFFFFFFFFu));
			const u32 ml = (u32)uni((int)wave_min(valid && dh == mh ? dl : 0xFFFFFFFFu));
			const u32 mo = (u32)uni((int)wave_min(valid && dh == mh && dl == ml ? tid : 0xFFFFFFFFu));
			if (ka->keys && tid == 0u) ka->keys[(size_t)blockIdx.x * ka->keys_stride + t] = (u64)mh << 32 | ml; // t < period <= keys_stride
			const u32 best_lo = best[0], best_hi = best[1]; // every lane reads the same words (t == 0: not looked at)
			if (tid == 0u && (t == 0u || mh < best_hi || (mh == best_hi && ml < best_lo))) // strictly smaller: the first t that reaches the key keeps it
			{
				u64 any = 0;
#pragma unroll
				for (u32 w = 0; w < kWaves; w++) any |= dif[w];
				const u64 sym = ~any & ((1ull << kOrientations) - 1ull);
				*reinterpret_cast<uint4 *>(best) = make_uint4(ml, mh, (u32)sym, (u32)(sym >> 32));
				*reinterpret_cast<uint4 *>(best + 4) = make_uint4(mo, t, pop, 0u);
				if (t == 0u) *reinterpret_cast<uint2 *>(best + 8) = make_uint2((u32)(mn[0] | mn[1] << 8 | mn[2] << 16), pop);
			}
		}

		// ---- one step. The thread's own eight words come back out of the image, where it put them itself at the top of the round:
		// nothing of the state is alive across the orientation pass. Buffer 0 of the exchange always (the header).
		{
			u32 row, wave;
			whoami(row, wave);
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const u32 w = (wave * kPT + p) * kImgPlane + row;
				R[p][0] = img[w];
				R[p][1] = img[kImgHalf + w];
			}
			// the rule's words, loaded in this round (not in front of the loop, with the expanded leaves held across the rounds) and made
			// wave-uniform again: Step::load expands them into scalar and vector leaves
			const u32 *mine = const_cast<const u32 *>(ka->rules) + (size_t)(ka->first + blockIdx.x) * Step::kRuleWords;
			u32 words[Step::kRuleWords];
#pragma unroll
			for (u32 i = 0; i < Step::kRuleWords; i++) words[i] = (u32)uni((int)mine[i]);
			Step st;
			st.load(words, 0u);
			u32 N[kPT][2];
			st.step(R, N, xch, 0u, wave, row); // its barrier is B3
#pragma unroll
			for (u32 p = 0; p < kPT; p++) { R[p][0] = N[p][0]; R[p][1] = N[p][1]; }
		}
	}

	// ---- S_period: T_0 alone, against the kept rows — an image row moved to the origin, zero outside the box
	u32 row, wave;
	whoami(row, wave);
	int mn[3], mx[3];
	(void)lay_out(row, wave, mn, mx);
	u32 ch = 0;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const int z = (int)(p * kWaves + wave), y = (int)row;
		u64 r64 = 0;
		if (z <= mx[2] - mn[2] && y <= mx[1] - mn[1]) // the address stays inside the image: z + mn[2] <= mx[2], y + mn[1] <= mx[1]
		{
			const u32 w = (u32)((z + mn[2]) * (int)kImgPlane + y + mn[1]);
			r64 = ((u64)img[kImgHalf + w] << 32 | img[w]) >> (u32)mn[0];
		}
		ch |= ((u32)r64 ^ kept[(2u * p) * kThreads + wave * 64u + row]) | ((u32)(r64 >> 32) ^ kept[(2u * p + 1u) * kThreads + wave * 64u + row]);
	}
	const bool wave_differs = __ballot(ch != 0u) != 0ull; // every lane votes
	// (dif was read last behind B2 of the last round; B3 and B1 lie in between)
	if (row == 0u) dif[wave] = wave_differs ? 1ull : 0ull;
	__syncthreads();
	if (wave == 0u && row == 0u) // thread 0, which wrote `best` itself
	{
		u64 any = 0;
#pragma unroll
		for (u32 w = 0; w < kWaves; w++) any |= dif[w];
		const uint4 b0 = *reinterpret_cast<const uint4 *>(best), b1 = *reinterpret_cast<const uint4 *>(best + 4);
		const u32 first_min = best[8], first_pop = best[9];
		u32 fs = 0;
		if (any == 0ull)
		{
			fs = CA3D_CANON_CLOSED;
			if (first_pop != 0u) // S_0 is not empty (then S_period is not either)
			{
#pragma unroll
				for (u32 i = 0; i < 3u; i++) fs |= ((u32)(mn[i] - (int)((first_min >> (8u * i)) & 0xFFu)) & 0xFFu) << (8u + 8u * i); // signed bytes
			}
		}
		uint4 *rec = reinterpret_cast<uint4 *>(ka->out + blockIdx.x);
		rec[0] = b0;
		rec[1] = make_uint4(b1.x, b1.y, b1.z, fs);
	}
	// the key slots past the period are zero
	if (ka->keys)
	{
		u64 *mine = ka->keys + (size_t)blockIdx.x * ka->keys_stride;
		for (u32 base = period; base < ka->keys_stride; base += kThreads) // workgroup-uniform bounds
			if (base + wave * 64u + row < ka->keys_stride) mine[base + wave * 64u + row] = 0ull;
	}
}

__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_canon_period_vn64(CanonPeriodArgs a) { canon_period_run<VnStep>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_canon_period_moore64(CanonPeriodArgs a) { canon_period_run<MooreStep>(a); }
__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_canon_period_clustered64(CanonPeriodArgs a) { canon_period_run<ClusteredStep>(a); }

} // namespace

hipError_t launch_canon_period(const CanonPeriodLaunch &l, hipStream_t stream)
{
	if (l.count == 0 || (l.clustered && l.neighbourhood != CA3D_ENSEMBLE_MOORE) || (l.keys && l.keys_stride == 0)) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_canon_period) == 32, "a record is two 16-byte stores");
	static_assert(MooreStep::kXchWords / 2u * 4u + kCanonBytes <= 163840u, "one parity of the Moore exchange and canon's arrays fit a workgroup's LDS");
	CanonPeriodArgs a;
	a.state = l.state;
	a.rules = l.rules;
	a.periods = l.periods;
	a.out = l.out;
	a.keys = reinterpret_cast<u64 *>(l.keys);
	a.keys_stride = l.keys_stride;
	a.first = l.first;
	auto kernel = l.clustered ? ca_ensemble_canon_period_clustered64 : l.neighbourhood == CA3D_ENSEMBLE_MOORE ? ca_ensemble_canon_period_moore64 : ca_ensemble_canon_period_vn64;
	hipLaunchKernelGGL(kernel, dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
