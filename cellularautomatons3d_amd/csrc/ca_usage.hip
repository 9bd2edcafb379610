// Usage kernels behind ca3d_ensemble_usage (include/ca3d.h): which entries of its rule tables a universe's run reads. For every step
// t = 0 .. P - 1 of the universe's own evolution every cell adds one to the bin (dead or alive in S_t, its neighbour count) of every
// table the kind looks up — von Neumann: F; Moore: the 26-count; clustered: T = F + E + C, E and C — in ONE launch that only reads the
// ensemble. ONE workgroup a universe; nine kernels, three ensemble kinds x three boundaries, share the body usage_run<Step> and differ
// in the step body (VnUsage<B>, MooreUsage<B>, ClusteredUsage<B> below).
//
// THE STEP BODIES are this unit's own: the policies of ca_ensemble_step.inc consume the count planes inside rule() and hide them. The
// bodies here keep those policies' neighbour access (Faces<B>) and adder trees (sum6, sum4, fa, ha, sum_moore,
// MooreStepT::plane_sum, ClusteredStepT::plane_set) and replace rule() by `tail`, which does both jobs from the same planes of one
// word w of 32 cells:
//   1. the count's planes are decoded into one-hot masks in two halves: lo[j], the minterms of the low two or three planes, and
//      hiA[k] / hiD[k], the minterms of the high planes ANDed with w / ~w. Bin c of the live cells is a = lo & hiA, of the dead d = lo & hiD;
//   2. popcount(a) and popcount(d) go into the bin's accumulator;
//   3. the next word is the OR over the bins of (a & survive_c) | (d & born_c): the leaves are all-ones or zero and uniform over the
//      workgroup, so they are formed by the scalar unit from the rule's words (one s_bfe_i32 each, where they are used), and no
//      multiplexer tree and no vector leaf is needed.
// Moore's planes count the cell itself (T = 0 .. 27, MooreStepT): a dead cell's bin is T, a live one's T - 1 (kSelf).
//
// WHERE THE STATE LIVES: in LDS, img[step parity][plane of the wave][word][thread], 2 x 32 KiB, not in registers: the accumulators
// need them. Step t reads S_t from parity t & 1 and writes S_t+1 into the other; ONE barrier a step, behind the writes, which no wave
// passes before every wave has finished reading S_t. A thread slides a window of three planes' sets over the six planes it sees, one
// word of a row at a time (ClusteredStepT's walk, here for all three kinds): its own four planes and the neighbouring waves' last and
// first plane, read straight out of the image — there is no exchange beside it — or dead, by the boundary. Moore forms the plane sums
// of those two planes itself (two of six a word more) instead of passing four sum planes through an exchange of 128 KiB.
//
// WHERE THE ACCUMULATORS LIVE: in REGISTERS, two 16-bit counts a register (alive low, dead high), one register a bin — 7, 27 and 49 for
// the three kinds — and in tot[wave][2 bins] LDS words behind them. A thread's share of one bin is 256 cells a step at most, so a
// register holds kFlush = 255 steps (255 * 256 < 2^16); the loop over the steps runs in stretches of kFlush at most, and behind a stretch
// every wave sums its registers' halves (wave_sum_uniform: DPP and the scalar unit, no LDS) and its lane 0 adds them to the wave's own
// tot words. Nothing orders those: a tot word is one thread's alone until the barrier behind the loop. A wave's share of a bin over
// 4096 steps is 2^26, the universe's 2^30: one word each.
// Behind the loop, ONE barrier; thread i < 98 sums bin i of the record over the sixteen waves into fin[i]; a second barrier; thread
// i < 108 writes word i of the record — the used masks are formed from fin by the six threads that write them.
//
// Every barrier is reached by all 1024 threads; every loop bound is uniform over the workgroup; no waits on other workgroups, no
// spins, no atomics, nothing but vector stores (ca_flood.inc's invariants).
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
#include "ca_ensemble_step.inc"

static_assert(kBoundaryReference == CA3D_ENSEMBLE_BOUNDARY_REFERENCE && kBoundaryTorus == CA3D_ENSEMBLE_BOUNDARY_TORUS &&
                  kBoundaryClosed == CA3D_ENSEMBLE_BOUNDARY_CLOSED,
              "the policies' boundary is the ABI's");

struct UsageArgs
{
	const u32 *state; // [B][8192], the ensemble's current states
	const u32 *rules; // [B][rule words of the kind]
	const u32 *steps; // [count]
	ca3d_usage *out;  // [count]
	u32 first;
};

constexpr u32 kFlush = 255u;                    // steps a packed accumulator holds: 255 * 256 cells of a thread < 2^16
constexpr u32 kRecordWords = sizeof(ca3d_usage) / 4u;
constexpr u32 kDeadAt = 8u, kAliveAt = kDeadAt + CA3D_USAGE_BINS; // words of the record
static_assert(sizeof(ca3d_usage) == 432 && kAliveAt + CA3D_USAGE_BINS + 2u == kRecordWords, "the record's layout");

// all-ones where bit c of a table is set; `table` is uniform, so this is the scalar unit's
__device__ __forceinline__ u32 leaf(u32 table, int c) { return (u32)((int)(table << (31 - c)) >> 31); }

// One word's share of one table: N bins (counts 0 .. N - 1) of the count whose NP bit planes are P, for the cells w. kSelf: the planes
// count the cell itself, so a live cell's bin is the count less one. Adds to acc[kBase .. kBase + N), returns the table's say on the
// next word. kOpaque: the tables are made opaque here, so their leaves are formed again for every word and do not stay in scalar
// registers across the step (clustered: 98 of them).
template <int N, int NP, int kSelf, int kBase, bool kOpaque, int NA>
__device__ __forceinline__ u32 tail(const u32 (&P)[NP], u32 w, u32 born, u32 surv, u32 (&acc)[NA])
{
	constexpr int LB = NP >= 5 ? 3 : 2, NL = 1 << LB, NH = ((N - 1 + kSelf) >> LB) + 1;
	static_assert(kBase + N <= NA && NP - LB >= 1 && NP - LB <= 2, "bins and planes");
	if (kOpaque)
	{
		asm volatile("" : "+s"(born));
		asm volatile("" : "+s"(surv));
	}
	u32 lo[NL], hiA[NH], hiD[NH];
#pragma unroll
	for (int j = 0; j < NL; j++)
	{
		u32 m = (j & 1 ? P[0] : ~P[0]) & (j & 2 ? P[1] : ~P[1]);
		if (LB == 3) m &= j & 4 ? P[2] : ~P[2];
		lo[j] = m;
	}
#pragma unroll
	for (int k = 0; k < NH; k++)
	{
		u32 m = k & 1 ? P[LB] : ~P[LB];
		if (NP - LB == 2) m &= k & 2 ? P[NP - 1] : ~P[NP - 1];
		hiA[k] = m & w;
		hiD[k] = m & ~w;
	}
	// Bin by bin, in this order: left to itself the compiler forms every mask of the word first and the leaves as 2 N condition pairs
	// held across the step, and spills both. The empty statements pin a leaf to a scalar register where it is used, and make the
	// masks of bin c + 1 wait for bin c's counts and its share of the next word.
	u32 next = 0u;
#pragma unroll
	for (int c = 0; c < N; c++)
	{
		const u32 a = lo[(c + kSelf) & (NL - 1)] & hiA[(c + kSelf) >> LB], d = lo[c & (NL - 1)] & hiD[c >> LB];
		acc[kBase + c] += (u32)__popc(a);
		acc[kBase + c] += (u32)__popc(d) << 16;
		u32 ls = leaf(surv, c), lb = leaf(born, c);
		asm volatile("" : "+s"(ls), "+s"(lb));
		next |= a & ls;
		next |= d & lb;
		if (c + 1 < N)
		{
			if (kSelf) asm volatile("" : "+v"(next), "+v"(acc[kBase + c]), "+v"(lo[(c + 1) & (NL - 1)]), "+v"(lo[(c + 1 + kSelf) & (NL - 1)]));
			else asm volatile("" : "+v"(next), "+v"(acc[kBase + c]), "+v"(lo[(c + 1) & (NL - 1)]));
		}
	}
	return next;
}

// ---- the three kinds: what a plane's word contributes to its neighbours' counts (Set, `set`) and one word's counts and tails (`word`)
// ---- von Neumann: the raw word of the planes below and above; x and y of the plane itself
template <int B>
struct VnUsage
{
	static constexpr u32 kBins = 7u;
	struct Set { u32 c, other; };
	u32 born, surv;

	__device__ __forceinline__ void load(const u32 *rules, u32 u)
	{
		const u32 lut = rules[u]; // lut_s | lut_b << 8
		surv = lut & 0x7Fu;
		born = (lut >> 8) & 0x7Fu;
	}
	static __device__ __forceinline__ Set set(u32 w, u32 other, u32 h) { return Set{w, other}; }
	__device__ __forceinline__ u32 word(const Set &b, const Set &m, const Set &a, u32 h, u32 (&acc)[kBins]) const
	{
		const u32 w = m.c;
		const u32 l = Faces<B>::left(w, m.other, h), r = Faces<B>::right(w, m.other, h);
		u32 F[3];
		sum6(l, r, Faces<B>::row_below(w), Faces<B>::row_above(w), b.c, a.c, F);
		return tail<7, 3, 0, 0, true>(F, w, born, surv, acc);
	}
};

// ---- Moore: MooreStepT<B>'s plane sums (x and y, the cell itself counted), three of them added along z
template <int B>
struct MooreUsage
{
	typedef MooreStepT<B> Base;
	static constexpr u32 kBins = 27u;
	struct Set { u32 c; typename Base::Sum4 q; };
	u32 born, surv;

	__device__ __forceinline__ void load(const u32 *rules, u32 u)
	{
		born = rules[2u * u] & 0x7FFFFFFu;
		surv = rules[2u * u + 1u] & 0x7FFFFFFu;
	}
	static __device__ __forceinline__ Set set(u32 w, u32 other, u32 h) { return Set{w, Base::plane_sum(w, other, h)}; }
	__device__ __forceinline__ u32 word(const Set &b, const Set &m, const Set &a, u32 h, u32 (&acc)[kBins]) const
	{
		u32 s0, k0, s1, k1, s2, k2, s3, k3;
		fa(b.q.b[0], m.q.b[0], a.q.b[0], s0, k0);
		fa(b.q.b[1], m.q.b[1], a.q.b[1], s1, k1);
		fa(b.q.b[2], m.q.b[2], a.q.b[2], s2, k2);
		fa(b.q.b[3], m.q.b[3], a.q.b[3], s3, k3);
		u32 T[5], c1, c2, c3;
		T[0] = s0;
		ha(s1, k0, T[1], c1);
		fa(s2, k1, c1, T[2], c2);
		fa(s3, k2, c2, T[3], c3);
		T[4] = k3 | c3; // T <= 27: no carry out
		return tail<27, 5, 1, 0, true>(T, m.c, born, surv, acc);
	}
};

// ---- clustered: ClusteredStepT<B>'s sets and its F, E, C, T, with three tails, ORed, in place of rule(); bins 0 .. 26 main (T),
// 27 .. 39 edges (E), 40 .. 48 corners (C), the record's order
template <int B>
struct ClusteredUsage
{
	typedef ClusteredStepT<B> Base;
	typedef typename Base::Set Set;
	static constexpr u32 kBins = CA3D_USAGE_BINS;
	static_assert(CA3D_USAGE_EDGES == 27u && CA3D_USAGE_CORNERS == 40u && CA3D_USAGE_BINS == 49u, "the record's classes");
	u32 t[6]; // born | survive of main, edges, corners

	__device__ __forceinline__ void load(const u32 *rules, u32 u)
	{
#pragma unroll
		for (u32 i = 0; i < 6u; i++) t[i] = rules[6u * u + i];
	}
	static __device__ __forceinline__ Set set(u32 w, u32 other, u32 h) { return Base::plane_set(w, other, h); }
	__device__ __forceinline__ u32 word(const Set &b, const Set &m, const Set &a, u32 h, u32 (&acc)[kBins]) const
	{
		u32 F[3], E[4], C[4], T[5], k1, k2, k3, k4, k5, x, y;
		fa(m.d[0], b.c, a.c, F[0], k1);
		ha(m.d[1], k1, F[1], k2);
		F[2] = m.d[2] | k2; // D == 4 leaves no carry below it
		fa(m.as[0], b.d[0], a.d[0], E[0], k1);
		fa(m.as[1], b.d[1], a.d[1], x, k2);
		ha(x, k1, E[1], k3);
		fa(m.as[2], b.d[2], a.d[2], y, k4);
		fa(y, k2, k3, E[2], k5);
		E[3] = k4 | k5; // E <= 12: one carry into plane 3 at most
		ha(b.as[0], a.as[0], C[0], k1);
		fa(b.as[1], a.as[1], k1, C[1], k2);
		fa(b.as[2], a.as[2], k2, C[2], C[3]);
		sum_moore(F, E, C, T);
		const u32 w = m.c;
		u32 next = tail<27, 5, 0, 0, true>(T, w, t[0] & 0x7FFFFFFu, t[1] & 0x7FFFFFFu, acc);
		next |= tail<13, 4, 0, 27, true>(E, w, t[2] & 0x1FFFu, t[3] & 0x1FFFu, acc);
		next |= tail<9, 4, 0, 40, true>(C, w, t[4] & 0x1FFu, t[5] & 0x1FFu, acc);
		return next;
	}
};

// One step: S_t in img[buf], S_t+1 into img[buf ^ 1]; the caller's barrier follows. A thread slides a window of three planes' sets
// over the six planes it sees, one word of a row at a time (ClusteredStepT's walk): planes 4 w .. 4 w + 3 are its own words, plane
// 4 w - 1 and 4 w + 4 the neighbouring waves' rows, or dead, by the boundary.
template <int B, typename Step>
__device__ __forceinline__ void usage_step(const Step &st, const u32 *img, u32 buf, u32 wave, u32 row, u32 (&acc)[Step::kBins])
{
	const u32 *src = img + buf * kEnsembleWords;
	u32 *dst = const_cast<u32 *>(img) + (buf ^ 1u) * kEnsembleWords + wave * 64u + row;
	// word h of row `row` of plane p of wave w: [p][h][thread]
	auto at = [&](u32 w, u32 p, u32 h) { return src[(2u * p + h) * kThreads + w * 64u + row]; };
#pragma unroll
	for (u32 h = 0; h < 2u; h++)
	{
		// (a plane that does not exist is read from a slot inside the image and zeroed: no branch)
		const u32 wb = Faces<B>::kMinusWraps ? Faces<B>::wave_below(wave) : wave ? wave - 1u : 0u, keep_b = Faces<B>::has_below(wave) ? ~0u : 0u;
		const u32 wa = Faces<B>::wave_above(wave), keep_a = Faces<B>::has_above(wave) ? ~0u : 0u;
		const u32 b0 = at(wb, kPT - 1u, h) & keep_b, b1 = at(wb, kPT - 1u, h ^ 1u) & keep_b; // z == -1: plane 63, or dead
		typename Step::Set lo = Step::set(b0, b1, h), mid = Step::set(at(wave, 0u, h), at(wave, 0u, h ^ 1u), h);
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
		{
			// z == 64: plane 0, or dead
			const u32 a0 = p + 1u < kPT ? at(wave, p + 1u, h) : at(wa, 0u, h) & keep_a, a1 = p + 1u < kPT ? at(wave, p + 1u, h ^ 1u) : at(wa, 0u, h ^ 1u) & keep_a;
			const typename Step::Set hi = Step::set(a0, a1, h);
			dst[(2u * p + h) * kThreads] = st.word(lo, mid, hi, h, acc);
			lo = mid;
			mid = hi;
		}
	}
}

template <int B, typename Step>
__device__ __forceinline__ void usage_run(const UsageArgs &a)
{
	constexpr u32 NB = Step::kBins;
	static_assert((2u * kEnsembleWords + kWaves * 2u * NB + 2u * CA3D_USAGE_BINS) * 4u <= 163840u, "a workgroup's LDS");
	__shared__ __attribute__((aligned(16))) u32 img[2u * kEnsembleWords]; // [step parity][plane of the wave][word][thread]
	__shared__ u32 tot[kWaves * 2u * NB];       // [wave][alive bins | dead bins], a wave's words its lane 0's alone until the barrier
	__shared__ u32 fin[2u * CA3D_USAGE_BINS];   // the record's dead[] and alive[]

	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const u32 u = a.first + blockIdx.x;
	const u32 P = (u32)__builtin_amdgcn_readfirstlane((int)a.steps[blockIdx.x]); // workgroup-uniform, read once

	Step st;
	st.load(a.rules, u);
	{
		u32 R[kPT][2];
		load_universe(a.state + (size_t)u * kEnsembleWords, wave, row, R);
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++) img[(2u * p + h) * kThreads + tid] = R[p][h];
	}

	u32 *const mine = tot + wave * (2u * NB);
	if (row == 0u)
#pragma unroll
		for (u32 i = 0; i < 2u * NB; i++) mine[i] = 0u;

	u32 acc[NB];
#pragma unroll
	for (u32 i = 0; i < NB; i++) acc[i] = 0u;

	__syncthreads(); // S_0 lies in img[0]
	u32 t = 0;
#pragma nounroll
	while (t < P) // workgroup-uniform bounds, here and below
	{
		const u32 end = P - t > kFlush ? t + kFlush : P;
#pragma nounroll
		for (; t < end; t++)
		{
			usage_step<B>(st, img, t & 1u, wave, row, acc);
			__syncthreads(); // S_t+1 lies in the other parity, and nobody reads S_t any more
		}
		// the stretch's counts: out of the packed registers into the wave's words
#pragma unroll
		for (u32 i = 0; i < NB; i++)
		{
			const u32 alive = wave_sum_uniform(acc[i] & 0xFFFFu), dead = wave_sum_uniform(acc[i] >> 16);
			if (row == 0u)
			{
				mine[i] += alive;
				mine[NB + i] += dead;
			}
			acc[i] = 0u;
		}
	}
	__syncthreads(); // (every wave's tot words; the loop's last barrier orders only the images)

	// the record's bin i (dead[] then alive[]) over the waves; a bin the kind does not have is zero
	if (tid < 2u * CA3D_USAGE_BINS)
	{
		const u32 is_alive = tid >= CA3D_USAGE_BINS ? 1u : 0u, bin = tid - is_alive * CA3D_USAGE_BINS;
		u32 sum = 0u;
		if (bin < NB)
#pragma unroll
			for (u32 w = 0; w < kWaves; w++) sum += tot[w * (2u * NB) + (is_alive ? 0u : NB) + bin];
		fin[tid] = sum;
	}
	__syncthreads();
	if (tid < kRecordWords)
	{
		u32 v = 0u;
		if (tid == 0u) v = P;
		else if (tid >= 2u && tid < 8u)
		{
			// used_born[3] from dead[], used_survive[3] from alive[]: bit c set where the class's bin c is not zero
			const u32 cls = (tid - 2u) % 3u, from = tid < 5u ? 0u : CA3D_USAGE_BINS;
			const u32 base = cls == 0u ? CA3D_USAGE_MAIN : cls == 1u ? CA3D_USAGE_EDGES : CA3D_USAGE_CORNERS;
			const u32 n = cls == 0u ? 27u : cls == 1u ? 13u : 9u;
#pragma nounroll
			for (u32 c = 0; c < n; c++) v |= fin[from + base + c] != 0u ? 1u << c : 0u;
		}
		else if (tid >= kDeadAt && tid < kAliveAt + CA3D_USAGE_BINS) v = fin[tid - kDeadAt];
		reinterpret_cast<u32 *>(a.out + blockIdx.x)[tid] = v;
	}
}

// a kind's kernels under the three boundaries; four waves per SIMD as in ca_ensemble.hip
#define CA3D_USAGE_KERNELS(kind, StepT)                                                                                                     \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_usage_##kind##64(UsageArgs a) { usage_run<kBoundaryReference, StepT<kBoundaryReference>>(a); }  \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_usage_##kind##64_torus(UsageArgs a) { usage_run<kBoundaryTorus, StepT<kBoundaryTorus>>(a); } \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_usage_##kind##64_closed(UsageArgs a) { usage_run<kBoundaryClosed, StepT<kBoundaryClosed>>(a); }
CA3D_USAGE_KERNELS(vn, VnUsage)
CA3D_USAGE_KERNELS(moore, MooreUsage)
CA3D_USAGE_KERNELS(clustered, ClusteredUsage)
#undef CA3D_USAGE_KERNELS

} // namespace

hipError_t launch_usage(const UsageLaunch &l, hipStream_t stream)
{
	const u32 kind = l.clustered ? 2u : l.neighbourhood == CA3D_ENSEMBLE_MOORE ? 1u : 0u;
	if (l.count == 0 || (l.clustered && l.neighbourhood != CA3D_ENSEMBLE_MOORE) || l.boundary < 0 || l.boundary > CA3D_ENSEMBLE_BOUNDARY_CLOSED) return hipErrorInvalidValue;
	if (!l.state || !l.rules || !l.steps || !l.out) return hipErrorInvalidValue;
	UsageArgs a;
	a.state = l.state;
	a.rules = l.rules;
	a.steps = l.steps;
	a.out = l.out;
	a.first = l.first;
	typedef void (*Kernel)(UsageArgs);
	static const Kernel kernels[3][3] = {{ca_ensemble_usage_vn64, ca_ensemble_usage_vn64_torus, ca_ensemble_usage_vn64_closed},
	                                     {ca_ensemble_usage_moore64, ca_ensemble_usage_moore64_torus, ca_ensemble_usage_moore64_closed},
	                                     {ca_ensemble_usage_clustered64, ca_ensemble_usage_clustered64_torus, ca_ensemble_usage_clustered64_closed}};
	hipLaunchKernelGGL(kernels[kind][l.boundary], dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
