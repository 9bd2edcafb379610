// Envelope kernels behind ca3d_ensemble_envelope (include/ca3d.h): how a universe oscillates over the phases t = 0 .. period - 1 of its
// own evolution — the cells that ever live (the envelope E, the OR of the phases), the cells that always live (the stator A, their AND),
// the cells that change (the rotor E & ~A), how much changes a step (the heat) — in ONE launch that only reads the source ensemble and
// may write the three images into universes of a destination. ONE workgroup a universe; nine kernels, three ensemble kinds x three
// boundaries, share the body envelope_run<Step, InRegisters> and differ in the step policy (ca_ensemble_step.inc: VnStepT<B>,
// MooreStepT<B>, ClusteredStepT<B>).
//
// The universe is loaded once into the ensemble's register layout (ca_flood.inc's load_universe), the rule's leaves once (Step::load),
// the period once, workgroup-uniform. Round t of the loop, t = 0 .. period - 1, with S_t in the thread's eight registers:
//   1. the thread's eight words go into its sixteen accumulator words (OR, AND) and their popcount into its population count;
//   2. one Step::step makes S_t+1, behind the step's barrier (B1);
//   3. the popcount of S_t ^ S_t+1 goes into the thread's heat count. (A thread's 256 cells over 4096 steps: 2^20 at most, a word each.)
// Behind the loop the thread reads its eight words of S_0 again from global memory — the source is unchanged — and compares them with
// S_period for RETURNS; the wave's ballot, heat and population go to `red`; extent of E (its barrier is also red's) and extent of
// E & ~A give populations and boxes; thread 0 writes the record, three 16-byte stores; every thread writes its rows of the selected
// images into both buffers of the destination universes, and thread 0 copies the rule words there when asked.
//
// WHERE THE ACCUMULATORS LIVE, chosen per kind.
//   von Neumann: in REGISTERS. The step takes 69 vector registers with its fourteen leaves; sixteen accumulator words and the two
//     counts fit beside it under the 128 a thread of 1024 may hold. The exchange keeps both parities (32 KiB), a step ONE barrier.
//   Moore and clustered: in LDS. Their steps take all 128 registers with the leaves, so the sixteen words and the two counts lie in
//     acc[word][thread], 18 x 4 KiB = 72 KiB, each slot one thread's alone (no barrier orders them), as `kept` in ca_canon_period.hip.
//     clustered: the exchange is the von Neumann one, both parities, 32 KiB: ONE barrier a step, 107 776 B with the partials.
//     Moore: both parities of the exchange would be 128 KiB, 200 KiB with acc; so ONE parity (64 KiB, buffer 0 always) and a SECOND
//       barrier a step (B2) behind the step. The argument is ca_canon_period.hip's: the last read of the exchange in round t follows
//       B1 of round t and lies in front of B2; its next write lies behind B2, which no wave passes before every wave has finished
//       those reads. 64 KiB + 72 KiB + partials = 140 544 B of the 163 840 a workgroup may hold.
//   A policy with both parities alternates them (t & 1): a wave writes a parity again two steps on, behind the next step's barrier,
//   which no wave passes before it has read this one's (ca_ensemble_run.inc's loop).
//
// BARRIERS behind the loop: `red` and partE are written in front of extent(E)'s barrier and read behind it; partR is an array of its
// own, because a fast wave writes the second extent's partials while a slow one still reads the first's. The step's exchange is not
// touched again. Layout, load_universe, extent and the invariants (every barrier reached by all 1024 threads, every loop bound uniform
// over the workgroup, no waits on other workgroups, no spins, no atomics, nothing but vector stores) are ca_flood.inc's.
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

struct EnvelopeArgs
{
	const u32 *state;        // [Bs][8192], the source ensemble's current states
	const u32 *rules;        // [Bs][rule words of the kind]
	const u32 *periods;      // [count]
	ca3d_envelope *out;      // [count]
	u32 *dst_state, *dst_prev; // [Bd][8192], both buffers of the destination ensemble; unused without images
	u32 *dst_rules;          // [Bd][rule_words]
	u32 first, dst_first;
	u32 images;              // CA3D_ENVELOPE_IMAGE_* bits
	u32 rule_words;          // 0: the destinations' rules stay
};

constexpr u32 kAccWords = 2u * kPT * 2u + 2u;  // OR and AND of the thread's eight words, its population and heat counts
constexpr u32 kRedWords = kWaves * 4u;         // a wave's "S_period differs from S_0", heat, population, unused

// an accumulator's box as the record holds it: min and max as x | y << 8 | z << 16, both zero for an empty set
__device__ __forceinline__ uint2 box_of(const Extent &e)
{
	if (e.pop == 0u) return make_uint2(0u, 0u);
	const u64 xm = (u64)e.x1 << 32 | e.x0;
	return make_uint2((u32)__builtin_ctzll(xm) | (u32)__builtin_ctzll(e.ym) << 8 | (u32)__builtin_ctzll(e.zm) << 16,
	                  (63u - (u32)__builtin_clzll(xm)) | (63u - (u32)__builtin_clzll(e.ym)) << 8 | (63u - (u32)__builtin_clzll(e.zm)) << 16);
}

template <typename Step, bool InRegisters>
__device__ __forceinline__ void envelope_run(const EnvelopeArgs &a)
{
	constexpr u32 kAccBytes = InRegisters ? 0u : kAccWords * kThreads * 4u;
	// ONE parity of the exchange where two do not fit beside the accumulators (the header)
	constexpr bool kOneParity = Step::kXchWords * 4u + kAccBytes + (2u * kPartWords + kRedWords) * 4u > 163840u;
	static_assert((kOneParity ? Step::kXchWords / 2u : Step::kXchWords) * 4u + kAccBytes + (2u * kPartWords + kRedWords) * 4u <= 163840u, "a workgroup's LDS");
	__shared__ __attribute__((aligned(16))) u32 xch[kOneParity ? Step::kXchWords / 2u : Step::kXchWords];
	__shared__ __attribute__((aligned(16))) u32 acc[InRegisters ? 4u : kAccWords * kThreads]; // [word][thread]
	__shared__ __attribute__((aligned(16))) u32 partE[kPartWords];
	__shared__ __attribute__((aligned(16))) u32 partR[kPartWords];
	__shared__ __attribute__((aligned(16))) u32 red[kRedWords];

	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const u32 u = a.first + blockIdx.x;
	const u32 *mine = a.state + (size_t)u * kEnsembleWords;
	const u32 period = (u32)__builtin_amdgcn_readfirstlane((int)a.periods[blockIdx.x]); // workgroup-uniform, read once

	Step st;
	st.load(a.rules, u);
	u32 R[kPT][2];
	load_universe(mine, wave, row, R);

	u32 E[kPT][2], A[kPT][2], pops = 0, heat = 0; // InRegisters: the accumulators; else what is read out of acc behind the loop
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			E[p][h] = 0u;
			A[p][h] = ~0u;
			if (!InRegisters)
			{
				acc[(2u * p + h) * kThreads + tid] = 0u;
				acc[(2u * kPT + 2u * p + h) * kThreads + tid] = ~0u;
			}
		}
	if (!InRegisters) acc[(4u * kPT) * kThreads + tid] = acc[(4u * kPT + 1u) * kThreads + tid] = 0u;

#pragma nounroll
	for (u32 t = 0; t < period; t++) // a workgroup-uniform bound
	{
		u32 pc = 0;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				pc += (u32)__popc(R[p][h]);
				if (InRegisters)
				{
					E[p][h] |= R[p][h];
					A[p][h] &= R[p][h];
				}
				else
				{
					acc[(2u * p + h) * kThreads + tid] |= R[p][h];
					acc[(2u * kPT + 2u * p + h) * kThreads + tid] &= R[p][h];
				}
			}
		if (InRegisters) pops += pc;
		else acc[(4u * kPT) * kThreads + tid] += pc;

		u32 N[kPT][2];
		st.step(R, N, xch, kOneParity ? 0u : t & 1u, wave, row); // its barrier is B1
		u32 hc = 0;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				hc += (u32)__popc(R[p][h] ^ N[p][h]);
				R[p][h] = N[p][h];
			}
		if (InRegisters) heat += hc;
		else acc[(4u * kPT + 1u) * kThreads + tid] += hc;
		if (kOneParity) __syncthreads(); // B2: the next round's exchange writes come behind this round's reads (the header)
	}

	if (!InRegisters)
	{
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				E[p][h] = acc[(2u * p + h) * kThreads + tid];
				A[p][h] = acc[(2u * kPT + 2u * p + h) * kThreads + tid];
			}
		pops = acc[(4u * kPT) * kThreads + tid];
		heat = acc[(4u * kPT + 1u) * kThreads + tid];
	}

	// ---- RETURNS: S_period against S_0, word for word; S_0 from global memory again
	u32 ch = 0;
	{
		u32 S0[kPT][2];
		load_universe(mine, wave, row, S0);
#pragma unroll
		for (u32 p = 0; p < kPT; p++) ch |= (S0[p][0] ^ R[p][0]) | (S0[p][1] ^ R[p][1]);
	}
	const u32 differs = __ballot(ch != 0u) != 0ull ? 1u : 0u; // every lane votes
	heat = wave_add(heat);
	pops = wave_add(pops);
	if (row == 0u) *reinterpret_cast<uint4 *>(red + 4u * wave) = make_uint4(differs, heat, pops, 0u);

	u32 Ro[kPT][2];
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
#pragma unroll
		for (u32 h = 0; h < 2u; h++) Ro[p][h] = E[p][h] & ~A[p][h];
	const Extent ee = extent(E, partE, wave, row); // its barrier is also red's
	const Extent er = extent(Ro, partR, wave, row);

	if (tid == 0u)
	{
		u32 any = 0, hsum = 0, psum = 0;
#pragma unroll
		for (u32 w = 0; w < kWaves; w++)
		{
			const uint4 v = *reinterpret_cast<const uint4 *>(red + 4u * w);
			any |= v.x; hsum += v.y; psum += v.z;
		}
		const uint2 be = box_of(ee), br = box_of(er);
		uint4 *rec = reinterpret_cast<uint4 *>(a.out + blockIdx.x);
		rec[0] = make_uint4(period, any ? 0u : (u32)CA3D_ENVELOPE_RETURNS, hsum, psum);
		rec[1] = make_uint4(ee.pop, ee.pop - er.pop, be.x, be.y); // the stator is the envelope without the rotor
		rec[2] = make_uint4(br.x, br.y, 0u, 0u);
	}

	// ---- the images, in bit order, into both buffers of universes dst_first + k n + i
	const u32 n_images = (u32)__popc(a.images & 7u);
	if (n_images == 0u) return; // workgroup-uniform, and no barrier follows
	u32 slot = a.dst_first + blockIdx.x * n_images;
	auto put = [&](const u32 (&img)[kPT][2]) __attribute__((always_inline)) {
		const size_t off = (size_t)slot * kEnsembleWords;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
		{
			const size_t at = off + (size_t)((wave * kPT + p) * 64u + row) * 2u; // inside universe `slot` of the destination
			*reinterpret_cast<uint2 *>(a.dst_state + at) = make_uint2(img[p][0], img[p][1]);
			*reinterpret_cast<uint2 *>(a.dst_prev + at) = make_uint2(img[p][0], img[p][1]);
		}
		if (tid == 0u)
		{
			const u32 *rs = a.rules + (size_t)u * Step::kRuleWords;
			u32 *rd = a.dst_rules + (size_t)slot * Step::kRuleWords;
#pragma nounroll
			for (u32 i = 0; i < a.rule_words; i++) rd[i] = rs[i]; // rule_words is 0 or Step::kRuleWords
		}
		slot++;
	};
	if (a.images & CA3D_ENVELOPE_IMAGE_ENVELOPE) put(E);
	if (a.images & CA3D_ENVELOPE_IMAGE_STATOR) put(A);
	if (a.images & CA3D_ENVELOPE_IMAGE_ROTOR) put(Ro);
}

// a kind's kernels under the three boundaries; four waves per SIMD as in ca_ensemble.hip
#define CA3D_ENVELOPE_KERNELS(kind, StepT, regs)                                                                                                              \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_envelope_##kind##64(EnvelopeArgs a) { envelope_run<StepT<kBoundaryReference>, regs>(a); }      \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_envelope_##kind##64_torus(EnvelopeArgs a) { envelope_run<StepT<kBoundaryTorus>, regs>(a); }    \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_envelope_##kind##64_closed(EnvelopeArgs a) { envelope_run<StepT<kBoundaryClosed>, regs>(a); }
CA3D_ENVELOPE_KERNELS(vn, VnStepT, true)
CA3D_ENVELOPE_KERNELS(moore, MooreStepT, false)
CA3D_ENVELOPE_KERNELS(clustered, ClusteredStepT, false)
#undef CA3D_ENVELOPE_KERNELS

} // namespace

hipError_t launch_envelope(const EnvelopeLaunch &l, hipStream_t stream)
{
	const u32 kind = l.clustered ? 2u : l.neighbourhood == CA3D_ENSEMBLE_MOORE ? 1u : 0u;
	if (l.count == 0 || (l.clustered && l.neighbourhood != CA3D_ENSEMBLE_MOORE) || l.boundary < 0 || l.boundary > CA3D_ENSEMBLE_BOUNDARY_CLOSED) return hipErrorInvalidValue;
	if (l.images & ~7u) return hipErrorInvalidValue;
	if (l.images && (!l.dst_state || !l.dst_prev)) return hipErrorInvalidValue;
	if (l.rule_words && (!l.images || !l.dst_rules || l.rule_words != ensemble_rule_words(l.neighbourhood, l.clustered))) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_envelope) == 48, "a record is three 16-byte stores");
	EnvelopeArgs a;
	a.state = l.state;
	a.rules = l.rules;
	a.periods = l.periods;
	a.out = l.out;
	a.dst_state = l.dst_state;
	a.dst_prev = l.dst_prev;
	a.dst_rules = l.dst_rules;
	a.first = l.first;
	a.dst_first = l.dst_first;
	a.images = l.images;
	a.rule_words = l.rule_words;
	typedef void (*Kernel)(EnvelopeArgs);
	static const Kernel kernels[3][3] = {{ca_ensemble_envelope_vn64, ca_ensemble_envelope_vn64_torus, ca_ensemble_envelope_vn64_closed},
	                                     {ca_ensemble_envelope_moore64, ca_ensemble_envelope_moore64_torus, ca_ensemble_envelope_moore64_closed},
	                                     {ca_ensemble_envelope_clustered64, ca_ensemble_envelope_clustered64_torus, ca_ensemble_envelope_clustered64_closed}};
	hipLaunchKernelGGL(kernels[kind][l.boundary], dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
