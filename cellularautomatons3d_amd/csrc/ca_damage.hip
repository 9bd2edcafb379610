// Damage kernels behind ca3d_ensemble_damage (include/ca3d.h): how a perturbation spreads. A universe's state S and a perturbed twin T
// are stepped side by side under the universe's rule and the ensemble's boundary, and the Hamming distance d_t = popcount(S_t ^ T_t) is
// taken at every t = 0 .. P, in ONE launch that only reads the source ensemble and may write the last difference D_P = S_P ^ T_P into a
// universe of a destination. ONE workgroup a universe; nine kernels, three ensemble kinds x three boundaries, share the body
// damage_run<Step, InRegisters> and differ in the step policy (ca_ensemble_step.inc: VnStepT<B>, MooreStepT<B>, ClusteredStepT<B>).
//
// S_0 is loaded into the ensemble's register layout (ca_flood.inc's load_universe), the rule's leaves once (Step::load), the step count
// P, the twin's universe and the four flip words once, workgroup-uniform. T_0 is the twin's universe (the source's own by default) with
// the flips XORed in, one after another, by the thread that owns the row. The loop runs over the step CALLS c = 0 .. 2 P - 1 — call
// 2 t steps S_t, call 2 t + 1 steps T_t — so a kernel holds ONE text of the step (two inlined bodies spill in the Moore and clustered
// kernels). Round t, with the thread's popcount of D_t in `pc`:
//   1. the wave's sum of pc goes to dpart[wave], in FRONT of the even call's barrier;
//   2. the even call's Step::step makes S_t+1 out of S_t (its barrier is B1);
//   3. behind B1 every wave reads the sixteen partials: d_t, uniform over the workgroup and held by the scalar unit. Thread 0 writes
//      curve[t] and keeps d_0, the maximum, its t and the sum in `stat`, an LDS record of its own. d_t == 0 ends the loop, for all
//      1024 threads or for none, in front of anything that puts S_t+1 away: S_t == T_t, so every later sample is 0 and D_P is empty;
//   4. S_t+1 is put away, the odd call's Step::step makes T_t+1 (the round's second barrier), T_t+1 is put away;
//   5. D_t+1 = S_t+1 ^ T_t+1 word by word: its popcount is the next pc, its words go into the thread's OR per x half (orx[2]) and its
//      planes into the thread's four-bit mask of planes ever touched.
// dpart is written again only behind the round's second barrier, which no wave passes before every wave has read this round's
// partials, lying as they do between the two barriers: the curve costs no barrier of its own.
// Behind the loop: extent(D_P) gives d_P (its barrier orders the partials) and the damage box; the pseudo-image
// X[p][h] = touched(p) ? orx[h] : 0 has the box of D_0 | .. | D_P along every axis, so extent(X) gives the touched box and no 32 KiB
// image is kept. Thread 0 writes the record, three 16-byte stores; the threads zero the rest of the curve in a strided loop; every
// thread writes its rows of D_P into both buffers of the destination universe when the image is asked for, and thread 0 copies the
// rule words there when asked.
//
// WHERE S AND T LIVE, chosen per kind.
//   von Neumann: in REGISTERS, eight words each. The step takes 69 vector registers with its fourteen leaves; sixteen words of state,
//     orx and the mask fit beside it under the 128 a thread of 1024 may hold. A call steps the first of the pair and leaves
//     (S, T) <- (T, stepped S): (S_t, T_t) in front of an even call, (T_t, S_t+1) in front of an odd one. The exchange keeps both
//     parities (32 KiB): call c takes parity c & 1, so a step is ONE barrier — a wave writes a parity again two step CALLS on, behind
//     the next call's barrier, which no wave passes before it has read this one's (ca_ensemble_run.inc's argument over the call index).
//   Moore and clustered: in LDS. Their steps take all 128 registers with the leaves, so S, T, orx and the mask are parked in
//     park[word][thread], 19 x 4 KiB = 76 KiB, each slot one thread's alone (no barrier orders them; consecutive threads on
//     consecutive banks), as `acc` in ca_envelope.hip. A round is: load S, step, store; load T, step, store; XOR against the parked
//     S word by word. Call c steps the parked state c & 1 in place.
//     clustered: the exchange is the von Neumann one, both parities, 32 KiB, S and T on a parity each: ONE barrier a step.
//     Moore: both parities of the exchange would be 128 KiB, 204 KiB with park; so ONE parity (64 KiB, buffer 0 always) and a SECOND
//       barrier a step (B2) behind each step. The argument is ca_envelope.hip's: the last read of the exchange in a step follows its B1
//       and lies in front of its B2; the next write lies behind B2, which no wave passes before every wave has finished those reads.
//       The early exit lies between B1 and B2 of the even call and is taken by all threads; nothing touches the exchange behind it.
//     Their steps leave no register free, so nothing the lines between the barriers use may live across a step: the lane's number is
//     counted where it is used, and behind the loop the thread's index is formed again from the wave's number and the lane's.
//
// BARRIERS behind the loop: partD is written in front of extent(D_P)'s barrier and read behind it; partX is an array of its own,
// because a fast wave writes the second extent's partials while a slow one still reads the first's. Layout, load_universe, extent and
// the invariants (every barrier reached by all 1024 threads, every loop bound uniform over the workgroup, no waits on other
// workgroups, no spins, no atomics, nothing but vector stores) are ca_flood.inc's.
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

struct DamageArgs
{
	const u32 *state;          // [Bs][8192], the source ensemble's current states
	const u32 *rules;          // [Bs][rule words of the kind]
	const u32 *steps;          // [count]
	const u32 *twins;          // [count], a universe of the source ensemble or CA3D_DAMAGE_SELF
	const u32 *flips;          // [count][CA3D_DAMAGE_FLIPS]
	ca3d_damage *out;          // [count]
	u32 *curve;                // [count][curve_stride], or NULL
	u32 *dst_state, *dst_prev; // [Bd][8192], both buffers of the destination ensemble; unused without the image
	u32 *dst_rules;            // [Bd][rule_words]
	u32 curve_stride;
	u32 first, dst_first;
	u32 image;                 // 0 or CA3D_DAMAGE_IMAGE_DAMAGE
	u32 rule_words;            // 0: the destinations' rules stay
};

constexpr u32 kStateWords = 2u * kPT;             // a thread's words of one universe
constexpr u32 kParkWords = 2u * kStateWords + 3u; // S, T, orx[2] and the mask of touched planes
constexpr u32 kOrx = 2u * kStateWords, kMask = kOrx + 2u;

// a set's box as the record holds it: min and max as x | y << 8 | z << 16, both zero for an empty set (ca_envelope.hip's)
__device__ __forceinline__ uint2 box_of(const Extent &e)
{
	if (e.pop == 0u) return make_uint2(0u, 0u);
	const u64 xm = (u64)e.x1 << 32 | e.x0;
	return make_uint2((u32)__builtin_ctzll(xm) | (u32)__builtin_ctzll(e.ym) << 8 | (u32)__builtin_ctzll(e.zm) << 16,
	                  (63u - (u32)__builtin_clzll(xm)) | (63u - (u32)__builtin_clzll(e.ym)) << 8 | (63u - (u32)__builtin_clzll(e.zm)) << 16);
}

template <typename Step, bool InRegisters>
__device__ __forceinline__ void damage_run(const DamageArgs &a)
{
	constexpr u32 kParkBytes = InRegisters ? 0u : kParkWords * kThreads * 4u;
	constexpr u32 kSmallBytes = (2u * kPartWords + kWaves + 4u) * 4u;
	// ONE parity of the exchange where two do not fit beside the parked states (the header)
	constexpr bool kOneParity = Step::kXchWords * 4u + kParkBytes + kSmallBytes > 163840u;
	static_assert((kOneParity ? Step::kXchWords / 2u : Step::kXchWords) * 4u + kParkBytes + kSmallBytes <= 163840u, "a workgroup's LDS");
	__shared__ __attribute__((aligned(16))) u32 xch[kOneParity ? Step::kXchWords / 2u : Step::kXchWords];
	__shared__ __attribute__((aligned(16))) u32 park[InRegisters ? 4u : kParkWords * kThreads]; // [word][thread]
	__shared__ __attribute__((aligned(16))) u32 partD[kPartWords];
	__shared__ __attribute__((aligned(16))) u32 partX[kPartWords];
	__shared__ __attribute__((aligned(16))) u32 dpart[kWaves]; // a wave's share of d_t
	__shared__ uint4 stat[1];                                  // thread 0's alone: d_0, the largest d_t, the first t that reaches it, the sum

	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const u32 k = blockIdx.x, u = a.first + k;
	auto uniform = [](u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); };
	const u32 P = uniform(a.steps[k]); // workgroup-uniform, read once
	const u32 twin = uniform(a.twins[k]);
	u32 *const curve = a.curve ? a.curve + (size_t)k * a.curve_stride : nullptr;

	Step st;
	st.load(a.rules, u);
	u32 S[kPT][2], T[kPT][2]; // InRegisters: the two states; else what a step reads and the XOR compares
	load_universe(a.state + (size_t)u * kEnsembleWords, wave, row, S);
	load_universe(a.state + (size_t)(twin == CA3D_DAMAGE_SELF ? u : twin) * kEnsembleWords, wave, row, T);
#pragma unroll
	for (u32 i = 0; i < CA3D_DAMAGE_FLIPS; i++)
	{
		const u32 f = uniform(a.flips[k * CA3D_DAMAGE_FLIPS + i]); // x | y << 8 | z << 16, checked by the host
		const u32 fx = f & 0xFFu, fy = (f >> 8) & 0xFFu, fz = (f >> 16) & 0xFFu;
		const bool own = f != CA3D_DAMAGE_NO_FLIP && wave == (fz >> 2) && row == fy;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++) T[p][h] ^= own && p == (fz & 3u) && h == (fx >> 5) ? 1u << (fx & 31u) : 0u;
	}

	// D_0, and what is kept of every D_t: its popcount for the next sample, the OR of its words per x half, its planes
	u32 pc = 0, orx[2] = {0u, 0u}, touched = 0;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const u32 d0 = S[p][0] ^ T[p][0], d1 = S[p][1] ^ T[p][1];
		pc += (u32)__popc(d0) + (u32)__popc(d1);
		orx[0] |= d0;
		orx[1] |= d1;
		touched |= (d0 | d1) != 0u ? 1u << p : 0u;
		if (!InRegisters)
		{
			park[(2u * p) * kThreads + tid] = S[p][0];
			park[(2u * p + 1u) * kThreads + tid] = S[p][1];
			park[(kStateWords + 2u * p) * kThreads + tid] = T[p][0];
			park[(kStateWords + 2u * p + 1u) * kThreads + tid] = T[p][1];
		}
	}
	if (!InRegisters)
	{
		park[kOrx * kThreads + tid] = orx[0];
		park[(kOrx + 1u) * kThreads + tid] = orx[1];
		park[kMask * kThreads + tid] = touched;
	}

	// ONE loop over the step CALLS c = 0 .. 2 P - 1, so one text of the step: call 2 t steps S_t, call 2 t + 1 steps T_t. InRegisters:
	// the call steps S and leaves (S, T) <- (T, stepped S), so the pair is (S_t, T_t) in front of an even call and (T_t, S_t+1) in
	// front of an odd one; else the call steps park's state c & 1 in place.
	u32 c = 0;
#pragma nounroll
	for (; c < 2u * P; c++) // a workgroup-uniform bound
	{
		const u32 which = c & 1u, t = c >> 1;
		if (!which)
		{
			const u32 mine = wave_sum_uniform(pc);
			if (row == 0u) dpart[wave] = mine;
		}
		u32 *const parked = park + which * (kStateWords * kThreads) + tid;
		u32 N[kPT][2];
		if (!InRegisters)
		{
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
#pragma unroll
				for (u32 h = 0; h < 2u; h++) S[p][h] = parked[(2u * p + h) * kThreads];
		}
		st.step(S, N, xch, kOneParity ? 0u : which, wave, row); // its barrier is B1

		if (!which)
		{
			// (the lane's number, counted here upon a zero the compiler cannot see through: `row`, the lane's number taken outside the
			// loop or a plain zero would live across the steps in a register, and the Moore step has none to spare: it spills them)
			u32 zero = 0u;
			asm volatile("" : "+v"(zero));
			const u32 lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
			const u32 d = (u32)__builtin_amdgcn_readlane((int)row16_sum(dpart[lane & 15u]), 0); // d_t
			if (wave == 0u && lane == 0u) // thread 0
			{
				if (curve) curve[t + zero] = d;
				uint4 s = t ? *stat : make_uint4(d, 0u, 0u, 0u);
				if (d > s.y)
				{
					s.y = d;
					s.z = t;
				}
				s.w += d;
				*stat = s;
			}
			if (d == 0u) break; // healed: by all 1024 threads, S_t and T_t still where they were
		}
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				if (InRegisters)
				{
					S[p][h] = T[p][h];
					T[p][h] = N[p][h];
				}
				else parked[(2u * p + h) * kThreads] = N[p][h];
			}
		if (kOneParity) __syncthreads(); // B2

		if (which) // D_t+1: N is T_t+1
		{
			pc = 0;
			u32 o0 = 0, o1 = 0, planes = 0;
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const u32 d0 = (InRegisters ? S[p][0] : park[(2u * p) * kThreads + tid]) ^ N[p][0];
				const u32 d1 = (InRegisters ? S[p][1] : park[(2u * p + 1u) * kThreads + tid]) ^ N[p][1];
				pc += (u32)__popc(d0) + (u32)__popc(d1);
				o0 |= d0;
				o1 |= d1;
				planes |= (d0 | d1) != 0u ? 1u << p : 0u;
			}
			if (InRegisters)
			{
				orx[0] |= o0;
				orx[1] |= o1;
				touched |= planes;
			}
			else
			{
				park[kOrx * kThreads + tid] |= o0;
				park[(kOrx + 1u) * kThreads + tid] |= o1;
				park[kMask * kThreads + tid] |= planes;
			}
		}
	}
	// (the thread's index once more, from the lane's number: what the lines below derive from it is then formed here, not in front of the
	// loop and carried through it in registers the Moore step does not have)
	const u32 rowb = __lane_id(), tidb = wave * 64u + rowb;
	const u32 t = c >> 1;
	const bool left_early = t < P;                 // d_t == 0 inside the loop
	const u32 written = (left_early ? t : P) + 1u; // samples of the curve that are settled by now, d_P among them

	if (!InRegisters)
	{
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				S[p][h] = park[(2u * p + h) * kThreads + tidb];
				T[p][h] = park[(kStateWords + 2u * p + h) * kThreads + tidb];
			}
		orx[0] = park[kOrx * kThreads + tidb];
		orx[1] = park[(kOrx + 1u) * kThreads + tidb];
		touched = park[kMask * kThreads + tidb];
	}
	u32 D[kPT][2], X[kPT][2]; // D_P (S_t ^ T_t, empty, after an early exit) and the pseudo-image of the touched cells
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			D[p][h] = S[p][h] ^ T[p][h];
			X[p][h] = touched >> p & 1u ? orx[h] : 0u;
		}
	const Extent ed = extent(D, partD, wave, rowb);
	const Extent ex = extent(X, partX, wave, rowb);

	if (tidb == 0u)
	{
		const u32 healed_at = left_early ? t : ed.pop == 0u ? P : 0xFFFFFFFFu;
		uint4 s = *stat; // P >= 1: round 0 has written it
		if (!left_early)
		{
			// sample P, taken by extent
			if (curve) curve[P] = ed.pop;
			if (ed.pop > s.y)
			{
				s.y = ed.pop;
				s.z = P;
			}
			s.w += ed.pop;
		}
		const uint2 bd = box_of(ed), bx = box_of(ex);
		uint4 *rec = reinterpret_cast<uint4 *>(a.out + k);
		rec[0] = make_uint4(P, healed_at != 0xFFFFFFFFu ? (u32)CA3D_DAMAGE_HEALED : 0u, healed_at, ed.pop);
		rec[1] = s;
		rec[2] = make_uint4(bd.x, bd.y, bx.x, bx.y);
	}
	if (curve)
#pragma nounroll
		for (u32 i = written + tidb; i < a.curve_stride; i += kThreads) curve[i] = 0u;

	// ---- the image: D_P into both buffers of universe dst_first + k
	if (!a.image) return; // workgroup-uniform, and no barrier follows
	const u32 slot = a.dst_first + k;
	const size_t off = (size_t)slot * kEnsembleWords;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const size_t at = off + (size_t)((wave * kPT + p) * 64u + rowb) * 2u; // inside universe `slot` of the destination
		*reinterpret_cast<uint2 *>(a.dst_state + at) = make_uint2(D[p][0], D[p][1]);
		*reinterpret_cast<uint2 *>(a.dst_prev + at) = make_uint2(D[p][0], D[p][1]);
	}
	if (tidb == 0u)
	{
		const u32 *rs = a.rules + (size_t)u * Step::kRuleWords;
		u32 *rd = a.dst_rules + (size_t)slot * Step::kRuleWords;
#pragma nounroll
		for (u32 i = 0; i < a.rule_words; i++) rd[i] = rs[i]; // rule_words is 0 or Step::kRuleWords
	}
}

// a kind's kernels under the three boundaries; four waves per SIMD as in ca_ensemble.hip
#define CA3D_DAMAGE_KERNELS(kind, StepT, regs)                                                                                                            \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_damage_##kind##64(DamageArgs a) { damage_run<StepT<kBoundaryReference>, regs>(a); }        \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_damage_##kind##64_torus(DamageArgs a) { damage_run<StepT<kBoundaryTorus>, regs>(a); }      \
	__global__ __launch_bounds__(kThreads, 4) void ca_ensemble_damage_##kind##64_closed(DamageArgs a) { damage_run<StepT<kBoundaryClosed>, regs>(a); }
CA3D_DAMAGE_KERNELS(vn, VnStepT, true)
CA3D_DAMAGE_KERNELS(moore, MooreStepT, false)
CA3D_DAMAGE_KERNELS(clustered, ClusteredStepT, false)
#undef CA3D_DAMAGE_KERNELS

} // namespace

hipError_t launch_damage(const DamageLaunch &l, hipStream_t stream)
{
	const u32 kind = l.clustered ? 2u : l.neighbourhood == CA3D_ENSEMBLE_MOORE ? 1u : 0u;
	if (l.count == 0 || (l.clustered && l.neighbourhood != CA3D_ENSEMBLE_MOORE) || l.boundary < 0 || l.boundary > CA3D_ENSEMBLE_BOUNDARY_CLOSED) return hipErrorInvalidValue;
	if (!l.steps || !l.twins || !l.flips || !l.out) return hipErrorInvalidValue;
	if (l.image & ~CA3D_DAMAGE_IMAGE_DAMAGE) return hipErrorInvalidValue;
	if (l.image && (!l.dst_state || !l.dst_prev)) return hipErrorInvalidValue;
	if (l.rule_words && (!l.image || !l.dst_rules || l.rule_words != ensemble_rule_words(l.neighbourhood, l.clustered))) return hipErrorInvalidValue;
	static_assert(sizeof(ca3d_damage) == 48, "a record is three 16-byte stores");
	DamageArgs a;
	a.state = l.state;
	a.rules = l.rules;
	a.steps = l.steps;
	a.twins = l.twins;
	a.flips = l.flips;
	a.out = l.out;
	a.curve = l.curve;
	a.curve_stride = l.curve_stride;
	a.dst_state = l.dst_state;
	a.dst_prev = l.dst_prev;
	a.dst_rules = l.dst_rules;
	a.first = l.first;
	a.dst_first = l.dst_first;
	a.image = l.image;
	a.rule_words = l.rule_words;
	typedef void (*Kernel)(DamageArgs);
	static const Kernel kernels[3][3] = {{ca_ensemble_damage_vn64, ca_ensemble_damage_vn64_torus, ca_ensemble_damage_vn64_closed},
	                                     {ca_ensemble_damage_moore64, ca_ensemble_damage_moore64_torus, ca_ensemble_damage_moore64_closed},
	                                     {ca_ensemble_damage_clustered64, ca_ensemble_damage_clustered64_torus, ca_ensemble_damage_clustered64_closed}};
	hipLaunchKernelGGL(kernels[kind][l.boundary], dim3(l.count), dim3(kThreads), 0, stream, a);
	return hipGetLastError();
}

} // namespace ca3d
