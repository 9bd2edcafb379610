// The body of every ensemble kernel: EnsembleArgs, what a launch is told, and ensemble_run<Step, Cycle, Trace, Moving>, the launch of one
// universe whatever its step (ca_ensemble.hip's head says what it does). Shared by ca_ensemble.hip, the kernels of the reference
// boundary, and ca_ensemble_boundary.hip, those of the torus and the closed cube: the two units hold the same text and differ in the
// Step they hand it. Nothing here knows a boundary: a check point looks at the words a thread holds, the record at the cells that live.
// Device code only; include inside namespace ca3d { namespace { ... } }, after ca3d_internal.h, ca_bitops.inc, ca_wave_ops.inc and
// ca_digest.h.
#pragma once

typedef unsigned long long u64;

constexpr u32 kThreads = 1024, kWaves = 16, kPT = 4; // threads, waves, planes per wave

struct EnsembleArgs
{
	u32 *state, *prev;
	const u32 *rules;
	ca3d_summary *records;
	u32 *steps_done, *reason;
	u32 first, steps, base;
	u32 check_every, first_check, stop_mask; // first_check: steps of this launch before the call's next check point (0: on entry)
	u32 final, reset;
	// the *_cycle kernels only (ca3d_ensemble_step_until_cycle); appended, so that the kernels above read what they always read
	u32 *anchor;    // [B][8192]: the state at the universe's anchor check point
	u32 *cycle;     // [B][4]: anchor step, anchor hash, period, unused — next to steps_done / reason. The *_moving kernels: [B][8], + packed
	                // shift, + the anchor's population, packed box_min, packed box_max (kMeta* below)
	u32 next_check; // number j of the call's next regular check point (the one first_check steps into this launch)
	// the *_trace kernels only (ca3d_ensemble_step_until_trace); appended likewise
	u32 *samples;      // [B][sample_stride][3]: population, births, deaths at check point j of the call
	u32 sample_stride; // samples of one universe: the call's K = ceil(max_steps / check_every) + 1
};

#include "ca_ensemble_step.inc"

// The cycle filter's hash of one word: a sum of these over a universe's words is equal for equal states, so a mismatch proves a
// difference. 32 bits, one multiply a word (digest_mix's 64-bit multiplies would cost more than a von Neumann step).
__device__ __forceinline__ u32 cycle_mix(u32 idx, u32 w)
{
	// (the word's upper half is folded into its lower half first: a product only carries upwards, and without the fold two words that differ
	// from zero in bit 31 alone cancel in the sum — an and-rounds fill dying out did exactly that one step before it was empty)
	const u32 x = (w ^ (w >> 16) ^ (idx * 0x9E3779B1u)) * 0x85EBCA6Bu;
	return x ^ (x >> 15);
}

// The *_moving kernels (CA3D_STOP_MOVING): a bounding box travels as two words, x | y << 8 | z << 16 of box_min and of box_max. Inside
// means clear of every face: a pattern on a - face sees the dead boundary, one on a + face wraps. The definition is the same under
// every boundary (include/ca3d.h): in a torus a ship that crossed a seam between anchor and check is compared as if it had not, and its
// shift comes out congruent to the true displacement modulo 64 per axis.
__device__ __forceinline__ bool box_inside(u32 mn, u32 mx)
{
	bool ok = true;
#pragma unroll
	for (u32 i = 0; i < 3u; i++) ok = ok && ((mn >> (8u * i)) & 0xFFu) >= 1u && ((mx >> (8u * i)) & 0xFFu) <= 62u;
	return ok;
}
// the *_moving kernels' chk, in words: the four per-wave words of the *_cycle kernels (flags, hash, "differs from the anchor", "differs
// from the shifted anchor"), the per-wave partials of a check point (8 words a wave: population, x-occupancy words 0 and 1, y ballot low
// and high, z bits low and high — the wave's four planes in place —, unused), the anchor's record (8 words, one copy per wave)
constexpr u32 kMovDiff = 3u * kWaves, kMovPart = 4u * kWaves, kMovCyc = 12u * kWaves, kMovWords = 20u * kWaves;
// the anchor's record, in chk and in EnsembleArgs::cycle
constexpr u32 kMetaStep = 0, kMetaHash = 1, kMetaPeriod = 2, kMetaShift = 3, kMetaPop = 4, kMetaMin = 5, kMetaMax = 6;

// The launch of one universe, whatever its step. Cycle: CA3D_STOP_PERIODIC is watched too (include/ca3d.h, ca3d_ensemble_step_until_cycle).
// Every universe keeps ONE anchor — the state at an earlier check point of the call, moved at check points 0, 1, 2, 4, 8 ... (Brent) — in
// a third per-universe buffer: a thread stores and later loads exactly the eight words it owns, so nobody reads what another thread
// wrote. At a check point the threads hash their words, the per-wave sums ride the chk exchange and its barrier, and only when the
// universe's hash equals the anchor's (held wave-uniform) are the anchor's words loaded and compared: one more reduction and barrier,
// and the only way PERIODIC is ever declared.
// Trace: every check point is reached whatever the stop mask, and leaves one sample — population, births, deaths of the state in the
// registers against the one a step earlier — in samples[u][j] (include/ca3d.h, ca3d_ensemble_step_until_trace). The per-thread counts
// are reduced over the wave, ride the chk exchange and its barrier as the hash does, and thread 0 sums the 16 partials and stores the
// three words. Births and deaths travel as ONE word, births | deaths << 16: a wave's 512 words hold 16 384 of each at most. The number j
// is worked out at the check point from base, t and check_every (read from the kernel's arguments there and then).
// Moving (with Cycle): CA3D_STOP_MOVING is watched as well (include/ca3d.h, ca3d_ensemble_step_until_moving). look() also reduces the
// population and the bounding box of the state — per-wave partials in chk behind the check's own barrier, joined by every wave for
// itself, wave-uniform — and the anchor's population and box are kept beside its step and hash. Equal populations, equal box extents,
// both boxes clear of the faces and a displacement d != 0 of box_min start the comparison with the anchor SHIFTED by d: a thread loads
// the anchor's row (y - dy, z - dz) for each of its four planes (a row outside the universe is zero and is not loaded), shifts the 64
// bits by dx and compares with its own two words. As both boxes are clear of the faces no live bit is shifted out: the comparison is
// exact, and only it declares MOVING.
template <typename Step, bool Cycle, bool Trace, bool Moving = false>
__device__ __forceinline__ void ensemble_run(const EnsembleArgs &a)
{
	__shared__ __attribute__((aligned(16))) u32 xch[Step::kXchWords];
	// per wave: bit 0 a cell is alive, bit 1 a cell changed in the last step; Cycle: + the wave's hash sum, + "differs from the anchor";
	// Trace: + the wave's population, + its births | deaths << 16
	// Cycle, behind those (one array, so that nothing moves in the kernels without it): the anchor's step and hash and the period found,
	// one copy PER WAVE (written by its lane 0, read by the wave itself: LDS order within a wave, no barrier) — in LDS, because the
	// Moore step has no scalar registers to spare across the steps either
	// Moving: laid out as kMovDiff .. kMovWords say
	__shared__ __attribute__((aligned(16))) u32 chk[Moving ? kMovWords : Cycle ? 7u * kWaves : Trace ? 3u * kWaves : kWaves];
	u32(*cyc)[Moving ? 8 : 4] = reinterpret_cast<u32(*)[Moving ? 8 : 4]>(chk + (Moving ? kMovCyc : Cycle ? 3u * kWaves : 0u));
	__shared__ u64 red64[kWaves][2];
	__shared__ u32 red32[kWaves][6];
	const u32 u = a.first + blockIdx.x;
	const u32 tid = threadIdx.x, row = tid & 63u;
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	if (a.stop_mask && a.reason[u]) return; // stopped in an earlier launch of the same call

	Step step;
	step.load(a.rules, u);

	u32 *mine = a.state + (size_t)u * kEnsembleWords;
	// Two register sets that change roles every step: the one a step reads still holds the state one step earlier afterwards,
	// which is what a check and the summary compare with — no copies.
	u32 ra[kPT][2], rb[kPT][2];
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const uint2 v = *reinterpret_cast<const uint2 *>(mine + ((size_t)((wave * kPT + p) * 64u + row)) * 2u);
		ra[p][0] = v.x; ra[p][1] = v.y;
		rb[p][0] = 0u; rb[p][1] = 0u;
	}
	const ca3d_summary *rec = a.records + u;
	const u64 step0 = Cycle || Trace ? 0ull : a.reset ? 0ull : rec->step; // (Cycle, Trace: read where it is used, by the thread that then rewrites the record)

	u32 t = 0, fired = 0, until = a.first_check;
	u32 jn = 0; // Cycle: the number of the next regular check point
	// Cycle, Trace: what only a check point needs is read from the kernel's arguments there and then, not held across the steps
	const volatile EnsembleArgs *ka = Cycle || Trace ? (const volatile EnsembleArgs *)__builtin_amdgcn_kernarg_segment_ptr() : nullptr;
	// The index of the thread's first word in the universe's array, worked out again at every check point: nothing of a check (indices,
	// their products, addresses) may stay in registers across the steps, where the Moore step has none to spare
	auto own = [&]() __attribute__((always_inline)) -> u32 {
		u32 r = row, w = wave;
		asm volatile("" : "+v"(r), "+s"(w));
		return (w * kPT * 64u + r) * 2u;
	};
	if (Cycle)
	{
		jn = a.next_check;
		if (row == 0u)
		{
			// the anchor the launch before left (the call's first launch sets it on entry)
			cyc[wave][0] = a.base ? a.cycle[(Moving ? 8u : 4u) * u] : 0u;
			cyc[wave][1] = a.base ? a.cycle[(Moving ? 8u : 4u) * u + 1u] : 0u;
			cyc[wave][2] = 0u;
			if (Moving)
			{
				cyc[wave][kMetaShift] = 0u;
#pragma unroll
				for (u32 i = kMetaPop; i <= kMetaMax; i++) cyc[wave][i] = a.base ? a.cycle[8u * u + i] : 0u;
			}
		}
	}
	// One round of the loop: the check that is due on the state in `s` (previous state in `o`), then one step from `s` into `o`.
	// Returns true when the launch is over for this universe, the state in `s` and the one before it in `o`.
	auto round = [&](const u32 (&s)[kPT][2], u32 (&o)[kPT][2]) __attribute__((always_inline)) -> bool {
		if ((Trace || a.stop_mask) && (until == 0u || (t == a.steps && a.final)))
		{
			bool alive, changed, has_prev;
			u32 hash = 0; // Cycle: of the state in `s`
			u32 cpop = 0, cmin = 0, cmax = 0; // Moving: its population and packed box (box_inside)
			// the workgroup's two bits (and hash) of the state in `s` against `o`
			auto look = [&]() __attribute__((always_inline)) -> u32 {
				u32 al = 0, ch = 0, hs = 0;
				const u32 first = Cycle ? own() : 0u;
#pragma unroll
				for (u32 p = 0; p < kPT; p++)
#pragma unroll
					for (u32 h = 0; h < 2u; h++)
					{
						al |= s[p][h];
						ch |= s[p][h] ^ o[p][h];
						if (Cycle) hs += cycle_mix(first + p * 128u + h, s[p][h]); // the word's index in the universe's array
					}
				const u32 f = (__ballot(al != 0u) ? 1u : 0u) | (__ballot(ch != 0u) ? 2u : 0u);
				if (Cycle) hs = wave_add(hs);
				// (chk is rewritten at the next check at the earliest: a step — and its barrier — lies in between)
				if (row == 0u)
				{
					chk[wave] = f;
					if (Cycle) chk[kWaves + wave] = hs;
				}
				if (Trace)
				{
					u32 pop = 0, bd = 0; // the thread's population; its births | deaths << 16 (256 of each at most)
#pragma unroll
					for (u32 p = 0; p < kPT; p++)
#pragma unroll
						for (u32 h = 0; h < 2u; h++)
						{
							pop += (u32)__popc(s[p][h]);
							bd += (u32)__popc(s[p][h] & ~o[p][h]) + ((u32)__popc(o[p][h] & ~s[p][h]) << 16);
						}
					pop = wave_sum_uniform(pop);
					bd = wave_sum_uniform(bd);
					if (row == 0u) { chk[kWaves + wave] = pop; chk[2u * kWaves + wave] = bd; }
				}
				if (Moving)
				{
					u32 pop = 0, x0 = 0, x1 = 0, zb = 0;
#pragma unroll
					for (u32 p = 0; p < kPT; p++)
					{
						pop += (u32)__popc(s[p][0]) + (u32)__popc(s[p][1]);
						x0 |= s[p][0];
						x1 |= s[p][1];
						if (__ballot((s[p][0] | s[p][1]) != 0u)) zb |= 1u << p;
					}
					const u64 ym = __ballot((x0 | x1) != 0u); // bit y: row y of one of the wave's planes holds a live cell
					pop = wave_sum_uniform(pop);
					x0 = wave_or_uniform(x0);
					x1 = wave_or_uniform(x1);
					if (row == 0u)
					{
						u32 w = wave;
						asm volatile("" : "+s"(w)); // (worked out here, not held across the steps: see own())
						const u64 zm = (u64)zb << (w * kPT);
						uint4 *part = reinterpret_cast<uint4 *>(chk + kMovPart) + 2u * w;
						part[0] = make_uint4(pop, x0, x1, (u32)ym);
						part[1] = make_uint4((u32)(ym >> 32), (u32)zm, (u32)(zm >> 32), 0u);
					}
				}
				__syncthreads();
				if (Moving)
				{
					// every wave joins the 16 partials for itself: lanes 0 .. 15 of every row of 16 take one wave's each, four DPP steps
					// leave the row's lanes with the whole, lane 0 is read
					u32 r = row;
					asm volatile("" : "+v"(r));
					const uint4 *part = reinterpret_cast<const uint4 *>(chk + kMovPart) + 2u * (r & 15u);
					const uint4 pa = part[0], pb = part[1];
					auto first = [](u32 v) { return (u32)__builtin_amdgcn_readlane((int)v, 0); };
					cpop = first(row16_sum(pa.x));
					const u32 x0 = first(row16_or(pa.y)), x1 = first(row16_or(pa.z));
					const u64 ym = (u64)first(row16_or(pb.x)) << 32 | first(row16_or(pa.w));
					const u64 zm = (u64)first(row16_or(pb.z)) << 32 | first(row16_or(pb.y));
					if (cpop)
					{
						cmin = (x0 ? (u32)__builtin_ctz(x0) : 32u + (u32)__builtin_ctz(x1)) | (u32)__builtin_ctzll(ym) << 8 | (u32)__builtin_ctzll(zm) << 16;
						cmax = (x1 ? 63u - (u32)__builtin_clz(x1) : 31u - (u32)__builtin_clz(x0)) | (63u - (u32)__builtin_clzll(ym)) << 8 |
						       (63u - (u32)__builtin_clzll(zm)) << 16;
					}
				}
				const uint4 *c4 = reinterpret_cast<const uint4 *>(chk);
				uint4 m = c4[0];
#pragma unroll
				for (int i = 1; i < (int)kWaves / 4; i++) { const uint4 n = c4[i]; m.x |= n.x; m.y |= n.y; m.z |= n.z; m.w |= n.w; }
				if (Cycle)
				{
					uint4 hsum = c4[kWaves / 4];
#pragma unroll
					for (int i = 1; i < (int)kWaves / 4; i++) { const uint4 n = c4[kWaves / 4 + i]; hsum.x += n.x; hsum.y += n.y; hsum.z += n.z; hsum.w += n.w; }
					hash = (u32)__builtin_amdgcn_readfirstlane((int)(hsum.x + hsum.y + hsum.z + hsum.w));
				}
				return (u32)__builtin_amdgcn_readfirstlane((int)(m.x | m.y | m.z | m.w));
			};
			if (t == 0u)
			{
				// nothing stepped in this launch yet: the record describes the state
				alive = rec->population != 0ull;
				has_prev = !a.reset && rec->has_previous != 0u;
				changed = rec->births + rec->deaths != 0ull;
				if (Cycle) (void)look(); // ... the hash comes from the registers just loaded
				// Trace: sample 0 is the record as it stands, on the call's first launch only — a check point that ended the launch
				// before has been sampled there, from the registers
				if (Trace && wave == 0u && row == 0u && ka->base == 0u)
				{
					u32 *out = ka->samples + (size_t)(a.first + blockIdx.x) * ka->sample_stride * 3u; // (not `u`: nothing new held across the steps)
					out[0] = (u32)rec->population;
					out[1] = (u32)rec->births;
					out[2] = (u32)rec->deaths;
				}
			}
			else
			{
				const u32 all = look();
				// Trace: the partials look() left behind its barrier become the sample (chk is rewritten after the next step's barrier at the earliest)
				if (Trace && wave == 0u)
				{
					// Lanes 0 .. 15 of wave 0 take one wave's partials each (every row of 16 lanes does, so that the DPP sums below are over
					// whole rows) and lane 0 stores the sample. Births or deaths of a universe do not fit 16 bits: unpacked before they are summed.
					u32 r = row;
					asm volatile("" : "+v"(r)); // (worked out here, not held across the steps: see own())
					const u32 pw = chk[kWaves + (r & 15u)], bw = chk[2u * kWaves + (r & 15u)];
					const u32 ps = row16_sum(pw), bs = row16_sum(bw & 0xFFFFu), ds = row16_sum(bw >> 16);
					if (r == 0u)
					{
						// check point number j of the call: a regular one, or the last one at max_steps between two regular ones
						// (j <= ceil(max_steps / check_every) = sample_stride - 1: launch_ensemble refuses a launch that could pass it)
						const u32 k = ka->base + t, every = ka->check_every;
						const u32 j = k / every + (k % every ? 1u : 0u);
						u32 *out = ka->samples + ((size_t)(a.first + blockIdx.x) * ka->sample_stride + j) * 3u;
						out[0] = ps;
						out[1] = bs;
						out[2] = ds;
					}
				}
				alive = (all & 1u) != 0u;
				changed = (all & 2u) != 0u;
				has_prev = true;
			}
			fired = ((alive ? 0u : (u32)CA3D_STOP_EXTINCT) | (has_prev && !changed ? (u32)CA3D_STOP_STILL : 0u)) & a.stop_mask;
			u32 j = 0;
			if (Cycle)
			{
				// check point number j of the call: a regular one, or the last one at max_steps between two regular ones. A check point that
				// ended the launch before and is looked at again on entry of this one has the same number and (k == astep) is not compared
				// with itself when the anchor moved there.
				const u32 k = ka->base + t;
				j = jn;
				if (until == 0u) jn++;
				const uint2 av = *reinterpret_cast<const uint2 *>(cyc[wave]);
				const u32 astep = (u32)__builtin_amdgcn_readfirstlane((int)av.x), ahash = (u32)__builtin_amdgcn_readfirstlane((int)av.y);
				if (j != 0u && k != astep && hash == ahash)
				{
					u32 diff = 0;
					const u32 *anchor = ka->anchor + (size_t)u * kEnsembleWords + own();
#pragma unroll
					for (u32 p = 0; p < kPT; p++)
					{
						const uint2 v = *reinterpret_cast<const uint2 *>(anchor + p * 128u);
						diff |= (v.x ^ s[p][0]) | (v.y ^ s[p][1]);
					}
					// every lane votes: the ballot is taken BEFORE the branch that leaves lane 0 alone
					const u32 differs = __ballot(diff != 0u) ? 1u : 0u;
					// (the third part of chk is written here only: a step's barrier, or the record's, lies before the next time)
					if (row == 0u) chk[2u * kWaves + wave] = differs;
					__syncthreads();
					const uint4 *d4 = reinterpret_cast<const uint4 *>(chk) + 2u * kWaves / 4u;
					uint4 m = d4[0];
#pragma unroll
					for (int i = 1; i < (int)kWaves / 4; i++) { const uint4 n = d4[i]; m.x |= n.x; m.y |= n.y; m.z |= n.z; m.w |= n.w; }
					if (__builtin_amdgcn_readfirstlane((int)(m.x | m.y | m.z | m.w)) == 0 && (a.stop_mask & (u32)CA3D_STOP_PERIODIC))
					{
						fired |= (u32)CA3D_STOP_PERIODIC;
						if (row == 0u) cyc[wave][2] = k - astep;
					}
				}
				if (Moving)
				{
					const uint4 am = *reinterpret_cast<const uint4 *>(cyc[wave] + kMetaPop);
					const u32 apop = (u32)__builtin_amdgcn_readfirstlane((int)am.x), amin = (u32)__builtin_amdgcn_readfirstlane((int)am.y),
					          amax = (u32)__builtin_amdgcn_readfirstlane((int)am.z);
					// the filter: nothing below runs unless the two states could be translates of each other, clear of the faces, d != 0
					if (j != 0u && k != astep && (a.stop_mask & (u32)CA3D_STOP_MOVING) && cpop != 0u && cpop == apop && cmin != amin && cmax - cmin == amax - amin &&
					    box_inside(cmin, cmax) && box_inside(amin, amax))
					{
						const int dx = (int)(cmin & 0xFFu) - (int)(amin & 0xFFu), dy = (int)((cmin >> 8) & 0xFFu) - (int)((amin >> 8) & 0xFFu),
						          dz = (int)(cmin >> 16) - (int)(amin >> 16);
						u32 r = row, w = wave;
						asm volatile("" : "+v"(r), "+s"(w));
						const u32 *anchor = ka->anchor + (size_t)u * kEnsembleWords;
						const u32 sy = r - (u32)dy; // the anchor's row that lands on this one; outside 0 .. 63: nothing does
						u32 diff = 0;
#pragma unroll
						for (u32 p = 0; p < kPT; p++)
						{
							const u32 sz = w * kPT + p - (u32)dz;
							uint2 v = make_uint2(0u, 0u);
							if (sy < 64u && sz < 64u) v = *reinterpret_cast<const uint2 *>(anchor + (sz * 64u + sy) * 2u); // inside the universe's 8192 words
							u64 from = (u64)v.y << 32 | v.x;
							from = dx >= 0 ? from << dx : from >> -dx; // |dx| <= 61
							diff |= ((u32)from ^ s[p][0]) | ((u32)(from >> 32) ^ s[p][1]);
						}
						// every lane votes: the ballot is taken BEFORE the branch that leaves lane 0 alone
						const u32 differs = __ballot(diff != 0u) ? 1u : 0u;
						// (a part of chk written here only: a step's barrier, or the record's, lies before the next time)
						if (row == 0u) chk[kMovDiff + wave] = differs;
						__syncthreads();
						const uint4 *d4 = reinterpret_cast<const uint4 *>(chk) + kMovDiff / 4u;
						uint4 m = d4[0];
#pragma unroll
						for (int i = 1; i < (int)kWaves / 4; i++) { const uint4 n = d4[i]; m.x |= n.x; m.y |= n.y; m.z |= n.z; m.w |= n.w; }
						if (__builtin_amdgcn_readfirstlane((int)(m.x | m.y | m.z | m.w)) == 0)
						{
							fired |= (u32)CA3D_STOP_MOVING;
							if (row == 0u)
							{
								cyc[wave][kMetaPeriod] = k - astep;
								cyc[wave][kMetaShift] = ((u32)dx & 0xFFu) | ((u32)dy & 0xFFu) << 8 | ((u32)dz & 0xFFu) << 16; // signed bytes
							}
						}
					}
				}
			}
			if (fired) return true;
			if (Cycle && (j & (j - 1u)) == 0u) // check points 0, 1, 2, 4, 8 ...: the anchor moves here, AFTER the comparison
			{
				u32 *anchor = ka->anchor + (size_t)u * kEnsembleWords + own();
#pragma unroll
				for (u32 p = 0; p < kPT; p++) *reinterpret_cast<uint2 *>(anchor + p * 128u) = make_uint2(s[p][0], s[p][1]);
				if (row == 0u) *reinterpret_cast<uint2 *>(cyc[wave]) = make_uint2(ka->base + t, hash);
				if (Moving && row == 0u) *reinterpret_cast<uint4 *>(cyc[wave] + kMetaPop) = make_uint4(cpop, cmin, cmax, 0u);
			}
			until = a.check_every;
		}
		if (t == a.steps) return true;

		step.step(s, o, xch, t & 1u, wave, row);
		t++;
		until--;
		return false;
	};
	u32 s[kPT][2], q[kPT][2]; // when the loop is over: the state; the state one step earlier
	auto leave = [&](const u32 (&cur)[kPT][2], const u32 (&old)[kPT][2]) __attribute__((always_inline)) {
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++) { s[p][h] = cur[p][h]; q[p][h] = old[p][h]; }
	};
	for (;;)
	{
		if (round(ra, rb)) { leave(ra, rb); break; }
		if (round(rb, ra)) { leave(rb, ra); break; }
	}

	if (a.stop_mask && tid == 0u)
	{
		a.steps_done[u] = a.base + t;
		a.reason[u] = fired;
		if (Cycle)
		{
			u32 *out = ka->cycle + (Moving ? 8u : 4u) * u; // (thread 0 reads what it wrote itself)
			out[0] = cyc[0][0];
			out[1] = cyc[0][1];
			out[2] = cyc[0][2];
			if (Moving)
			{
#pragma unroll
				for (u32 i = kMetaShift; i <= kMetaMax; i++) out[i] = cyc[0][i];
			}
		}
	}
	if (t == 0u && !a.reset) return; // nothing moved: state and record stand

	// ---- the record, from the registers
	const bool hp = t != 0u;
	u32 pop = 0, births = 0, deaths = 0, o0 = 0, o1 = 0, zbits = 0;
	u64 dig = 0;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			const u32 w = s[p][h], was = q[p][h];
			pop += (u32)__popc(w);
			if (hp)
			{
				births += (u32)__popc(w & ~was);
				deaths += (u32)__popc(was & ~w);
			}
			// digest index = the word's index in the universe's own 64^3 array
			if (w) dig += digest_mix((u64)(((wave * kPT + p) * 64u + row) * 2u + h), w);
		}
		o0 |= s[p][0];
		o1 |= s[p][1];
		if (__ballot((s[p][0] | s[p][1]) != 0u)) zbits |= 1u << p;
	}
	const u64 ymask = __ballot((o0 | o1) != 0u); // bit y: row y of one of the wave's planes holds a live cell
	pop = wave_add(pop); births = wave_add(births); deaths = wave_add(deaths); dig = wave_add(dig);
	o0 = wave_or(o0); o1 = wave_or(o1);
	__syncthreads(); // (a check may have read chk just now; the arrays below are separate, this orders the launch's last LDS traffic all the same)
	if (row == 0u)
	{
		red64[wave][0] = dig; red64[wave][1] = ymask;
		red32[wave][0] = pop; red32[wave][1] = births; red32[wave][2] = deaths;
		red32[wave][3] = o0; red32[wave][4] = o1; red32[wave][5] = zbits;
	}
	__syncthreads();
	if (tid == 0u)
	{
		u64 d = 0, ym = 0, zm = 0;
		u32 r[5] = {0, 0, 0, 0, 0};
#pragma nounroll
		for (u32 w = 0; w < kWaves; w++)
		{
			d += red64[w][0];
			ym |= red64[w][1];
			zm |= (u64)red32[w][5] << (w * kPT);
			for (int i = 0; i < 3; i++) r[i] += red32[w][i];
			r[3] |= red32[w][3];
			r[4] |= red32[w][4];
		}
		ca3d_summary o;
		o.step = (Cycle || Trace ? (a.reset ? 0ull : a.records[u].step) : step0) + t;
		o.population = r[0];
		o.births = r[1];
		o.deaths = r[2];
		o.digest = d;
		o.has_previous = hp ? 1u : 0u;
		if (r[0])
		{
			o.box_min[0] = r[3] ? (u32)__builtin_ctz(r[3]) : 32u + (u32)__builtin_ctz(r[4]);
			o.box_max[0] = r[4] ? 63u - (u32)__builtin_clz(r[4]) : 31u - (u32)__builtin_clz(r[3]);
			o.box_min[1] = (u32)__builtin_ctzll(ym);
			o.box_max[1] = 63u - (u32)__builtin_clzll(ym);
			o.box_min[2] = (u32)__builtin_ctzll(zm);
			o.box_max[2] = 63u - (u32)__builtin_clzll(zm);
		}
		else
		{
			for (int i = 0; i < 3; i++) { o.box_min[i] = 64u; o.box_max[i] = 0u; }
		}
		a.records[u] = o;
	}
	if (!hp) return; // a record rebuilt after an upload: the state is where the host put it

	// every word of the universe was read into registers before the first barrier: writing in place is safe
	u32 *old = a.prev + (size_t)u * kEnsembleWords;
#pragma unroll
	for (u32 p = 0; p < kPT; p++)
	{
		const size_t i = Cycle || Trace ? (size_t)own() + p * 128u : ((size_t)((wave * kPT + p) * 64u + row)) * 2u; // (Cycle, Trace: as at the check points)
		*reinterpret_cast<uint2 *>(mine + i) = make_uint2(s[p][0], s[p][1]);
		*reinterpret_cast<uint2 *>(old + i) = make_uint2(q[p][0], q[p][1]);
	}
}

