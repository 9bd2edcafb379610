// The step policies of the ensemble kernels: one step of a 64^3 universe held in eight registers a thread (lane = row y, wave w = planes
// 4 w .. 4 w + 3, a row's two words in one thread), with the rule as data. A policy (VnStep, MooreStep, ClusteredStep) owns the rule's
// registers (`load`), the words of a universe's rule (`kRuleWords`, checked against the host's ensemble_rule_words()), the size of its
// LDS exchange (`kXchWords`, two step parities) and one step (`step`, ONE barrier, reached by all 1024 threads). Shared by ca_ensemble.hip
// and ca_ensemble_boundary.hip (through ca_ensemble_run.inc), ca_canon_period.hip and ca_envelope.hip. Device code only; include inside
// namespace ca3d { namespace { ... } }, after ca3d_internal.h and ca_bitops.inc, with u32, kWaves and kPT defined.
//
// A policy is a template over the universe's BOUNDARY (include/ca3d.h, ca3d_ensemble_set_boundary), which sits in three places of a step:
// the operand that enters a row's end word (x), the DPP control that brings the neighbouring row (y), the exchange slot that brings the
// neighbouring wave's plane (z). Faces<B> below is all of it; VnStep, MooreStep and ClusteredStep are the kBoundaryReference forms.
#pragma once

constexpr int kBoundaryReference = 0, kBoundaryTorus = 1, kBoundaryClosed = 2; // = CA3D_ENSEMBLE_BOUNDARY_*

template <int B>
struct Faces
{
	static_assert(B == kBoundaryReference || B == kBoundaryTorus || B == kBoundaryClosed, "unknown boundary");
	static constexpr bool kMinusWraps = B == kBoundaryTorus, kPlusWraps = B != kBoundaryClosed; // reference: - faces dead, + faces wrap
	// cell x - 1 of word h of a row (`other`: the row's other word): word 1's comes from word 0, word 0's from word 1 (x == -1 wraps) or
	// from nowhere (dead)
	static __device__ __forceinline__ u32 left(u32 w, u32 other, u32 h)
	{
		if constexpr (kMinusWraps) return from_left(w, other);
		else return from_left(w, h ? other : 0u);
	}
	// cell x + 1: word 0's comes from word 1, word 1's from word 0 (x == 64 wraps) or from nowhere
	static __device__ __forceinline__ u32 right(u32 w, u32 other, u32 h)
	{
		if constexpr (kPlusWraps) return from_right(other, w);
		else return from_right(h ? 0u : other, w);
	}
	// row y - 1 (row 63, or zero, into row 0) and row y + 1 (row 0, or zero, into row 63)
	static __device__ __forceinline__ u32 row_below(u32 v) { return dpp_mov<kMinusWraps ? kDppWaveRor1 : kDppWaveShr1>(v); }
	static __device__ __forceinline__ u32 row_above(u32 v) { return dpp_mov<kPlusWraps ? kDppWaveRol1 : kDppWaveShl1>(v); }
	// whether a wave's plane z - 1 / z + 1 exists (else it is dead), and the wave whose last / first plane it then is. Ask first: without
	// a plane below the answer is no wave of the 16, and a slot of it lies outside the exchange (the wave above is always one of them)
	static __device__ __forceinline__ bool has_below(u32 wave) { return kMinusWraps || wave; }
	static __device__ __forceinline__ bool has_above(u32 wave) { return kPlusWraps || wave + 1u < kWaves; }
	static __device__ __forceinline__ u32 wave_below(u32 wave)
	{
		if constexpr (kMinusWraps) return (wave - 1u) & (kWaves - 1u);
		else return wave - 1u;
	}
	static __device__ __forceinline__ u32 wave_above(u32 wave) { return (wave + 1u) & (kWaves - 1u); }
};

__device__ __forceinline__ u32 mux(u32 sel, u32 one, u32 zero) { return next_state(sel, one, zero); } // sel ? one : zero, bit by bit

// ---- von Neumann: the table pair in one word, lut_s | lut_b << 8 (7 bits each)
template <int B>
struct VnStepT
{
	static constexpr u32 kXchWords = 2u * kWaves * 2u * 2u * 64u; // [step parity][wave][first / last plane][word][row]: 32 KiB
	static constexpr u32 kRuleWords = 1u; // a universe's rule in the ensemble's rule array, as `load` indexes it
	static_assert(kRuleWords == ensemble_rule_words(CA3D_ENSEMBLE_VON_NEUMANN), "the host's rule array and the policy agree");
	// leaf[c] = all-ones where a DEAD cell with c live neighbours is born, leaf[7 + c] where a LIVE one survives
	u32 leaf[14];

	__device__ __forceinline__ void load(const u32 *rules, u32 u)
	{
		const u32 lut = rules[u];
#pragma unroll
		for (int c = 0; c < 7; c++)
		{
			leaf[c] = 0u - ((lut >> (8 + c)) & 1u);
			leaf[7 + c] = 0u - ((lut >> c) & 1u);
			asm volatile("" : "+v"(leaf[c]));     // in vector registers for the whole launch: a select reads one other operand at most
			asm volatile("" : "+v"(leaf[7 + c]));
		}
	}
	__device__ __forceinline__ u32 rule(u32 w, u32 l, u32 r, u32 ym, u32 yp, u32 below, u32 above) const
	{
		u32 p[3];
		sum6(l, r, ym, yp, below, above, p);
		u32 t[7];
#pragma unroll
		for (int c = 0; c < 7; c++) t[c] = mux(w, leaf[7 + c], leaf[c]);
		const u32 q0 = mux(p[0], t[1], t[0]), q1 = mux(p[0], t[3], t[2]), q2 = mux(p[0], t[5], t[4]);
		return mux(p[2], mux(p[1], t[6], q2), mux(p[1], q1, q0));
	}
	static __device__ __forceinline__ u32 slot(u32 buf, u32 w, u32 which, u32 h, u32 row) { return (((buf * kWaves + w) * 2u + which) * 2u + h) * 64u + row; }

	// one step from `s` into `o` (resident64_run's, with the rule as data); buf: the step's parity
	__device__ __forceinline__ void step(const u32 (&s)[kPT][2], u32 (&o)[kPT][2], u32 *xch, u32 buf, u32 wave, u32 row) const
	{
		xch[slot(buf, wave, 0u, 0u, row)] = s[0][0];
		xch[slot(buf, wave, 0u, 1u, row)] = s[0][1];
		xch[slot(buf, wave, 1u, 0u, row)] = s[kPT - 1][0];
		xch[slot(buf, wave, 1u, 1u, row)] = s[kPT - 1][1];
		auto plane = [&](u32 p, const u32 (&bl)[2], const u32 (&ab)[2]) {
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				const u32 w = s[p][h], other = s[p][h ^ 1u];
				const u32 l = Faces<B>::left(w, other, h), r = Faces<B>::right(w, other, h);
				const u32 ym = Faces<B>::row_below(w), yp = Faces<B>::row_above(w);
				o[p][h] = rule(w, l, r, ym, yp, bl[h], ab[h]);
			}
		};
		// the planes that need nothing from another wave first, under the exchange's LDS writes and the other waves' way to the barrier
#pragma unroll
		for (u32 p = 1; p + 1u < kPT; p++) plane(p, s[p - 1], s[p + 1]);
		__syncthreads();
		u32 below[2], above[2];
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			below[h] = Faces<B>::has_below(wave) ? xch[slot(buf, Faces<B>::wave_below(wave), 1u, h, row)] : 0u; // z == -1: plane 63, or dead
			above[h] = Faces<B>::has_above(wave) ? xch[slot(buf, Faces<B>::wave_above(wave), 0u, h, row)] : 0u; // z == 64: plane 0, or dead
		}
		plane(0u, below, s[1]);
		plane(kPT - 1u, s[kPT - 2], above);
	}
};
struct VnStep : VnStepT<kBoundaryReference> {}; // (a type of its own name: what is named after it, a kernel's LDS arrays, keeps its name)

// ---- Moore: two words per universe, born | survive, bit c (0 .. 26) = at c live neighbours of 26
// The count is separable, the cell itself included: T = sum over the 3 x 3 x 3 cube, 0 .. 27. x: (left, self, right) of a word -> 2 bit
// planes; y: plus the x-sums of rows y - 1 and y + 1 (DPP) -> 4 bit planes, the PLANE SUM 0 .. 9; z: plus the plane sums of planes z - 1
// and z + 1 -> 5 bit planes. Every axis applies its own boundary (reference: - dead, + wraps) to what the axis before it produced, which
// is the reference's per-axis rule on edges and corners too, and a torus or a closed cube when every axis wraps or none does. A dead cell
// looks up born[T], a live one survive[T - 1]: the survive table is shifted by one when it is loaded and both are indexed by T.
// The plane sums of a wave's first and last plane go through the LDS exchange (8 words a thread and plane, two ds_write_b128 /
// ds_read_b128 each) instead of the raw words with the sums recomputed: 4 writes and 8 reads of 16 bytes a step against 4 + 4 of 4 bytes
// and the x and y sums of four more words, 64 vector instructions (DESIGN 12.1).
template <int B>
struct MooreStepT
{
	static constexpr u32 kXchWords = 2u * kWaves * 2u * 2u * 64u * 4u; // [step parity][wave][first / last plane][word][row][sum plane]: 128 KiB
	static constexpr u32 kRuleWords = 2u;
	static_assert(kRuleWords == ensemble_rule_words(CA3D_ENSEMBLE_MOORE), "the host's rule array and the policy agree");
	// The update is a multiplexer tree over (alive, T4 .. T0) with 28 + 28 workgroup-uniform leaves. A select reads ONE scalar operand, so
	// the born leaves live in vector registers and the (shifted) survive leaves in scalar ones: the leaf level is 28 selects on the
	// alive word with one operand of each kind.
	u32 born[28], surv[28];

	__device__ __forceinline__ void load(const u32 *rules, u32 u)
	{
		const u32 b = rules[2u * u] & 0x7FFFFFFu, sv = (rules[2u * u + 1u] & 0x7FFFFFFu) << 1; // a live cell has T >= 1
#pragma unroll
		for (int c = 0; c < 28; c++)
		{
			born[c] = 0u - ((b >> c) & 1u);
			surv[c] = 0u - ((sv >> c) & 1u);
			asm volatile("" : "+v"(born[c]));
			asm volatile("" : "+s"(surv[c]));
		}
	}
	struct Sum4 { u32 b[4]; }; // a plane sum (0 .. 9) of 32 cells as bit planes

	// x and y of one word: the plane sum
	static __device__ __forceinline__ Sum4 plane_sum(u32 w, u32 other, u32 h)
	{
		const u32 l = Faces<B>::left(w, other, h), r = Faces<B>::right(w, other, h);
		u32 x0, x1;
		fa(l, w, r, x0, x1);
		const u32 m0 = Faces<B>::row_below(x0), m1 = Faces<B>::row_below(x1);
		const u32 p0 = Faces<B>::row_above(x0), p1 = Faces<B>::row_above(x1);
		Sum4 q;
		u32 c0, s1, c1, k;
		fa(x0, m0, p0, q.b[0], c0);
		fa(x1, m1, p1, s1, c1);
		ha(s1, c0, q.b[1], k);
		ha(c1, k, q.b[2], q.b[3]);
		return q;
	}
	// z and the rule: three plane sums -> T (5 planes) -> the multiplexer
	__device__ __forceinline__ u32 rule(u32 w, const Sum4 &a, const Sum4 &b, const Sum4 &c) const
	{
		u32 s0, k0, s1, k1, s2, k2, s3, k3;
		fa(a.b[0], b.b[0], c.b[0], s0, k0);
		fa(a.b[1], b.b[1], c.b[1], s1, k1);
		fa(a.b[2], b.b[2], c.b[2], s2, k2);
		fa(a.b[3], b.b[3], c.b[3], s3, k3);
		u32 T[5], c1, c2, c3;
		T[0] = s0;
		ha(s1, k0, T[1], c1);
		fa(s2, k1, c1, T[2], c2);
		fa(s3, k2, c2, T[3], c3);
		T[4] = k3 | c3; // T <= 27: no carry out
		u32 t[28];
#pragma unroll
		for (int i = 0; i < 28; i++) t[i] = mux(w, surv[i], born[i]);
#pragma unroll
		for (int i = 0; i < 14; i++) t[i] = mux(T[0], t[2 * i + 1], t[2 * i]);
#pragma unroll
		for (int i = 0; i < 7; i++) t[i] = mux(T[1], t[2 * i + 1], t[2 * i]);
#pragma unroll
		for (int i = 0; i < 3; i++) t[i] = mux(T[2], t[2 * i + 1], t[2 * i]);
		// (T = 28 .. 31 does not exist: counts 24 .. 27 need no select on plane 2)
		return mux(T[4], mux(T[3], t[6], t[2]), mux(T[3], t[1], t[0]));
	}
	// in uint4: a row's four sum planes are one 16-byte access, a wave's 64 rows lie back to back
	static __device__ __forceinline__ u32 slot(u32 buf, u32 w, u32 which, u32 h, u32 row) { return (((buf * kWaves + w) * 2u + which) * 2u + h) * 64u + row; }

	__device__ __forceinline__ void step(const u32 (&s)[kPT][2], u32 (&o)[kPT][2], u32 *xch, u32 buf, u32 wave, u32 row) const
	{
		uint4 *x4 = reinterpret_cast<uint4 *>(xch);
		auto put = [&](u32 which, u32 h, const Sum4 &v) { x4[slot(buf, wave, which, h, row)] = make_uint4(v.b[0], v.b[1], v.b[2], v.b[3]); };
		auto get = [&](u32 w, u32 which, u32 h) -> Sum4 {
			const uint4 v = x4[slot(buf, w, which, h, row)];
			return Sum4{{v.x, v.y, v.z, v.w}};
		};
		// A wave's first and last plane sums go to the exchange and are NOT kept: after the barrier the thread reads its own two back
		// beside its neighbours' (4 more ds_read_b128 a step), which frees 16 registers across the interior planes' rule evaluation.
		Sum4 q[kPT - 2][2]; // the interior planes' sums, kept for the outer planes
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			const Sum4 first = plane_sum(s[0][h], s[0][h ^ 1u], h), last = plane_sum(s[kPT - 1][h], s[kPT - 1][h ^ 1u], h);
			put(0u, h, first);
			put(1u, h, last);
			// the planes that need nothing from another wave, under the exchange's LDS writes and the other waves' way to the barrier
#pragma unroll
			for (u32 p = 1; p + 1u < kPT; p++) q[p - 1u][h] = plane_sum(s[p][h], s[p][h ^ 1u], h);
#pragma unroll
			for (u32 p = 1; p + 1u < kPT; p++)
				o[p][h] = rule(s[p][h], p == 1u ? first : q[p - 2u][h], q[p - 1u][h], p + 2u == kPT ? last : q[p][h]);
		}
		__syncthreads();
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			// A plane that does not exist is read from a slot inside the exchange and zeroed. (The - side is written on `wave` itself and
			// the + side keeps both sums as temporaries of the call: through Faces' helpers the reference kernels come out with
			// instructions in another order, DESIGN 12.12)
			Sum4 below = get(Faces<B>::kMinusWraps ? Faces<B>::wave_below(wave) : wave ? wave - 1u : 0u, 1u, h); // z == -1: plane 63, or
			if (!Faces<B>::kMinusWraps && !wave) below = Sum4{{0u, 0u, 0u, 0u}};                                   // dead
			o[0][h] = rule(s[0][h], below, get(wave, 0u, h), q[0][h]);
			if constexpr (Faces<B>::kPlusWraps)
				o[kPT - 1][h] = rule(s[kPT - 1][h], q[kPT - 3][h], get(wave, 1u, h), get(Faces<B>::wave_above(wave), 0u, h)); // z == 64 is plane 0
			else
			{
				// (read ahead of the wave's own sums: with the two reads the other way round the closed kernels spill)
				Sum4 above = get(Faces<B>::wave_above(wave), 0u, h);
				if (!Faces<B>::has_above(wave)) above = Sum4{{0u, 0u, 0u, 0u}}; // z == 64 is dead
				o[kPT - 1][h] = rule(s[kPT - 1][h], q[kPT - 3][h], get(wave, 1u, h), above);
			}
		}
	}
};
struct MooreStep : MooreStepT<kBoundaryReference> {};

// ---- clustered: six words per universe, born | survive of the main (Moore, counts 0 .. 26), edges (0 .. 12) and corners (0 .. 8) rule-sets
// A cell is alive afterwards if ANY of the three lookups says so (oracle/ca_oracle.c, lit_next). A Moore total does not separate the
// classes, so a word of a plane is summarised as seven bit planes that do: `c`, the word itself; D = left + right + c(y - 1) + c(y + 1),
// the four in-plane face neighbours (0 .. 4); As = the left and right neighbours of rows y - 1 and y + 1, the four in-plane diagonals
// (0 .. 4). With b, m, a for the planes z - 1, z, z + 1:
//     faces   F = D(m) + c(b) + c(a)        edges   E = As(m) + D(b) + D(a)        corners   C = As(b) + As(a)        T = F + E + C
// Every axis applies its own boundary to what the axis before it produced (x: alignbit, y: DPP, z: the exchange), as in MooreStep.
// The RAW words of a wave's first and last plane go through the von Neumann exchange (32 KiB); a thread then slides a window of three
// planes' sets over the six planes it sees, one word of a row at a time: 21 registers of sets alive, not 6 x 7 x 2.
template <int B>
struct ClusteredStepT
{
	static constexpr u32 kXchWords = VnStep::kXchWords;
	static constexpr u32 kRuleWords = 6u;
	static_assert(kRuleWords == ensemble_rule_words(CA3D_ENSEMBLE_MOORE, true), "the host's rule array and the policy agree");
	// all-zeros / all-ones per table bit: the born leaves in vector registers, the survive leaves in scalar ones (a select reads ONE scalar)
	u32 bornM[27], survM[27], bornE[13], survE[13], bornC[9], survC[9];

	template <int N>
	static __device__ __forceinline__ void expand(u32 b, u32 sv, u32 (&born)[N], u32 (&surv)[N])
	{
#pragma unroll
		for (int c = 0; c < N; c++)
		{
			born[c] = 0u - ((b >> c) & 1u);
			surv[c] = 0u - ((sv >> c) & 1u);
			asm volatile("" : "+v"(born[c]));
			asm volatile("" : "+s"(surv[c]));
		}
	}
	__device__ __forceinline__ void load(const u32 *rules, u32 u)
	{
		const u32 *r = rules + 6u * u;
		expand<27>(r[0], r[1], bornM, survM);
		expand<13>(r[2], r[3], bornE, survE);
		expand<9>(r[4], r[5], bornC, survC);
	}
	struct Set { u32 c, d[3], as[3]; };

	// x and y of one word
	static __device__ __forceinline__ Set plane_set(u32 w, u32 other, u32 h)
	{
		const u32 l = Faces<B>::left(w, other, h), r = Faces<B>::right(w, other, h);
		Set q;
		q.c = w;
		sum4(l, r, Faces<B>::row_below(w), Faces<B>::row_above(w), q.d);
		sum4(Faces<B>::row_below(l), Faces<B>::row_below(r), Faces<B>::row_above(l), Faces<B>::row_above(r), q.as);
		return q;
	}
	// a multiplexer tree over N leaves (counts 0 .. N - 1) and the count's bit planes p[0] ..; a node without a partner moves up as it is
	template <int N>
	static __device__ __forceinline__ u32 tree(u32 w, const u32 (&born)[N], const u32 (&surv)[N], const u32 *p)
	{
		u32 t[N];
#pragma unroll
		for (int i = 0; i < N; i++) t[i] = mux(w, surv[i], born[i]);
		int n = N;
#pragma unroll
		for (int level = 0; level < 5; level++)
		{
			if (n > 1)
			{
#pragma unroll
				for (int i = 0; i < N / 2; i++)
					if (2 * i + 1 < n) t[i] = mux(p[level], t[2 * i + 1], t[2 * i]);
				if (n & 1) t[n / 2] = t[n - 1];
				n = (n + 1) / 2;
			}
		}
		return t[0];
	}
	// z and the rule: three planes' sets -> F, E, C, T -> three multiplexers, ORed
	__device__ __forceinline__ u32 rule(const Set &b, const Set &m, const Set &a) const
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
		return bitop3<(TA | TB | TC)>(tree<27>(w, bornM, survM, T), tree<13>(w, bornE, survE, E), tree<9>(w, bornC, survC, C));
	}

	__device__ __forceinline__ void step(const u32 (&s)[kPT][2], u32 (&o)[kPT][2], u32 *xch, u32 buf, u32 wave, u32 row) const
	{
		xch[VnStep::slot(buf, wave, 0u, 0u, row)] = s[0][0];
		xch[VnStep::slot(buf, wave, 0u, 1u, row)] = s[0][1];
		xch[VnStep::slot(buf, wave, 1u, 0u, row)] = s[kPT - 1][0];
		xch[VnStep::slot(buf, wave, 1u, 1u, row)] = s[kPT - 1][1];
		__syncthreads();
		u32 below[2], above[2];
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			below[h] = Faces<B>::has_below(wave) ? xch[VnStep::slot(buf, Faces<B>::wave_below(wave), 1u, h, row)] : 0u; // z == -1: plane 63, or dead
			above[h] = Faces<B>::has_above(wave) ? xch[VnStep::slot(buf, Faces<B>::wave_above(wave), 0u, h, row)] : 0u; // z == 64: plane 0, or dead
		}
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			Set lo = plane_set(below[h], below[h ^ 1u], h), mid = plane_set(s[0][h], s[0][h ^ 1u], h);
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const Set hi = p + 1u < kPT ? plane_set(s[p + 1u][h], s[p + 1u][h ^ 1u], h) : plane_set(above[h], above[h ^ 1u], h);
				o[p][h] = rule(lo, mid, hi);
				lo = mid;
				mid = hi;
			}
		}
	}
};
struct ClusteredStep : ClusteredStepT<kBoundaryReference> {};
