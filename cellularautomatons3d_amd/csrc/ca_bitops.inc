// v_bitop3 helpers and carry-save adder trees over 1-bit planes: the part of the bit-sliced CA code that needs
// nothing but the compiler (shared by every kernel, and compiled at run time by hiprtc for the rule-specialised
// kernels of ca_jit.cpp). Device code only; include inside namespace ca3d { namespace { ... } }.
#pragma once

typedef unsigned int u32;

constexpr u32 TA = 0xF0, TB = 0xCC, TC = 0xAA; // truth-table columns of the three v_bitop3 inputs

template <u32 IMM>
__device__ __forceinline__ u32 bitop3(u32 a, u32 b, u32 c)
{
	return __builtin_amdgcn_bitop3_b32(a, b, c, IMM);
}
__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) { return bitop3<(TA ^ TB ^ TC)>(a, b, c); }
__device__ __forceinline__ u32 maj3(u32 a, u32 b, u32 c) { return bitop3<((TA & TB) | (TA & TC) | (TB & TC))>(a, b, c); }
// bit i of the result = bit i-1 of the row (neighbour at x-1): (w << 1) | (lower >> 31)
__device__ __forceinline__ u32 from_left(u32 w, u32 lower) { return __builtin_amdgcn_alignbit(w, lower, 31); }
// bit i of the result = bit i+1 of the row (neighbour at x+1): (w >> 1) | (upper << 31)
__device__ __forceinline__ u32 from_right(u32 upper, u32 w) { return __builtin_amdgcn_alignbit(upper, w, 1); }

__device__ __forceinline__ void fa(u32 a, u32 b, u32 c, u32 &s, u32 &k) { s = xor3(a, b, c); k = maj3(a, b, c); }
__device__ __forceinline__ void ha(u32 a, u32 b, u32 &s, u32 &k) { s = a ^ b; k = a & b; }

// ---- lane exchange without LDS ----------------------------------------------------------------------------
// DPP controls (gfx9 encoding)
constexpr int kDppWaveShl1 = 0x130; // lane i <- lane i + 1
constexpr int kDppWaveRol1 = 0x134; // lane i <- lane (i + 1) % 64
constexpr int kDppWaveShr1 = 0x138; // lane i <- lane i - 1
constexpr int kDppWaveRor1 = 0x13C; // lane i <- lane (i + 63) % 64
template <int CTRL>
__device__ __forceinline__ u32 dpp_mov(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true); }

// Word 0 of the lane that starts this lane's row (CV lanes per row), valid in the row's last lane.
// CVL < 0: rows that are not a power of two of lanes — `lane` is then the index of the row's FIRST lane (ds_bpermute, no LDS traffic).
template <int CVL>
__device__ __forceinline__ u32 row_first(u32 w0, int lane)
{
	if (CVL < 0) return (u32)__builtin_amdgcn_ds_bpermute(lane << 2, (int)w0);
	if (CVL == 1) return dpp_mov<0 | (0 << 2) | (2 << 4) | (2 << 6)>(w0);  // quad_perm:[0,0,2,2]
	if (CVL == 2) return dpp_mov<0>(w0);                                     // quad_perm:[0,0,0,0]
	if (CVL == 3) return dpp_mov<0x110 + 7>(w0);                             // row_shr:7
	if (CVL == 4) return dpp_mov<0x110 + 15>(w0);                            // row_shr:15
	if (CVL == 5) return (u32)__shfl((int)w0, lane & 32);                    // 32 lanes per row: no DPP pattern
	return dpp_mov<kDppWaveRol1>(w0);                                        // the row is the wave
}

// ---- sums of 1-bit planes (carry-save trees) -------------------------------------------------------------
__device__ __forceinline__ void sum4(u32 a, u32 b, u32 c, u32 d, u32 (&p)[3])
{
	u32 s, k, k2;
	fa(a, b, c, s, k);
	ha(s, d, p[0], k2);
	ha(k, k2, p[1], p[2]);
}

__device__ __forceinline__ void sum6(u32 a, u32 b, u32 c, u32 d, u32 e, u32 f, u32 (&p)[3])
{
	u32 s0, k0, s1, k1, c0;
	fa(a, b, c, s0, k0);
	fa(d, e, f, s1, k1);
	ha(s0, s1, p[0], c0);
	fa(k0, k1, c0, p[1], p[2]);
}

__device__ __forceinline__ void sum8(const u32 (&x)[8], u32 (&p)[4])
{
	u32 s0, k0, s1, k1, s2, k2, k3, t, u, v;
	fa(x[0], x[1], x[2], s0, k0);
	fa(x[3], x[4], x[5], s1, k1);
	ha(x[6], x[7], s2, k2);
	fa(s0, s1, s2, p[0], k3);
	fa(k0, k1, k2, t, u);
	ha(t, k3, p[1], v);
	ha(u, v, p[2], p[3]);
}

__device__ __forceinline__ void sum12(const u32 (&x)[12], u32 (&p)[4])
{
	u32 s0, s1, s2, s3, k0, k1, k2, k3, t, u, v, a, b, c, d, e;
	fa(x[0], x[1], x[2], s0, k0);
	fa(x[3], x[4], x[5], s1, k1);
	fa(x[6], x[7], x[8], s2, k2);
	fa(x[9], x[10], x[11], s3, k3);
	fa(s0, s1, s2, t, u);
	ha(t, s3, p[0], v);
	fa(k0, k1, k2, a, b);
	fa(k3, u, v, c, d);
	ha(a, c, p[1], e);
	fa(b, d, e, p[2], p[3]);
}

// vn (0..6, 3 planes) + corners (0..8, 4 planes) + edges (0..12, 4 planes) -> 0..26, 5 planes
__device__ __forceinline__ void sum_moore(const u32 (&vn)[3], const u32 (&ed)[4], const u32 (&co)[4], u32 (&p)[5])
{
	u32 q0, q1, q2, q3, c;
	ha(vn[0], co[0], q0, c);
	fa(vn[1], co[1], c, q1, c);
	fa(vn[2], co[2], c, q2, c);
	q3 = co[3] ^ c; // <= 14: no carry out of plane 3
	ha(q0, ed[0], p[0], c);
	fa(q1, ed[1], c, p[1], c);
	fa(q2, ed[2], c, p[2], c);
	fa(q3, ed[3], c, p[3], p[4]);
}

__device__ __forceinline__ u32 next_state(u32 alive, u32 S, u32 B)
{
	return bitop3<((TA & TB) | (~TA & TC)) & 0xFF>(alive, S, B); // alive ? survive : born
}

// ---- von Neumann rule from compile-time truth tables ------------------------------------------------------------
// New state of 32 cells from their own word and the six face-neighbour words, for rule tables known when the kernel is
// compiled (bit k of LS / LB: a live / dead cell with k live neighbours is alive afterwards; k = 0 .. 6, entry 7 is a
// don't-care the host has canonicalised). The compiler does not see through v_bitop3's immediate, so what the tables
// make unnecessary is dropped here: count bit-planes neither table depends on are not formed, and when at most two
// count planes matter the whole update "alive ? survive(count) : born(count)" is ONE v_bitop3 of (alive, plane, plane).
// The reference's start-up rule B1,3 / S0-6 (LS 0xFF, LB 0x0A) needs planes 0 and 2 only: 8 ops instead of 11 — 7 with the carry that
// the tables make a don't-care dropped (vn_same_for_parity).
template <int T>
__device__ constexpr bool vn_table_depends(int k)
{
	for (int i = 0; i < 8; i++)
		if (((T >> i) & 1) != ((T >> (i ^ (1 << k))) & 1)) return true;
	return false;
}
// truth table of bitop3(alive, pa, pb) for count planes at bit positions ka > kb (kb < 0: unused)
template <int LS, int LB>
__device__ constexpr u32 vn_fused_imm(int ka, int kb)
{
	u32 imm = 0;
	for (int idx = 0; idx < 8; idx++)
	{
		const int alive = (idx >> 2) & 1, xa = (idx >> 1) & 1, xb = idx & 1;
		const int cnt = (ka >= 0 ? xa << ka : 0) | (kb >= 0 ? xb << kb : 0);
		const int v = alive ? (LS >> cnt) & 1 : (LB >> cnt) & 1;
		imm |= (u32)v << idx;
	}
	return imm;
}
// Do both tables give one answer for every entry 0 .. 7 of parity v? Then the count's high planes are only ever consulted where
// plane 0 is 1 - v, and there the carry out of plane 0 is known: the six inputs are summed as two full adders (s0, k0), (s1, k1) and
// plane 0 = s0 ^ s1, carry t = s0 & s1 — plane 0 set means s0 != s1, so t = 0; plane 0 clear means s0 == s1, so t = s0.
template <int LS, int LB>
__device__ constexpr bool vn_same_for_parity(int v)
{
	// (entry 7 included: with the wrong carry the planes of an odd count can read 1, 1, 1 — a count no cell has, whose entry the host
	// fills as it likes)
	for (int c = v; c <= 7; c += 2)
		if (((LS >> c) & 1) != ((LS >> v) & 1) || ((LB >> c) & 1) != ((LB >> v) & 1)) return false;
	return true;
}
template <int LS, int LB>
__device__ __forceinline__ u32 vn_next(u32 alive, u32 a, u32 b, u32 c, u32 d, u32 e, u32 f)
{
	constexpr bool n0 = vn_table_depends<LS>(0) || vn_table_depends<LB>(0);
	constexpr bool n1 = vn_table_depends<LS>(1) || vn_table_depends<LB>(1);
	constexpr bool n2 = vn_table_depends<LS>(2) || vn_table_depends<LB>(2);
	constexpr int needed = (n0 ? 1 : 0) + (n1 ? 1 : 0) + (n2 ? 1 : 0);
	u32 p0 = 0, p1 = 0, p2 = 0;
	if constexpr (needed > 0)
	{
		const u32 s0 = xor3(a, b, c), s1 = xor3(d, e, f);
		if constexpr (n0) p0 = s0 ^ s1;
		if constexpr (n1 || n2)
		{
			const u32 k0 = maj3(a, b, c), k1 = maj3(d, e, f);
			if constexpr (vn_same_for_parity<LS, LB>(0))
			{
				// the start-up rule B1,3 / S0-6 is of this kind (no even count changes anything): one instruction fewer, 7 instead of 8
				if constexpr (n1) p1 = k0 ^ k1;
				if constexpr (n2) p2 = k0 & k1;
			}
			else
			{
				const u32 t = vn_same_for_parity<LS, LB>(1) ? s0 : (s0 & s1);
				if constexpr (n1) p1 = xor3(k0, k1, t);
				if constexpr (n2) p2 = maj3(k0, k1, t);
			}
		}
	}
	if constexpr (needed <= 2)
	{
		constexpr int ka = n2 ? 2 : (n1 ? 1 : (n0 ? 0 : -1));
		constexpr int kb = n2 ? (n1 ? 1 : (n0 ? 0 : -1)) : (n1 ? (n0 ? 0 : -1) : -1);
		constexpr u32 imm = vn_fused_imm<LS, LB>(ka, kb);
		const u32 pa = ka == 2 ? p2 : (ka == 1 ? p1 : p0), pb = kb == 1 ? p1 : p0;
		return bitop3<imm>(alive, pa, pb);
	}
	else
	{
		const u32 S = bitop3<(LS & 0xFF)>(p2, p1, p0), B = bitop3<(LB & 0xFF)>(p2, p1, p0);
		return next_state(alive, S, B);
	}
}
