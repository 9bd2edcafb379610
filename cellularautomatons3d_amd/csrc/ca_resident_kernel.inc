// Device code of the resident multi-step kernel: K steps of the packed CA in ONE launch with the state held on chip.
// Compiled ahead of time (ca_resident.hip: the start-up rule) and at run time by hiprtc with the rule's truth tables
// as constants (ca_jit.cpp). Needs ca_bitops.inc.
//
// Why. A 512^3 step moves 32 MiB and takes 5.8 us as a kernel per step, of which ~1.5 us is the launch boundary and
// most of the rest one load and one store round trip (DESIGN.md 4.6): at this size the step is a latency chain, and
// the whole state (16 MiB) is smaller than the chip's register files (256 CUs x 512 KiB). So: no launch boundary and no
// round trip through memory for the bulk of the state.
//   * The grid is cut into 256 tiles of 32 (y) x 32 (z) rows, full x extent (512 cells = 16 words); one 512-thread
//     workgroup per tile, one tile per CU. A thread owns word x of row y for all 32 planes of the tile: 32 VGPRs that
//     stay in registers for the whole launch.
//   * Neighbours: z +- 1 are the thread's own registers; x +- 1 come from the neighbour lanes by DPP (a row of 16 words
//     is exactly one DPP row: row_shr:1 zero-fills lane 0 = the dead x-1 of word 0, row_ror:15 wraps word 15 to word 0);
//     y +- 1 come from the workgroup's LDS image of the tile (each thread publishes its 32 words as 8 ds_write_b128 and
//     reads the rows above and below as 16 ds_read_b128; double-buffered: one barrier per step).
//   * Only tile FACES cross the chip: after each step a tile publishes its first / last plane and its first / last row
//     (4 x 512 words) as 8-byte {tag = state number, word} granules written with one sc1 store each, and polls the
//     four neighbour tiles' granules for the same state number (data-tagged hand-off: no flags, no fences, no grid
//     barrier; a tile waits only for its four neighbours). 2 MiB per step chip-wide instead of 32 MiB.
//   * Boundary semantics as everywhere (SURVEY Appendix A): faces at coordinate -1 are dead (read as zero), faces at
//     coordinate G are the opposite tile's first rows / planes.
// Every spin is bounded by a wall-clock timeout (s_memrealtime): a workgroup that is not resident, or any other
// surprise, ends the launch with status[0] != 0 instead of hanging the GPU; the host then reports an error.

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) u32 gu32;

struct ResidentArgs
{
	const u32 *in;            // state T0: whole grid, packed layout
	u32 *out_last;            // receives state T0 + steps
	u32 *out_prev;            // receives state T0 + steps - 1 (the other ping-pong buffer)
	unsigned long long *mail; // granules [2 parities][tiles][4 faces][512]
	u32 *status;              // [0] != 0: a wait timed out (1 + the tile that gave up first), the state is then invalid;
	                          // [4 + tile]: steps that tile has finished (diagnostics)
	u32 *host_flag;           // pinned host word, written (system scope) only when a wait times out: the host sees the
	                          // failure at its next synchronisation without a copy per launch
	u32 steps;                // >= 1
	u32 epoch0;               // tag of state T0 + j is epoch0 + j + 1; never repeats between memsets of `mail`
	u32 timeout_ticks;        // per wait, in s_memrealtime ticks (100 MHz)
	u32 fault_tile;           // diagnostics (option "resident_fault_tile"): tile + 1 that leaves at once, as a workgroup that never became
	                          // resident would; 0 in normal operation
};

// A launch does nothing when an earlier one gave up (status[0] stays set until the host has recovered): the launches queued
// behind the failed one must not overwrite the buffers the host re-runs the steps from.
__device__ __forceinline__ bool res_must_skip(const ResidentArgs &a, u32 tile)
{
	if (__hip_atomic_load((const gu32 *)a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return true;
	return a.fault_tile == tile + 1u;
}
// The first tile to time out names itself and the launch (its epoch0) for the host.
__device__ __forceinline__ void res_report_timeout(const ResidentArgs &a, u32 tile)
{
	__hip_atomic_store((gu32 *)a.status + 1, a.epoch0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_store(a.host_flag + 1, a.epoch0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store((gu32 *)a.status, tile + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	__hip_atomic_store(a.host_flag, tile + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int kResTileRows = 32;   // y rows and z planes per tile
constexpr int kResThreads = 512;   // 16 words x 32 rows
constexpr int kResFaceWords = 512; // words per face
enum { RES_FACE_ZLO = 0, RES_FACE_ZHI = 1, RES_FACE_YLO = 2, RES_FACE_YHI = 3 };
// LDS image of one state: 34 rows (halo row, 32 own rows, halo row) x 8 chunks of 4 planes x 16 words, 16 bytes per
// (row, chunk, word): the 16 lanes of a row are contiguous (a ds_read_b128 / ds_write_b128 of a wave touches every
// bank group once) and a thread's chunks and neighbour rows sit at compile-time offsets from one base address.
constexpr u32 kResImageBytes = 34u * 16u * 128u;
constexpr u32 kResLdsBytes = 2u * kResImageBytes + 2u * 64u * 4u + 16u; // two images, the face pass's side words, the abort word: 136.5 KiB

template <int RY, int CW = 16, int PZ = 32, int ZS = 1>
struct ResidentLds
{
	static constexpr u32 bytes = 2u * (RY + 2u) * (PZ / 4u) * CW * 16u + 2u * 4u * CW * 4u + 16u; // two images, the face pass's side words, the abort word
};

// byte offset of (row, chunk of 4 planes, word) in an image of NCH chunks per row and CW words per row
template <u32 NCH = 8u, u32 CW = 16u>
__device__ __forceinline__ u32 res_chunk_off(u32 row, u32 x, u32 chunk) { return ((row * NCH + chunk) * CW + x) * 16u; }

__device__ __forceinline__ void res_store_granule(unsigned long long *p, u32 tag, u32 value)
{
	__hip_atomic_store((gu64 *)p, ((unsigned long long)tag << 32) | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // ONE sc1 store
}

// One output word of the von Neumann rule from its six neighbour words.
template <int LS, int LB>
__device__ __forceinline__ u32 res_rule(u32 w, u32 l, u32 r, u32 ym, u32 yp, u32 below, u32 above)
{
	return vn_next<LS, LB>(w, l, r, yp, ym, above, below);
}
__device__ __forceinline__ u32 res_left(u32 w) { return from_left(w, dpp_mov<0x111>(w)); }   // row_shr:1 — word x-1, zero at x == 0 (x-1 == -1 is dead)
__device__ __forceinline__ u32 res_right(u32 w) { return from_right(dpp_mov<0x12F>(w), w); } // row_ror:15 — word x+1, word 0 after word 15 (x == G wraps)
// Rows of 8 words (256^3): a DPP row of 16 lanes holds TWO grid rows. x-1: row_shr:1, masked at x == 0 (lane 8 would get the
// other row's word 7); x+1: row_shl:1, except word 7, which takes its own row's word 0 by row_shr:7.
template <int CW>
__device__ __forceinline__ u32 res_left_w(u32 w, u32 xmask)
{
	if (CW == 16) return res_left(w);
	return from_left(w, dpp_mov<0x111>(w) & xmask);
}
template <int CW>
__device__ __forceinline__ u32 res_right_w(u32 w, bool last_word)
{
	if (CW == 16) return res_right(w);
	const u32 nxt = dpp_mov<0x101>(w), wrap = dpp_mov<0x117>(w); // row_shl:1, row_shr:7
	return from_right(last_word ? wrap : nxt, w);
}

// RY = rows of a tile (32: one workgroup per CU; 16: two per CU, whose phases interleave).
// CW = words per grid row, PZ = planes per tile: 16 / 32 at 512^3; 8 / 8 at 256^3 (256 tiles of 8 words x 32 rows x 8 planes,
// one workgroup per CU — the step is a latency chain there, and the shortest one is the one with the least work per thread
// that still gives every CU a tile).
// ZS = thread groups along z (round 3). ZS = 1: a thread owns word x of row y for ALL PZ planes of the tile — 512 threads per CU
// at 512^3, two waves per SIMD. ZS = 2: two threads share a (row, word) column, PT = PZ / 2 planes each — 1024 threads per CU,
// four waves per SIMD; the plane across the split comes from the LDS image (one ds_read_b32), the thread group at either end of
// the tile handles that end's z face, and a thread handles one y-face word of one face instead of one of each. Same image, same
// mailboxes, same tags. Built to test whether two waves per SIMD were what held the kernel at 0.32 of the VALU peak: they were
// not — a wave of this kernel has 32 independent planes to issue from, and ZS = 2 measures 2.61 against 2.52 us per step at
// 512^3 (1.37 / 1.26 at 256^3; with 16-row tiles, two workgroups per CU, it wins: 2.89 / 3.31). The default stays ZS = 1.
#ifndef CA3D_RES_PIN_PASS
#define CA3D_RES_PIN_PASS 1 // 0: the main pass is free to sink behind the request for the next faces (the order up to round 5)
#endif
template <int LS, int LB, int RY, int CW = 16, int PZ = 32, int ZS = 1>
__device__ __forceinline__ void resident_run(const ResidentArgs &a, char *lds)
{
	constexpr u32 C = (u32)CW, G = 32u * C, TPAY = G / RY, TPAZ = G / (u32)PZ; // words per row, grid edge, tiles per axis
	constexpr u32 PT = (u32)PZ / (u32)ZS;                                       // planes per thread
	static_assert(PT * ZS == PZ && PT % 4 == 0 && PT >= 4, "a thread owns whole 4-plane chunks");
	constexpr u32 ZF = C * RY, NT = ZF * ZS, YF = C * (u32)PZ;                 // words of a z face; threads; words of a y face
	constexpr u32 FE = (2u * YF + NT - 1u) / NT;                                // y-face words per thread (both faces together: entry e = face * YF + word)
	constexpr u32 FW = ZF > YF ? ZF : YF;                                       // mailbox words per face
	constexpr u32 NCH = (u32)PZ / 4u, TCH = PT / 4u;                            // chunks of 4 planes per row / per thread
	constexpr u32 kImage = (RY + 2u) * NCH * C * 16u;                          // bytes of one LDS image
	// Where the next faces are asked for (prefetch_faces): after the main pass when that pass is long, after the image write
	// when it is short (8 planes or fewer per thread: asked for earlier, the loads came back with the old tags and the next step
	// began with a second round trip — 1.67 vs 1.37 us per step at 256^3; a further delay of 64 - 512 cycles changes nothing)
	constexpr bool kPreAfterImage = PT <= 8;
	const u32 tile = blockIdx.x;
	if (res_must_skip(a, tile)) return;
	const u32 ty = tile % TPAY, tz = tile / TPAY;
	const u32 tid = threadIdx.x, zt = tid % ZF, zh = tid / ZF; // position in the (row, word) face; z group
	const u32 x = zt % C, yl = zt / C;
	const u32 y0 = ty * RY, z0 = tz * (u32)PZ, pz0 = zh * PT;
	const bool z_first = zh == 0u, z_last = zh == (u32)ZS - 1u;
	u32 xmask = x == 0u ? 0u : 0xFFFFFFFFu; // rows of 8 words: x-1 is dead at x == 0
	asm volatile("" : "+v"(xmask));
	const bool xlast = x == C - 1u;
	auto left_of = [&](u32 w) { return res_left_w<CW>(w, xmask); };
	auto right_of = [&](u32 w) { return res_right_w<CW>(w, xlast); };
	// LDS: two images, then per image parity the planes below / above the tile for rows 0 and RY - 1 ([parity][lo|hi][row 0|RY-1][x]),
	// then the workgroup's abort word
	u32 *side = reinterpret_cast<u32 *>(lds + 2u * kImage);
	u32 *abort_lds = side + 2u * 2u * 2u * C;

	// neighbour tiles (faces at coordinate -1 are dead: read as zero; coordinate G wraps to tile 0 of that axis)
	const bool dead_ylo = ty == 0, dead_zlo = tz == 0;
	const u32 t_ylo = (ty == 0 ? TPAY - 1u : ty - 1u) + tz * TPAY, t_yhi = (ty + 1u == TPAY ? 0u : ty + 1u) + tz * TPAY;
	const u32 t_zlo = ty + (tz == 0 ? TPAZ - 1u : tz - 1u) * TPAY, t_zhi = ty + (tz + 1u == TPAZ ? 0u : tz + 1u) * TPAY;
	auto mailbox = [&](u32 parity, u32 t, u32 face) { return a.mail + (((size_t)parity * (TPAY * TPAZ) + t) * 4u + face) * FW; };
	// y-face entries of this thread: e = tid + NT * k; entry e = (face e / YF: 0 = row 0 / the lower neighbour, 1 = row RY - 1 / the
	// upper one; word e % YF = plane * C + x'). NT and YF are multiples of C, so x' == x: whole DPP rows take part together.
	auto y_entry_active = [&](u32 k) { return tid + NT * k < 2u * YF; };

	// ---- state T0 into registers
	u32 s[PT];
	{
		const u32 *src = a.in + ((size_t)(z0 + pz0) * G + (y0 + yl)) * C + x;
#pragma unroll
		for (int p = 0; p < (int)PT; p++) s[p] = src[(size_t)p * G * C];
	}
	if (tid == 0) *abort_lds = 0;

	// my PT words -> own row of LDS image `img`
	auto to_image = [&](u32 img) {
		char *base = lds + img * kImage;
#pragma unroll
		for (int c = 0; c < (int)TCH; c++)
		{
			uint4 v;
			v.x = s[4 * c]; v.y = s[4 * c + 1]; v.z = s[4 * c + 2]; v.w = s[4 * c + 3];
			*reinterpret_cast<uint4 *>(base + res_chunk_off<NCH, C>(yl + 1u, x, zh * TCH + (u32)c)) = v;
		}
	};
	// the initial state's faces: later states publish theirs from inside the step (below)
	to_image(0);
	{
		const u32 tag0 = a.epoch0 + 1u, par0 = tag0 & 1u;
		if (z_first) res_store_granule(mailbox(par0, tile, RES_FACE_ZLO) + zt, tag0, s[0]);
		if (z_last) res_store_granule(mailbox(par0, tile, RES_FACE_ZHI) + zt, tag0, s[PT - 1]);
		if (yl == 0)
		{
#pragma unroll
			for (int p = 0; p < (int)PT; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YLO) + (pz0 + (u32)p) * C + x, tag0, s[p]);
		}
		if (yl == RY - 1)
		{
#pragma unroll
			for (int p = 0; p < (int)PT; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YHI) + (pz0 + (u32)p) * C + x, tag0, s[p]);
		}
	}

	// faces of the next state fetched ahead, under the main pass (valid when their tags match)
	unsigned long long pre[2 + FE];
#pragma unroll
	for (int k = 0; k < 2 + (int)FE; k++) pre[k] = 0;
	bool have_pre = false;

#ifdef CA3D_RES_STAMPS
	// diagnostic build (tools/ubench/resident_probe): cycles per phase, summed over the steps, for wave 0 and the middle wave of tile 37
	unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = 0;
#define RES_STAMP(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); st_acc[i] += now_ - st_prev; st_prev = now_; } while (0)
#else
#define RES_STAMP(i) do { } while (0)
#endif
	for (u32 t = 0; t < a.steps; t++)
	{
		const u32 tag = a.epoch0 + t + 1u, par = tag & 1u, img = t & 1u;
		const bool last = t + 1u == a.steps;
#ifdef CA3D_RES_STAMPS
		st_prev = __builtin_amdgcn_s_memtime();
		__builtin_amdgcn_s_waitcnt(0xC07F);
#endif
		// ---- A. the neighbour faces of state t: my word of the plane below (first z group) / above (last z group), and my
		// entries of the rows below / above, which go into the image's halo rows
		const gu64 *g_zlo = (const gu64 *)(mailbox(par, t_zlo, RES_FACE_ZHI) + zt);
		const gu64 *g_zhi = (const gu64 *)(mailbox(par, t_zhi, RES_FACE_ZLO) + zt);
		auto y_granule = [&](u32 parity, u32 k) {
			const u32 e = tid + NT * k, f = e / YF, g = e % YF;
			return (const gu64 *)(mailbox(parity, f ? t_yhi : t_ylo, f ? RES_FACE_YLO : RES_FACE_YHI) + g);
		};
		u32 zlo = 0, zhi = 0, hy[FE];
		{
			const unsigned long long done = (unsigned long long)tag << 32; // stands for a granule this thread does not wait for
			unsigned long long q0 = pre[0], q1 = pre[1], q2[FE];
#pragma unroll
			for (int k = 0; k < (int)FE; k++) q2[k] = pre[2 + k];
			unsigned long long t_start = 0;
			for (u32 spins = 0;; spins++)
			{
				// A dead face is waited for like a live one and its data dropped: the tile on the other side reads MY
				// face of this state (its +1 wraps to me), and a mailbox slot is reused two states later — if I did not
				// wait for that tile I could run ahead of it and overwrite a face it has not read yet.
				if (spins || !have_pre)
				{
					q0 = z_first ? __hip_atomic_load(g_zlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					q1 = z_last ? __hip_atomic_load(g_zhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
#pragma unroll
					for (int k = 0; k < (int)FE; k++)
						q2[k] = y_entry_active((u32)k) ? __hip_atomic_load(y_granule(par, (u32)k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
				}
				zlo = dead_zlo ? 0u : (u32)q0; zhi = (u32)q1;
				bool ok = (u32)(q0 >> 32) == tag && (u32)(q1 >> 32) == tag;
#pragma unroll
				for (int k = 0; k < (int)FE; k++)
				{
					const bool lower = (tid + NT * (u32)k) / YF == 0u; // an entry of the LOWER neighbour's face: dead at the grid's y == 0
					hy[k] = (lower && dead_ylo) ? 0u : (u32)q2[k];
					ok = ok && (u32)(q2[k] >> 32) == tag;
				}
#ifdef CA3D_RES_NO_WAIT
				break; // timing experiment only (tools/ubench/resident_probe): results are wrong
#endif
				if (__all(ok)) break;
				// bounded: give up (and tell everybody) after timeout_ticks of wall clock, or when somebody else has
				if ((spins & 63u) == 63u)
				{
					const unsigned long long now = __builtin_amdgcn_s_memrealtime();
					if (t_start == 0) t_start = now;
					const bool expired = now - t_start > a.timeout_ticks;
					const u32 other = __hip_atomic_load((const gu32 *)a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (expired || other)
					{
						if (expired && !other && (tid & 63u) == 0) res_report_timeout(a, tile);
						if ((tid & 63u) == 0) *abort_lds = 1; // every wave of the workgroup leaves after the barrier below
						break;
					}
				}
				if (spins) __builtin_amdgcn_s_sleep(1);
			}
		}
		RES_STAMP(0);
		// ---- B. halo rows of the image; the planes below / above rows 0 and RY - 1 for the face pass
		{
			char *base = lds + img * kImage;
#pragma unroll
			for (int k = 0; k < (int)FE; k++)
			{
				if (!y_entry_active((u32)k)) continue;
				const u32 e = tid + NT * (u32)k, f = e / YF, g = e % YF, hp = g / C, hx = g % C; // word g = (plane hp, word hx) of a y face
				*reinterpret_cast<u32 *>(base + res_chunk_off<NCH, C>(f ? RY + 1u : 0u, hx, hp >> 2) + (hp & 3u) * 4u) = hy[k];
			}
			if (yl == 0 || yl == RY - 1)
			{
				u32 *sd = side + img * (4u * C) + (yl ? C : 0u) + x; // [lo | hi][row 0 | RY - 1][x]
				if (z_first) sd[0] = zlo;
				if (z_last) sd[2u * C] = zhi;
			}
		}
		__syncthreads(); // image `img` complete: own rows (written at the end of the previous step) + both halo rows
		if (*abort_lds) return;
		RES_STAMP(1);

		const char *im = lds + img * kImage;
		const u32 ntag = tag + 1u, npar = ntag & 1u;
		RES_STAMP(2);
		// ---- C. the y faces of state t + 1 FIRST: rows 0 and RY - 1 of every plane, one word per entry (plane fp, word fx),
		// from the image — so that they are on their way to the neighbours while the main pass runs
		if (!last)
#pragma unroll
		for (int k = 0; k < (int)FE; k++)
		{
			if (!y_entry_active((u32)k)) continue; // (whole waves: 2 YF is a multiple of 64)
			const u32 e = tid + NT * (u32)k, f = e / YF, g = e % YF, fp = g / C, fx = g % C, ch = fp >> 2, wi = (fp & 3u) * 4u;
			const u32 fpm = fp ? fp - 1u : 0u, fpp = fp < (u32)PZ - 1u ? fp + 1u : (u32)PZ - 1u; // clamped: the ends take the side words instead
			const u32 chm = fpm >> 2, wim = (fpm & 3u) * 4u, chp = fpp >> 2, wip = (fpp & 3u) * 4u;
			const u32 row = f ? RY : 1u; // image row of the tile's first / last row
			const u32 w = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, fx, ch) + wi);
			const u32 fym = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row - 1u, fx, ch) + wi);
			const u32 fyp = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row + 1u, fx, ch) + wi);
			const u32 *sd = side + img * (4u * C) + (f ? C : 0u) + fx;
			const u32 below = fp ? *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, fx, chm) + wim) : sd[0];
			const u32 above = fp < (u32)PZ - 1u ? *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, fx, chp) + wip) : sd[2u * C];
			const u32 o = res_rule<LS, LB>(w, left_of(w), right_of(w), fym, fyp, below, above);
			res_store_granule(mailbox(npar, tile, f ? RES_FACE_YHI : RES_FACE_YLO) + g, ntag, o);
		}

		// ---- rows y-1 and y+1 of my PT planes; the plane across the z split of the tile (ZS > 1)
		u32 ym[PT], yp[PT];
#pragma unroll
		for (int c = 0; c < (int)TCH; c++)
		{
			const uint4 m = *reinterpret_cast<const uint4 *>(im + res_chunk_off<NCH, C>(yl, x, zh * TCH + (u32)c));
			const uint4 q = *reinterpret_cast<const uint4 *>(im + res_chunk_off<NCH, C>(yl + 2u, x, zh * TCH + (u32)c));
			ym[4 * c] = m.x; ym[4 * c + 1] = m.y; ym[4 * c + 2] = m.z; ym[4 * c + 3] = m.w;
			yp[4 * c] = q.x; yp[4 * c + 1] = q.y; yp[4 * c + 2] = q.z; yp[4 * c + 3] = q.w;
		}
		u32 below_first = zlo, above_last = zhi;
		if (ZS > 1)
		{
			// my own row, the plane just below my first / just above my last one: the other z group's word of state t
			if (!z_first) below_first = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(yl + 1u, x, (pz0 - 1u) >> 2) + ((pz0 - 1u) & 3u) * 4u);
			if (!z_last) above_last = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(yl + 1u, x, (pz0 + PT) >> 2) + ((pz0 + PT) & 3u) * 4u);
		}

		RES_STAMP(3);
		// ---- D. one step in place. My first and last plane first: at the tile's ends they are the z faces of state t + 1
		const u32 n0 = res_rule<LS, LB>(s[0], left_of(s[0]), right_of(s[0]), ym[0], yp[0], below_first, s[1]);
		const u32 nl = res_rule<LS, LB>(s[PT - 1], left_of(s[PT - 1]), right_of(s[PT - 1]), ym[PT - 1], yp[PT - 1], s[PT - 2], above_last);
		if (!last)
		{
			if (z_first) res_store_granule(mailbox(npar, tile, RES_FACE_ZLO) + zt, ntag, n0);
			if (z_last) res_store_granule(mailbox(npar, tile, RES_FACE_ZHI) + zt, ntag, nl);
		}
		__builtin_amdgcn_sched_barrier(0);
		RES_STAMP(4);
		u32 below = s[0];
#pragma unroll
		for (int p = 1; p < (int)PT - 1; p++)
		{
			const u32 w = s[p];
			s[p] = res_rule<LS, LB>(w, left_of(w), right_of(w), ym[p], yp[p], below, s[p + 1]);
			below = w;
		}
		auto prefetch_faces = [&]() {
			if (!last)
			{
				// The neighbours published their faces of state t + 1 about as long ago as I did mine (two thirds of a main
				// pass): ask for them now, so that the answer is there when the next step starts — asked for right after
				// publishing, the loads came back with the old tags every time and the next step began with a full poll
				// round trip (1 200 - 1 700 cycles of a 6 400-cycle step).
				const unsigned long long done = (unsigned long long)ntag << 32;
				pre[0] = z_first ? __hip_atomic_load((const gu64 *)(mailbox(npar, t_zlo, RES_FACE_ZHI) + zt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
				pre[1] = z_last ? __hip_atomic_load((const gu64 *)(mailbox(npar, t_zhi, RES_FACE_ZLO) + zt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
#pragma unroll
				for (int k = 0; k < (int)FE; k++)
					pre[2 + k] = y_entry_active((u32)k) ? __hip_atomic_load(y_granule(npar, (u32)k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
				have_pre = true;
			}
		};
		if (!kPreAfterImage)
		{
			// "after the main pass" has to be said to the compiler: nothing but the image write reads the new words, so the pass's
			// arithmetic sank behind the branch inside prefetch_faces() and the request went out at the HEAD of the pass (up to round 5)
			if (CA3D_RES_PIN_PASS)
			{
#pragma unroll
				for (int p = 1; p < (int)PT - 1; p++) asm volatile("" : "+v"(s[p]));
				__builtin_amdgcn_sched_barrier(0);
			}
			prefetch_faces();
		}
		s[0] = n0;
		s[PT - 1] = nl;
		RES_STAMP(5);

		to_image(img ^ 1u);
		if (kPreAfterImage) prefetch_faces();
		RES_STAMP(6);
		if (tid == 0) __hip_atomic_store((gu32 *)a.status + 4u + tile, t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (t + 2u == a.steps)
		{
			// the other ping-pong buffer keeps the state one step earlier (main_pathtraced.js:1580-1609); with steps == 1
			// that is the input buffer itself
			u32 *dst = a.out_prev + ((size_t)(z0 + pz0) * G + (y0 + yl)) * C + x;
			asm volatile("" : "+v"(dst)); // opaque: otherwise the store addresses are hoisted out of the step loop and live (spilled) through it
#pragma unroll
			for (int p = 0; p < (int)PT; p++) dst[(size_t)p * G * C] = s[p];
		}
	}
#ifdef CA3D_RES_STAMPS
	if (tile == 37u && (tid == 0 || tid == NT / 2u))
		for (int i = 0; i < 7; i++) a.status[600 + (tid ? 8 : 0) + i] = (u32)(st_acc[i] / a.steps);
#endif
	u32 *dst = a.out_last + ((size_t)(z0 + pz0) * G + (y0 + yl)) * C + x;
#pragma unroll
	for (int p = 0; p < (int)PT; p++) dst[(size_t)p * G * C] = s[p];
}

// ----------------------------------------------------------------------------------------------------------------
// Row-pair form of the 512^3 kernel (round 3). The per-phase cycle counts of resident_run (tools/ubench/resident_probe, stamps
// build) put a quarter of a step into LDS traffic: a thread writes its 32 words and reads the 64 of the rows above and below.
// Here a thread owns word x of TWO adjacent rows for 16 planes (same 32 registers of state, same 512 threads: 16 words x 16
// row pairs x 2 z groups): each row's second y neighbour is the thread's other row — a register — so only 32 words are read
// (rows y-1 of the lower and y+1 of the upper row) plus the two words across the z split, a third less LDS traffic in all.
// Same tiles, image, mailboxes, tags and y-face pass as resident_run<32, 16, 32, *> (a launch of either form can follow one of
// the other); the z faces are two words per thread, of the z group that touches them.
// Where the faces of the next state are asked for ahead of the poll (round 4, per-wave phase stamps of this form and a count of the
// polls that found an old tag: tools/ubench/resident_probe.hip, mode 33, -DCA3D_RES_STAMPS). An agent-scope load of a granule another
// XCD has just written takes 1 250 - 1 350 cycles to answer, so a request that is made too early costs a whole second round trip and
// one that is made late leaves the wave waiting for it:
//   * the SECOND z group (the younger wave of every SIMD: it gets what issue slots its partner leaves and is the last to arrive at
//     the barrier) asks after plane CA3D_RES_PAIR_PRE of its main pass — pinned with scheduling barriers: left to itself the compiler
//     hoists the loads to the head of the pass, where the answer is stale in most steps. Planes 5 / 9 / 12 / 14 / behind the pass:
//     2.55 / 2.40 / 2.37 / 2.39 / 2.39 us per step (4 096-step launches), at plane 12 one request in a hundred comes back stale;
//   * the FIRST z group is through its main pass a thousand cycles before the partner, and whatever it asks ahead comes back stale
//     (95 % of the steps): CA3D_RES_PAIR_PRE0 = 2 lets it poll in the ordinary way behind the image write (stale 0 - 3 %, one round
//     trip, and it still waits ~1 100 cycles at the barrier for the partner): 2.351 -> 2.339 us; 1 (asking behind the image write
//     AND keeping the compiler from moving that): 2.46.
// What the compiler made of that placement (round 6, profiles/r6_a_resident_request_placement.txt). The scheduling barriers only order
// instructions inside one basic block, and the request sits behind branches (asks_ahead, !last). Once the step read one register set and
// wrote the other (round 4's last change), nothing but the image write read the new words: the arithmetic of planes 1 .. 12 sank behind
// the branch, only the (convergent) DPP moves stayed, and the emitted kernel asked BEFORE the first arithmetic instruction of the pass —
// with 48 fetched words live across the request, 216 VGPRs. The plane figures above and the stale counts were taken on the order the
// in-place step had; nothing measured the production order, the stamps build (RES_STAMP) changes what may move. Now the words of
// planes 1 .. CA3D_RES_PAIR_PRE are made opaque in front of the request (pin_planes: an empty asm volatile, CA3D_RES_PAIR_PIN): the
// request is emitted behind that many planes, each plane's DPP moves beside its arithmetic, 194 VGPRs, no spill; tests/
// test_resident_codegen.py reads that order out of the assembly. -DCA3D_RES_COUNT_STALE counts the first polls of a step that found an
// old tag without a stamp or a wait (one scalar add per poll, one store per wave at the end; resident_probe mode 33 prints it).
// The sweep on the emitted order (4 096-step launches, us per step): the order up to round 5 2.10 (and only 1 - 7 % of its first polls
// were stale: "stale in most steps" was not true of it); held, first group not asking, planes 5 / 9 / 12 / 14 / behind the pass:
// 1.99 / 2.00 / 1.99 / 2.00 / 1.99 — the plane no longer matters, what the 5 % buy is each plane's DPP moves beside its arithmetic;
// first group asking behind its image write (PRE0 = 1): 1.87 / 1.91 / 1.88 / 1.96 / 2.42, asking like the second (0): 2.15 / 2.04 /
// 2.09 / 2.20 / 2.20. Defaults: plane 5, PRE0 = 1. The figures of round 4 above belong to the order of their day.
// With the requests placed like this the static issue priority round 4 first gave the older half (s_setprio 1: 2.479 -> 2.385 with
// the compiler's placement) no longer matters (2.353 - 2.363 without, 2.357 - 2.379 with: CA3D_RES_PAIR_PRIO, off); priorities that
// alternate between the two waves during the main pass (per plane, per four planes, per half) cost 4 - 7 %.
// What the stamps say is left (cycles of a 5 200-cycle step, second group): face pass 610, row reads 630, z faces 520, main pass 2 350
// — 350 instructions; a wave issues at most one vector instruction per ~4.3 cycles, and this one only gets the slots the older
// wave leaves (its main pass: 1 510) —, image 450, poll 250, halo rows + barrier 450. Tried against that and not kept: the y faces
// formed by the first group alone, four words a thread (they leave 350 cycles later and a third of the partner's requests turn
// stale: 2.52); an uneven z split emulated by moving two / four planes of arithmetic from the younger to the older wave (2.38 / 2.63:
// the younger wave's pass does not get shorter, it is starved for as long as the older one computes); the give-up flag read after
// the face pass instead of right behind the barrier (no change); -amdgpu-sched-strategy=max-ilp / iterative-ilp (2.39 / 2.46).
#ifndef CA3D_RES_PAIR_PRE0
#define CA3D_RES_PAIR_PRE0 1 // first z group: 0 asks like the second, 1 asks behind the image write, 2 does not ask ahead (round 6, emitted order: 2.04 / 1.87 / 1.99 us)
#endif
#ifndef CA3D_RES_PAIR_PRE
#define CA3D_RES_PAIR_PRE 5 // the plane of the main pass after which the next faces are asked for (15: behind the pass)
#endif
#ifndef CA3D_RES_PAIR_PIN
#define CA3D_RES_PAIR_PIN 1 // 0: the arithmetic of the planes in front of the request is free to sink behind it (the order up to round 5)
#endif
#ifndef CA3D_RES_PAIR_LOADS_FIRST
#define CA3D_RES_PAIR_LOADS_FIRST 0
#endif
#ifndef CA3D_RES_PAIR_PRIO
#define CA3D_RES_PAIR_PRIO 0 // 1: static issue priority for the first z group
#endif
template <int LS, int LB>
__device__ __forceinline__ void resident_pair_run(const ResidentArgs &a, char *lds)
{
	constexpr u32 C = 16u, G = 512u, RY = 32u, PZ = 32u, TPAY = G / RY, TPAZ = G / PZ;
	constexpr u32 PT = 16u, TCH = PT / 4u, NCH = PZ / 4u, NT = 512u, ZF = C * RY, YF = C * PZ, FW = 512u;
	constexpr u32 kImage = (RY + 2u) * NCH * C * 16u;
	const u32 tile = blockIdx.x;
	if (res_must_skip(a, tile)) return;
	const u32 ty = tile % TPAY, tz = tile / TPAY;
	const u32 tid = threadIdx.x, x = tid & 15u, yq = (tid >> 4) & 15u, zh = tid >> 8; // word, row pair, z group (wave-uniform)
	const u32 r0 = 2u * yq;                                                            // tile rows r0 and r0 + 1
	const u32 y0 = ty * RY, z0 = tz * PZ, pz0 = zh * PT;
	const bool z_first = zh == 0u;                                                     // the other group is the last one
	u32 *side = reinterpret_cast<u32 *>(lds + 2u * kImage);
	u32 *abort_lds = side + 2u * 2u * 2u * C;

	const bool dead_ylo = ty == 0, dead_zlo = tz == 0;
	const u32 t_ylo = (ty == 0 ? TPAY - 1u : ty - 1u) + tz * TPAY, t_yhi = (ty + 1u == TPAY ? 0u : ty + 1u) + tz * TPAY;
	const u32 t_zlo = ty + (tz == 0 ? TPAZ - 1u : tz - 1u) * TPAY, t_zhi = ty + (tz + 1u == TPAZ ? 0u : tz + 1u) * TPAY;
	auto mailbox = [&](u32 parity, u32 t, u32 face) { return a.mail + (((size_t)parity * (TPAY * TPAZ) + t) * 4u + face) * FW; };
	const u32 zt0 = r0 * C + x; // my words of a z face: zt0 (row r0) and zt0 + C (row r0 + 1)
	if (CA3D_RES_PAIR_PRIO == 1 && zh == 0) __builtin_amdgcn_s_setprio(1);
	const bool asks_ahead = CA3D_RES_PAIR_PRE0 == 0 || zh == 1;

	u32 s[2][PT];
#pragma unroll
	for (int r = 0; r < 2; r++)
	{
		const u32 *src = a.in + ((size_t)(z0 + pz0) * G + (y0 + r0 + (u32)r)) * C + x;
#pragma unroll
		for (int p = 0; p < (int)PT; p++) s[r][p] = src[(size_t)p * G * C];
	}
	if (tid == 0) *abort_lds = 0;

	auto to_image = [&](const u32 (&sv)[2][PT], u32 img) __attribute__((always_inline)) {
		char *base = lds + img * kImage;
#pragma unroll
		for (int r = 0; r < 2; r++)
#pragma unroll
			for (int c = 0; c < (int)TCH; c++)
			{
				uint4 v;
				v.x = sv[r][4 * c]; v.y = sv[r][4 * c + 1]; v.z = sv[r][4 * c + 2]; v.w = sv[r][4 * c + 3];
				*reinterpret_cast<uint4 *>(base + res_chunk_off<NCH, C>(r0 + (u32)r + 1u, x, zh * TCH + (u32)c)) = v;
			}
	};
	to_image(s, 0);
	{
		const u32 tag0 = a.epoch0 + 1u, par0 = tag0 & 1u;
#pragma unroll
		for (int r = 0; r < 2; r++)
			res_store_granule(mailbox(par0, tile, z_first ? RES_FACE_ZLO : RES_FACE_ZHI) + zt0 + (u32)r * C, tag0, z_first ? s[r][0] : s[r][PT - 1]);
		if (yq == 0)
		{
#pragma unroll
			for (int p = 0; p < (int)PT; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YLO) + (pz0 + (u32)p) * C + x, tag0, s[0][p]);
		}
		if (yq == 15u)
		{
#pragma unroll
			for (int p = 0; p < (int)PT; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YHI) + (pz0 + (u32)p) * C + x, tag0, s[1][p]);
		}
	}

	// granules of a state this thread waits for: its two words of the z face its group touches, word `tid` of both y faces
	auto z_granule = [&](u32 parity, u32 r) {
		return (const gu64 *)(mailbox(parity, z_first ? t_zlo : t_zhi, z_first ? RES_FACE_ZHI : RES_FACE_ZLO) + zt0 + r * C);
	};
	auto y_granule = [&](u32 parity, u32 f) { return (const gu64 *)(mailbox(parity, f ? t_yhi : t_ylo, f ? RES_FACE_YLO : RES_FACE_YHI) + tid); };
	unsigned long long pre[4] = {0, 0, 0, 0};
	bool have_pre = false;
#ifdef CA3D_RES_STAMPS
	unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = 0; // as resident_run: cycles per phase, every wave of tile 37
	u32 stale = 0;
#elif defined(CA3D_RES_COUNT_STALE)
	u32 stale = 0; // first polls of a step that found an old tag — counted in the production instruction order: no stamp, no wait
#endif

	// One step: state t in `si`, state t + 1 into `so`. The step loop below calls it with the two register sets changing roles — written as
	// one in-place update (new words into a fresh quad of registers for the image's 16-byte stores, then back into the registers the
	// loop carries) every step ended in 31 v_mov, 6 % of its vector instructions.
	auto step = [&](const u32 t, const u32 (&si)[2][PT], u32 (&so)[2][PT]) __attribute__((always_inline)) -> bool {
		const u32 tag = a.epoch0 + t + 1u, par = tag & 1u, img = t & 1u;
		const bool last = t + 1u == a.steps;
#ifdef CA3D_RES_STAMPS
		st_prev = __builtin_amdgcn_s_memtime();
		__builtin_amdgcn_s_waitcnt(0xC07F);
#endif
		// ---- A. the neighbour faces of state t
		u32 zf[2], hy[2];
		{
			unsigned long long q[4] = {pre[0], pre[1], pre[2], pre[3]};
			unsigned long long t_start = 0;
			for (u32 spins = 0;; spins++)
			{
				if (spins || !have_pre)
				{
					q[0] = __hip_atomic_load(z_granule(par, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					q[1] = __hip_atomic_load(z_granule(par, 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					q[2] = __hip_atomic_load(y_granule(par, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					q[3] = __hip_atomic_load(y_granule(par, 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
				// a dead face is waited for like a live one and its data dropped (resident_run)
				zf[0] = (z_first && dead_zlo) ? 0u : (u32)q[0];
				zf[1] = (z_first && dead_zlo) ? 0u : (u32)q[1];
				hy[0] = dead_ylo ? 0u : (u32)q[2];
				hy[1] = (u32)q[3];
				const bool ok = (u32)(q[0] >> 32) == tag && (u32)(q[1] >> 32) == tag && (u32)(q[2] >> 32) == tag && (u32)(q[3] >> 32) == tag;
#ifdef CA3D_RES_NO_WAIT
				break;
#endif
#ifdef CA3D_RES_STAMPS
				if (!__all(ok)) stale++; // polls that found an old tag
#ifdef CA3D_RES_STAMPS_POLL
				if (spins == 0) { __builtin_amdgcn_sched_barrier(0); RES_STAMP(7); __builtin_amdgcn_sched_barrier(0); } // the answer to the request made ahead is there
#endif
#elif defined(CA3D_RES_COUNT_STALE)
				if (spins == 0 && !__all(ok)) stale++;
#endif
				if (__all(ok)) break;
				if ((spins & 63u) == 63u)
				{
					const unsigned long long now = __builtin_amdgcn_s_memrealtime();
					if (t_start == 0) t_start = now;
					const bool expired = now - t_start > a.timeout_ticks;
					const u32 other = __hip_atomic_load((const gu32 *)a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (expired || other)
					{
						if (expired && !other && (tid & 63u) == 0) res_report_timeout(a, tile);
						if ((tid & 63u) == 0) *abort_lds = 1;
						break;
					}
				}
				if (spins) __builtin_amdgcn_s_sleep(1);
			}
		}
		RES_STAMP(0);
		// ---- B. halo rows of the image (word `tid` = plane tid / 16, word x of each y face); the planes below / above rows 0 and 31
		{
			char *base = lds + img * kImage;
			const u32 hp = tid >> 4;
			*reinterpret_cast<u32 *>(base + res_chunk_off<NCH, C>(0u, x, hp >> 2) + (hp & 3u) * 4u) = hy[0];
			*reinterpret_cast<u32 *>(base + res_chunk_off<NCH, C>(RY + 1u, x, hp >> 2) + (hp & 3u) * 4u) = hy[1];
			// side: [lo | hi][row 0 | row 31][x]; row 0 is the first row of pair 0, row 31 the second row of pair 15
			if (yq == 0) side[img * (4u * C) + (z_first ? 0u : 2u * C) + x] = zf[0];
			if (yq == 15u) side[img * (4u * C) + (z_first ? 0u : 2u * C) + C + x] = zf[1];
		}
		__syncthreads();
		if (*abort_lds) return false;
		RES_STAMP(1);

		const char *im = lds + img * kImage;
		const u32 ntag = tag + 1u, npar = ntag & 1u;
#if CA3D_RES_PAIR_LOADS_FIRST
		// ---- C. every LDS read of the step back to back — the words of the y-face pass (word `tid` of the lower and of the upper face, as
		// resident_run), the rows below / above my pair, my rows across the z split — and only then the arithmetic: with the face pass
		// inside `if (!last)` the reads of the rows could not be issued before the pass's two round trips were over
		u32 fw[2], fm[2], fq[2], fb[2], fa[2];
#pragma unroll
		for (int f = 0; f < 2; f++)
		{
			const u32 fp = tid >> 4, ch = fp >> 2, wi = (fp & 3u) * 4u;
			const u32 fpm = fp ? fp - 1u : 0u, fpp = fp < PZ - 1u ? fp + 1u : PZ - 1u;
			const u32 row = f ? RY : 1u;
			fw[f] = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, x, ch) + wi);
			fm[f] = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row - 1u, x, ch) + wi);
			fq[f] = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row + 1u, x, ch) + wi);
			const u32 *sd = side + img * (4u * C) + (f ? C : 0u) + x;
			fb[f] = fp ? *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, x, fpm >> 2) + (fpm & 3u) * 4u) : sd[0];
			fa[f] = fp < PZ - 1u ? *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, x, fpp >> 2) + (fpp & 3u) * 4u) : sd[2u * C];
		}
		u32 ym[PT], yp[PT];
#pragma unroll
		for (int c = 0; c < (int)TCH; c++)
		{
			const uint4 m = *reinterpret_cast<const uint4 *>(im + res_chunk_off<NCH, C>(r0, x, zh * TCH + (u32)c));       // tile row r0 - 1
			const uint4 q = *reinterpret_cast<const uint4 *>(im + res_chunk_off<NCH, C>(r0 + 3u, x, zh * TCH + (u32)c));  // tile row r0 + 2
			ym[4 * c] = m.x; ym[4 * c + 1] = m.y; ym[4 * c + 2] = m.z; ym[4 * c + 3] = m.w;
			yp[4 * c] = q.x; yp[4 * c + 1] = q.y; yp[4 * c + 2] = q.z; yp[4 * c + 3] = q.w;
		}
		u32 bf[2], al[2]; // the plane below my first / above my last plane, per row: the neighbour tile's face or the other group's plane
#pragma unroll
		for (int r = 0; r < 2; r++)
		{
			const u32 across = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(r0 + (u32)r + 1u, x, z_first ? TCH : TCH - 1u) + (z_first ? 0u : 12u)); // plane 16 / plane 15
			bf[r] = z_first ? zf[r] : across;
			al[r] = z_first ? across : zf[r];
		}
#pragma unroll
		for (int f = 0; f < 2; f++)
		{
			const u32 o = res_rule<LS, LB>(fw[f], res_left(fw[f]), res_right(fw[f]), fm[f], fq[f], fb[f], fa[f]);
			if (!last) res_store_granule(mailbox(npar, tile, f ? RES_FACE_YHI : RES_FACE_YLO) + tid, ntag, o);
		}
		RES_STAMP(2);
#else
		// ---- C. the y faces of state t + 1 first (as resident_run: word `tid` of the lower and of the upper face)
		if (!last)
#pragma unroll
		for (int f = 0; f < 2; f++)
		{
			const u32 fp = tid >> 4, ch = fp >> 2, wi = (fp & 3u) * 4u;
			const u32 fpm = fp ? fp - 1u : 0u, fpp = fp < PZ - 1u ? fp + 1u : PZ - 1u;
			const u32 row = f ? RY : 1u;
			const u32 w = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, x, ch) + wi);
			const u32 fym = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row - 1u, x, ch) + wi);
			const u32 fyp = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row + 1u, x, ch) + wi);
			const u32 *sd = side + img * (4u * C) + (f ? C : 0u) + x;
			const u32 below = fp ? *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, x, fpm >> 2) + (fpm & 3u) * 4u) : sd[0];
			const u32 above = fp < PZ - 1u ? *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(row, x, fpp >> 2) + (fpp & 3u) * 4u) : sd[2u * C];
			const u32 o = res_rule<LS, LB>(w, res_left(w), res_right(w), fym, fyp, below, above);
			res_store_granule(mailbox(npar, tile, f ? RES_FACE_YHI : RES_FACE_YLO) + tid, ntag, o);
		}

		RES_STAMP(2);
		// ---- the row below my lower row and the row above my upper row (16 planes each); my rows across the z split
		u32 ym[PT], yp[PT];
#pragma unroll
		for (int c = 0; c < (int)TCH; c++)
		{
			const uint4 m = *reinterpret_cast<const uint4 *>(im + res_chunk_off<NCH, C>(r0, x, zh * TCH + (u32)c));       // tile row r0 - 1
			const uint4 q = *reinterpret_cast<const uint4 *>(im + res_chunk_off<NCH, C>(r0 + 3u, x, zh * TCH + (u32)c));  // tile row r0 + 2
			ym[4 * c] = m.x; ym[4 * c + 1] = m.y; ym[4 * c + 2] = m.z; ym[4 * c + 3] = m.w;
			yp[4 * c] = q.x; yp[4 * c + 1] = q.y; yp[4 * c + 2] = q.z; yp[4 * c + 3] = q.w;
		}
		u32 bf[2], al[2]; // the plane below my first / above my last plane, per row: the neighbour tile's face or the other group's plane
#pragma unroll
		for (int r = 0; r < 2; r++)
		{
			const u32 across = *reinterpret_cast<const u32 *>(im + res_chunk_off<NCH, C>(r0 + (u32)r + 1u, x, z_first ? TCH : TCH - 1u) + (z_first ? 0u : 12u)); // plane 16 / plane 15
			bf[r] = z_first ? zf[r] : across;
			al[r] = z_first ? across : zf[r];
		}

#endif
		RES_STAMP(3);
		// ---- D. one step in place, both rows plane by plane (each row's other y neighbour is the old word of the other row)
		u32 n0[2], nl[2];
		n0[0] = res_rule<LS, LB>(si[0][0], res_left(si[0][0]), res_right(si[0][0]), ym[0], si[1][0], bf[0], si[0][1]);
		n0[1] = res_rule<LS, LB>(si[1][0], res_left(si[1][0]), res_right(si[1][0]), si[0][0], yp[0], bf[1], si[1][1]);
		nl[0] = res_rule<LS, LB>(si[0][PT - 1], res_left(si[0][PT - 1]), res_right(si[0][PT - 1]), ym[PT - 1], si[1][PT - 1], si[0][PT - 2], al[0]);
		nl[1] = res_rule<LS, LB>(si[1][PT - 1], res_left(si[1][PT - 1]), res_right(si[1][PT - 1]), si[0][PT - 1], yp[PT - 1], si[1][PT - 2], al[1]);
		if (!last)
		{
#pragma unroll
			for (int r = 0; r < 2; r++)
				res_store_granule(mailbox(npar, tile, z_first ? RES_FACE_ZLO : RES_FACE_ZHI) + zt0 + (u32)r * C, ntag, z_first ? n0[r] : nl[r]);
		}
		__builtin_amdgcn_sched_barrier(0);
		RES_STAMP(4);
		auto prefetch_faces = [&]() {
			if (!last)
			{
				// ask for the neighbours' faces of state t + 1: they were published about as long ago as mine (resident_run)
				pre[0] = __hip_atomic_load(z_granule(npar, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				pre[1] = __hip_atomic_load(z_granule(npar, 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				pre[2] = __hip_atomic_load(y_granule(npar, 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				pre[3] = __hip_atomic_load(y_granule(npar, 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				have_pre = true;
			}
		};
		// the words of planes 1 .. n are made before what follows (see above resident_pair_run: CA3D_RES_PAIR_PIN)
		auto pin_planes = [&](int n) __attribute__((always_inline)) {
#pragma unroll
			for (int q = 1; q <= n; q++) asm volatile("" : "+v"(so[0][q]), "+v"(so[1][q]));
		};
#pragma unroll
		for (int p = 1; p < (int)PT - 1; p++)
		{
			const u32 w0 = si[0][p], w1 = si[1][p];
			so[0][p] = res_rule<LS, LB>(w0, res_left(w0), res_right(w0), ym[p], w1, si[0][p - 1], si[0][p + 1]);
			so[1][p] = res_rule<LS, LB>(w1, res_left(w1), res_right(w1), w0, yp[p], si[1][p - 1], si[1][p + 1]);
			if (p == CA3D_RES_PAIR_PRE && asks_ahead)
			{
				if (CA3D_RES_PAIR_PIN) pin_planes(p);
				__builtin_amdgcn_sched_barrier(0);
				prefetch_faces();
				__builtin_amdgcn_sched_barrier(0);
			}
		}
		if (CA3D_RES_PAIR_PRE >= (int)PT - 1 && asks_ahead)
		{
			if (CA3D_RES_PAIR_PIN) pin_planes((int)PT - 2);
			__builtin_amdgcn_sched_barrier(0);
			prefetch_faces();
			__builtin_amdgcn_sched_barrier(0);
		}
		so[0][0] = n0[0]; so[1][0] = n0[1];
		so[0][PT - 1] = nl[0]; so[1][PT - 1] = nl[1];
		RES_STAMP(5);

		to_image(so, img ^ 1u);
		if (CA3D_RES_PAIR_PRE0 == 1 && zh == 0)
		{
			__builtin_amdgcn_sched_barrier(0);
			prefetch_faces();
			__builtin_amdgcn_sched_barrier(0);
		}
		RES_STAMP(6);
		if (tid == 0) __hip_atomic_store((gu32 *)a.status + 4u + tile, t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (t + 2u == a.steps)
		{
#pragma unroll
			for (int r = 0; r < 2; r++)
			{
				u32 *dst = a.out_prev + ((size_t)(z0 + pz0) * G + (y0 + r0 + (u32)r)) * C + x;
				asm volatile("" : "+v"(dst)); // opaque: see resident_run
#pragma unroll
				for (int p = 0; p < (int)PT; p++) dst[(size_t)p * G * C] = so[r][p];
			}
		}
			return true;
	};
	u32 s2[2][PT];
	u32 t_done = 0;
	for (; t_done + 1u < a.steps; t_done += 2u)
	{
		if (!step(t_done, s, s2)) return;
		if (!step(t_done + 1u, s2, s)) return;
	}
	const bool odd_tail = t_done < a.steps; // one more step, which leaves the final state in the second set
	if (odd_tail)
	{
		if (!step(t_done, s, s2)) return;
#pragma unroll
		for (int r = 0; r < 2; r++)
#pragma unroll
			for (int p = 0; p < (int)PT; p++) s[r][p] = s2[r][p]; // (by value, once: a select between the two arrays' addresses would put both into scratch)
	}
#ifdef CA3D_RES_STAMPS
	if (tile == 37u && (tid & 63u) == 0) // every wave of the tile
	{
		for (int i = 0; i < 8; i++) a.status[600 + (tid >> 6) * 8 + i] = (u32)(st_acc[i] / a.steps);
		a.status[680 + (tid >> 6)] = (u32)((unsigned long long)stale * 1000u / a.steps);
	}
#elif defined(CA3D_RES_COUNT_STALE)
	if (tile == 37u && (tid & 63u) == 0) a.status[680 + (tid >> 6)] = (u32)((unsigned long long)stale * 1000u / a.steps); // every wave of the tile
#endif
#pragma unroll
	for (int r = 0; r < 2; r++)
	{
		u32 *dst = a.out_last + ((size_t)(z0 + pz0) * G + (y0 + r0 + (u32)r)) * C + x;
#pragma unroll
		for (int p = 0; p < (int)PT; p++) dst[(size_t)p * G * C] = s[r][p];
	}
}

// ----------------------------------------------------------------------------------------------------------------
// Two more forms of these kernels were built, measured and — having lost twice — REMOVED in round 5 (the code is in the git history up to
// round 4; DESIGN.md 4.7 and 10 keep the measurements):
//   * the STAGGERED row-pair form (round 4: the two z groups of a 512^3 tile half a step apart, so that one wave's LDS / poll phases lie
//     beside its SIMD partner's arithmetic): 2.356 us per step against the row-pair form's 2.35 — staggering moved the idle time, it did
//     not remove it: what a wave does between two barriers is a dependent chain whose length the partner's phase does not change;
//   * the two-steps-per-hand-off form at 256^3 (round 3: faces two cells deep every second step, the step in between on the tile plus a
//     one-cell ring): 1.38-1.52 us per step against 1.27 — twice the face payload and a longer chain in front of every request cost
//     more than the halved hand-off count saved.

// ----------------------------------------------------------------------------------------------------------------
// 64^3 — the reference UI's start-up grid (main_pathtraced.js:101) — in ONE workgroup (round 5). The per-step kernels step it in
// 1.85 us: the launch floor, 0.005 of the HBM figure. Its state is 32 KiB: 1 024 threads hold it in eight registers each — lane = row y,
// wave w = planes 4 w .. 4 w + 3, a row's two words side by side in one thread — and nothing leaves the CU between the load and the
// store of a launch: x neighbours are the thread's own other word (v_alignbit; x == -1 dead, x == 64 wraps to the row's first word),
// y neighbours the lanes either side by wave-wide DPP (wave_shr:1 with a zero shifted in at row 0: y == -1 is dead; wave_rol:1: row 63's
// upper neighbour is row 0), z neighbours the thread's own planes and, at a wave's first and last plane, the neighbouring waves'
// through a double-buffered exchange in LDS with ONE barrier per step (wave 0 has nothing below it: z == -1 is dead; wave 15's plane
// above is wave 0's first: z == 64 wraps). No mailboxes, no tags, no waits that can time out: ResidentArgs' mail / status / epoch are
// unused. One CU is 1 / 256 of the chip's arithmetic — 8 words x ~12 instructions per thread and step on four waves per SIMD — so this
// pays for the von Neumann table rules at THIS grid only (DESIGN.md 11.5: at 128^3 the same arithmetic on one CU takes longer than a
// launch of the whole chip, and a rule with diagonal classes is slower than its per-step kernel already here).
// Measured: 0.655 us per step in batches of 256 and more (0.91 at 8) against the rows kernel's 1.79-1.81 (3.5 at 8): ~100 instructions per
// wave and step, a third of them half-rate (DPP moves, v_alignbit), four waves per SIMD — the CU's issue rate. Computing the two planes
// that need nothing from another wave BEFORE the barrier took it from 0.706 to 0.655; eight planes per wave (512 threads) 0.662.
constexpr u32 kRes64LdsBytes = 2u * 16u * 2u * 2u * 64u * 4u; // [step parity][wave][first / last plane][word][row]

template <int LS, int LB, int PT_ = 4>
__device__ __forceinline__ void resident64_run(const ResidentArgs &a, char *lds)
{
	constexpr u32 G = 64u, PT = (u32)PT_, NW = 64u / PT; // planes per wave, waves
	const u32 tid = threadIdx.x, row = tid & 63u, wave = tid >> 6;
	u32 *xch = reinterpret_cast<u32 *>(lds);
	auto slot = [&](u32 buf, u32 w, u32 which, u32 h) { return (((buf * NW + w) * 2u + which) * 2u + h) * 64u + row; };
	u32 s[PT][2];
#pragma unroll
	for (u32 p = 0; p < PT; p++)
	{
		const uint2 v = *reinterpret_cast<const uint2 *>(a.in + ((size_t)((wave * PT + p) * G + row)) * 2u);
		s[p][0] = v.x;
		s[p][1] = v.y;
	}
	for (u32 step = 0; step < a.steps; step++)
	{
		const u32 buf = step & 1u;
		xch[slot(buf, wave, 0u, 0u)] = s[0][0];
		xch[slot(buf, wave, 0u, 1u)] = s[0][1];
		xch[slot(buf, wave, 1u, 0u)] = s[PT - 1][0];
		xch[slot(buf, wave, 1u, 1u)] = s[PT - 1][1];
		if (step + 1u == a.steps && a.steps >= 2u) // the state one step before the last: the other ping-pong buffer
		{
#pragma unroll
			for (u32 p = 0; p < PT; p++) *reinterpret_cast<uint2 *>(a.out_prev + ((size_t)((wave * PT + p) * G + row)) * 2u) = make_uint2(s[p][0], s[p][1]);
		}
		u32 n[PT][2];
		auto plane = [&](u32 p, const u32 (&bl)[2], const u32 (&ab)[2]) {
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				const u32 w = s[p][h], other = s[p][h ^ 1u];
				const u32 l = from_left(w, h ? other : 0u); // cell x - 1: word 0's comes from nowhere (dead), word 1's from word 0
				const u32 r = from_right(other, w);         // cell x + 1: word 0's from word 1, word 1's from word 0 (x == 64 wraps)
				const u32 ym = dpp_mov<kDppWaveShr1>(w);    // row y - 1 (zero into row 0)
				const u32 yp = dpp_mov<kDppWaveRol1>(w);    // row y + 1 (row 0 into row 63)
				n[p][h] = res_rule<LS, LB>(w, l, r, ym, yp, bl[h], ab[h]);
			}
		};
		// the planes that need nothing from another wave first: the exchange's LDS writes and the other waves' arrival at the barrier
		// lie behind half of the step's arithmetic
#pragma unroll
		for (u32 p = 1; p + 1u < PT; p++) plane(p, s[p - 1], s[p + 1]);
		__syncthreads();
		u32 below[2], above[2];
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			below[h] = wave ? xch[slot(buf, wave - 1u, 1u, h)] : 0u; // z == -1 is dead
			above[h] = xch[slot(buf, (wave + 1u) & (NW - 1u), 0u, h)]; // z == 64 is plane 0
		}
		plane(0u, below, s[1]);
		plane(PT - 1u, s[PT - 2], above);
#pragma unroll
		for (u32 p = 0; p < PT; p++) { s[p][0] = n[p][0]; s[p][1] = n[p][1]; }
	}
#pragma unroll
	for (u32 p = 0; p < PT; p++) *reinterpret_cast<uint2 *>(a.out_last + ((size_t)((wave * PT + p) * G + row)) * 2u) = make_uint2(s[p][0], s[p][1]);
}

#if defined(CA3D_JIT) && defined(CA3D_JIT_LS) && !defined(CA3D_JIT_SLAB_PZ)
// entry points: <rows per tile>[_z2: two thread groups along z = twice the threads, four waves per SIMD where one group gives two]
#define CA3D_RES_ENTRY(NAME_, THREADS_, WAVES_, ...)                                                   \
	extern "C" __global__ __launch_bounds__(THREADS_, WAVES_) void NAME_(ResidentArgs a)              \
	{                                                                                                  \
		__shared__ __attribute__((aligned(16))) char res_lds[ResidentLds<__VA_ARGS__>::bytes]; /* static: no dynamic-LDS opt-in needed above 64 KiB */ \
		resident_run<CA3D_JIT_LS, CA3D_JIT_LB, __VA_ARGS__>(a, res_lds);                               \
	}
CA3D_RES_ENTRY(ca3d_jit_resident, 512, 2, 32, 16, 32, 1)
CA3D_RES_ENTRY(ca3d_jit_resident_z2, 1024, 4, 32, 16, 32, 2)
CA3D_RES_ENTRY(ca3d_jit_resident16, 256, 2, 16, 16, 32, 1)
CA3D_RES_ENTRY(ca3d_jit_resident16_z2, 512, 4, 16, 16, 32, 2)
CA3D_RES_ENTRY(ca3d_jit_resident256, 256, 1, 32, 8, 8, 1)      // 256^3: 8 words x 32 rows x 8 planes per tile
CA3D_RES_ENTRY(ca3d_jit_resident256_z2, 512, 2, 32, 8, 8, 2)
#undef CA3D_RES_ENTRY
extern "C" __global__ __launch_bounds__(512, 2) void ca3d_jit_resident_pair(ResidentArgs a) // row-pair form, 512^3
{
	__shared__ __attribute__((aligned(16))) char res_lds[ResidentLds<32, 16, 32, 1>::bytes];
	resident_pair_run<CA3D_JIT_LS, CA3D_JIT_LB>(a, res_lds);
}
extern "C" __global__ __launch_bounds__(1024, 4) void ca3d_jit_resident64(ResidentArgs a) // 64^3 in one workgroup
{
	__shared__ __attribute__((aligned(16))) char res_lds[kRes64LdsBytes];
	resident64_run<CA3D_JIT_LS, CA3D_JIT_LB>(a, res_lds);
}
#elif !defined(CA3D_JIT)
// second launch-bounds argument: waves per SIMD the launch NEEDS to be resident as a whole — without it the compiler is free to
// take more registers than that allows, and a launch that is not fully resident waits for itself
template <int LS, int LB, int RY, int ZS>
__global__ __launch_bounds__(16 * RY * ZS, 2 * ZS) void ca_resident_vn(ResidentArgs a)
{
	__shared__ __attribute__((aligned(16))) char res_lds[ResidentLds<RY, 16, 32, ZS>::bytes];
	resident_run<LS, LB, RY, 16, 32, ZS>(a, res_lds);
}
template <int LS, int LB>
__global__ __launch_bounds__(512, 2) void ca_resident_vn_pair(ResidentArgs a) // row-pair form, 512^3
{
	__shared__ __attribute__((aligned(16))) char res_lds[ResidentLds<32, 16, 32, 1>::bytes];
	resident_pair_run<LS, LB>(a, res_lds);
}
template <int LS, int LB, int PT>
__global__ __launch_bounds__(4096 / PT, 16 / PT) void ca_resident_vn64(ResidentArgs a) // 64^3 in one workgroup
{
	__shared__ __attribute__((aligned(16))) char res_lds[kRes64LdsBytes];
	resident64_run<LS, LB, PT>(a, res_lds);
}
template <int LS, int LB, int ZS>
__global__ __launch_bounds__(256 * ZS, ZS) void ca_resident_vn256(ResidentArgs a) // 256^3
{
	__shared__ __attribute__((aligned(16))) char res_lds[ResidentLds<32, 8, 8, ZS>::bytes];
	resident_run<LS, LB, 32, 8, 8, ZS>(a, res_lds);
}
#endif

// ================================================================================================================
// Slab form: K sub-steps of one rank's Z-slab of a 1024^3 grid (multi-GPU runs, SURVEY 8(e)) in one launch. The array
// is L = nz + 2 * ghost planes of 1024 x 1024 cells (32 words per row); 256 tiles of 32 rows x PZ = L / 8 planes, one
// 1024-thread workgroup each (a thread owns word x of row y for PZ planes). Differences from the full-grid form above:
//   * a row is two DPP rows: the word to the left comes by wave_shr:1 (masked at x == 0), the word to the right by
//     ds_bpermute (lane + 1, wrapping inside the 32 lanes of the row);
//   * LDS holds ONE image (two would not fit beside 1024 threads): a second barrier separates the step's reads of the
//     image from the writes of the new rows;
//   * the array has two ends: the tiles at either end have no z neighbour there (the outermost ghost planes go stale one
//     plane per sub-step, which is what the ghost depth is for), rows wrap in y as everywhere;
//   * every plane is updated in every sub-step; the plane whose global z is 0 (the owned plane 0 of rank 0, or its copy
//     in the top rank's high ghost) has a dead plane below it — a run-time plane index.
struct ResidentSlabArgs
{
	const u32 *in;            // L planes (buffer `cur` of the slab engine)
	u32 *out;                 // L planes: the state after `steps` sub-steps
	unsigned long long *mail; // granules [2 parities][256 tiles][4 faces][1024]
	u32 *status;
	u32 *host_flag;
	u32 steps, epoch0, timeout_ticks;
	int dead_plane; // array plane whose global z is 0 (the plane below it is dead), or -1
};

#ifndef CA3D_SLAB_LATE_PREFETCH
#define CA3D_SLAB_LATE_PREFETCH(PZ) ((2 * (PZ)) / 3) // kLate: the plane of the main pass after which the next faces are asked for
#endif
#ifndef CA3D_SLAB_LATE_FROM
#define CA3D_SLAB_LATE_FROM 16 // planes per tile layer above which the rows beside a thread's own are read inside the pass (kLate); measured at 20 / 24 planes (an eighth of 1024^3, K = 16 / 32): 4.77 / 4.64 us per step with, 4.87 / 5.09 without (at 24 the early-read form spills 3 registers under the run-time compiler torch ships)
#endif
#ifndef CA3D_SLAB_LOOKAHEAD
#define CA3D_SLAB_LOOKAHEAD 0 // kLate: 1 asks for the rows of a chunk of four planes while the chunk before it is computed
#endif
#ifndef CA3D_SLAB_PREFETCH_PLANE
#define CA3D_SLAB_PREFETCH_PLANE 8
#endif
constexpr int kSlabCW = 32, kSlabTY = 32, kSlabTZ = 8, kSlabThreads = 1024;
constexpr int kSlabMaxPZ = 36;                 // planes per tile layer the kernel is built for (LDS: 34 rows x 9 chunks x 512 B = 153 KB)
constexpr int kSlabFace = kSlabMaxPZ * kSlabCW; // granules per mailbox face: a z face is 32 rows x 32 words = 1024, a y face PZ planes x 32 words

__device__ __forceinline__ u32 slab_chunk_off(u32 row, u32 x, u32 chunk, u32 nchunks) { return ((row * nchunks + chunk) * 32u + x) * 16u; }

template <int LS, int LB, int PZ>
__device__ __forceinline__ void resident_slab_run(const ResidentSlabArgs &a, char *lds)
{
	constexpr u32 C = kSlabCW, G = 1024u, NCH = (PZ + 3) / 4;
	static_assert(PZ >= 4 && PZ <= kSlabMaxPZ && PZ % 2 == 0, "planes per tile layer: even (the face pass runs whole waves), a y face fits its mailbox");
	constexpr u32 YF = (u32)PZ * 32u;                                   // words of a y face
	constexpr u32 FE = (YF + (u32)kSlabThreads - 1u) / (u32)kSlabThreads; // y-face words per thread and face: entry k is word tid + 1024 k (plane 32 k + tid / 32, word tid % 32)
	constexpr u32 kImage = 34u * NCH * 32u * 16u;
	// Many planes per thread (round 4: a rank's share of 1024^3 over FOUR ranks, 256 + 2 K planes -> 34 / 36 per tile layer): the state
	// alone is then 36 registers of the 128 that four waves per SIMD leave, and the rows y-1 / y+1 of every plane (72 more) cannot be
	// held beside it. kLate: those rows are read four planes at a time INSIDE the main pass and the barrier that separates the step's
	// reads of the image from the writes of the new rows moves behind the pass. The 8-rank shapes (20 / 24 planes) run this way too
	// since it measured faster there (CA3D_SLAB_LATE_FROM).
	constexpr bool kLate = PZ > CA3D_SLAB_LATE_FROM;
	constexpr int kSlabPrefetchPlane = kLate ? CA3D_SLAB_LATE_PREFETCH(PZ) : CA3D_SLAB_PREFETCH_PLANE;
	const u32 tile = blockIdx.x;
	const u32 ty = tile % kSlabTY, tz = tile / kSlabTY;
	const u32 tid = threadIdx.x, x = tid & 31u, yl = tid >> 5;
	const int lane = (int)(tid & 63u);
	const u32 y0 = ty * 32u, z0 = tz * PZ;
	u32 *side = reinterpret_cast<u32 *>(lds + kImage); // [lo|hi][row 0|31][x]
	u32 *abort_lds = side + 2u * 2u * 32u;

	const bool dead_ylo = ty == 0, end_zlo = tz == 0, end_zhi = tz == kSlabTZ - 1;
	const u32 t_ylo = (ty == 0 ? kSlabTY - 1u : ty - 1u) + tz * kSlabTY, t_yhi = (ty + 1u == kSlabTY ? 0u : ty + 1u) + tz * kSlabTY;
	const u32 t_zlo = ty + (end_zlo ? 0u : tz - 1u) * kSlabTY, t_zhi = ty + (end_zhi ? tz : tz + 1u) * kSlabTY;
	auto mailbox = [&](u32 parity, u32 t, u32 face) { return a.mail + (((size_t)parity * (kSlabTY * kSlabTZ) + t) * 4u + face) * kSlabFace; };
	// the plane of THIS tile whose plane below is dead (-1: none)
	const int dead_p = a.dead_plane >= (int)z0 && a.dead_plane < (int)(z0 + PZ) ? a.dead_plane - (int)z0 : -1;

	u32 xmask = x == 0 ? 0u : 0xFFFFFFFFu; // x-1 is dead at x == 0
	asm volatile("" : "+v"(xmask));
	const int right_lane = (lane & 32) | ((lane + 1) & 31); // the row's next word, word 0 after word 31
	auto left_of = [&](u32 w) { return from_left(w, dpp_mov<kDppWaveShr1>(w) & xmask); };
	auto right_of = [&](u32 w) { return from_right((u32)__builtin_amdgcn_ds_bpermute(right_lane << 2, (int)w), w); };

	u32 s[PZ];
	{
		const u32 *src = a.in + ((size_t)z0 * G + (y0 + yl)) * C + x;
#pragma unroll
		for (int p = 0; p < PZ; p++) s[p] = src[(size_t)p * G * C];
	}
	if (tid == 0) *abort_lds = 0;

	auto to_image = [&]() {
#pragma unroll
		for (int c = 0; c < (int)NCH; c++)
		{
			uint4 v;
			v.x = s[4 * c];
			v.y = 4 * c + 1 < PZ ? s[4 * c + 1 < PZ ? 4 * c + 1 : 0] : 0u;
			v.z = 4 * c + 2 < PZ ? s[4 * c + 2 < PZ ? 4 * c + 2 : 0] : 0u;
			v.w = 4 * c + 3 < PZ ? s[4 * c + 3 < PZ ? 4 * c + 3 : 0] : 0u;
			*reinterpret_cast<uint4 *>(lds + slab_chunk_off(yl + 1u, x, (u32)c, NCH)) = v;
		}
	};
	to_image();
	{
		const u32 tag0 = a.epoch0 + 1u, par0 = tag0 & 1u;
		res_store_granule(mailbox(par0, tile, RES_FACE_ZLO) + tid, tag0, s[0]);
		res_store_granule(mailbox(par0, tile, RES_FACE_ZHI) + tid, tag0, s[PZ - 1]);
		if (yl == 0)
		{
#pragma unroll
			for (int p = 0; p < PZ; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YLO) + (u32)p * 32u + x, tag0, s[p]);
		}
		if (yl == 31)
		{
#pragma unroll
			for (int p = 0; p < PZ; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YHI) + (u32)p * 32u + x, tag0, s[p]);
		}
	}

	unsigned long long pre[2 + 2 * FE];
#pragma unroll
	for (int k = 0; k < 2 + 2 * (int)FE; k++) pre[k] = 0;
	bool have_pre = false;
	for (u32 t = 0; t < a.steps; t++)
	{
		// The thread index as the loop body sees it, opaque: what the y-face duties derive from it (mailbox addresses, image offsets of up to
		// two face words per thread) is then formed again in every step instead of being carried through the pass in registers the pass
		// has no room for (36 planes: 10 registers spilled otherwise).
		u32 tl = tid;
		asm volatile("" : "+v"(tl));
		auto face_entry = [&](u32 k) { return tl + (u32)kSlabThreads * k < YF; }; // (whole waves: YF is a multiple of 64)
		const u32 tag = a.epoch0 + t + 1u, par = tag & 1u;
		const bool last = t + 1u == a.steps;
		const gu64 *g_zlo = (const gu64 *)(mailbox(par, t_zlo, RES_FACE_ZHI) + tl);
		const gu64 *g_zhi = (const gu64 *)(mailbox(par, t_zhi, RES_FACE_ZLO) + tl);
		const gu64 *g_ylo = (const gu64 *)(mailbox(par, t_ylo, RES_FACE_YHI) + tl);
		const gu64 *g_yhi = (const gu64 *)(mailbox(par, t_yhi, RES_FACE_YLO) + tl);
		u32 zlo = 0, zhi = 0, hlo[FE], hhi[FE];
		{
			const unsigned long long done = (unsigned long long)tag << 32; // stands for a face nobody has to wait for
			unsigned long long q0 = pre[0], q1 = pre[1], q2[FE], q3[FE];
#pragma unroll
			for (int k = 0; k < (int)FE; k++) { q2[k] = pre[2 + 2 * k]; q3[k] = pre[3 + 2 * k]; }
			unsigned long long t_start = 0;
			for (u32 spins = 0;; spins++)
			{
				if (spins || !have_pre)
				{
					// the array's ends have no tile beyond them; the dead y face IS waited for (its tile reads my face of this
					// state through the wrap: see the full-grid form)
					q0 = end_zlo ? done : __hip_atomic_load(g_zlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					q1 = end_zhi ? done : __hip_atomic_load(g_zhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
					for (int k = 0; k < (int)FE; k++)
					{
						q2[k] = face_entry((u32)k) ? __hip_atomic_load(g_ylo + (u32)kSlabThreads * (u32)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
						q3[k] = face_entry((u32)k) ? __hip_atomic_load(g_yhi + (u32)kSlabThreads * (u32)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					}
				}
				zlo = (u32)q0; zhi = (u32)q1;
				bool ok = (u32)(q0 >> 32) == tag && (u32)(q1 >> 32) == tag;
#pragma unroll
				for (int k = 0; k < (int)FE; k++)
				{
					hlo[k] = dead_ylo ? 0u : (u32)q2[k]; hhi[k] = (u32)q3[k];
					ok = ok && (u32)(q2[k] >> 32) == tag && (u32)(q3[k] >> 32) == tag;
				}
#ifdef CA3D_RES_NO_WAIT
				break;
#endif
				if (__all(ok)) break;
				if ((spins & 63u) == 63u)
				{
					const unsigned long long now = __builtin_amdgcn_s_memrealtime();
					if (t_start == 0) t_start = now;
					const bool expired = now - t_start > a.timeout_ticks;
					const u32 other = __hip_atomic_load((const gu32 *)a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (expired || other)
					{
						if (expired && !other && (tid & 63u) == 0)
						{
							__hip_atomic_store((gu32 *)a.status, tile + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							__hip_atomic_store(a.host_flag, tile + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
						}
						if ((tid & 63u) == 0) *abort_lds = 1;
						break;
					}
				}
				if (spins) __builtin_amdgcn_s_sleep(1);
			}
		}
		// ---- halo rows of the image, side words for the face pass
#pragma unroll
		for (int k = 0; k < (int)FE; k++)
			if (face_entry((u32)k))
			{
				const u32 hp = (tl >> 5) + 32u * (u32)k, hx = tl & 31u;
				*reinterpret_cast<u32 *>(lds + slab_chunk_off(0u, hx, hp >> 2, NCH) + (hp & 3u) * 4u) = hlo[k];
				*reinterpret_cast<u32 *>(lds + slab_chunk_off(33u, hx, hp >> 2, NCH) + (hp & 3u) * 4u) = hhi[k];
			}
		if (yl == 0 || yl == 31)
		{
			u32 *sd = side + (yl ? 32u : 0u) + x;
			sd[0] = zlo;
			sd[64] = zhi;
		}
		__syncthreads(); // the image holds state t: own rows (end of the previous step) + both halo rows
		if (*abort_lds) return;

		const u32 ntag = tag + 1u, npar = ntag & 1u;
		// ---- the y faces of state t + 1 first (one word per thread), then this thread's rows y-1 / y+1
		if (!last)
#pragma unroll
		for (int k = 0; k < (int)FE; k++)
		if (face_entry((u32)k))
		{
			const u32 fp = (tl >> 5) + 32u * (u32)k, fx = tl & 31u, ch = fp >> 2, wi = (fp & 3u) * 4u;
			const u32 fpm = fp ? fp - 1u : 0u, fpp = fp < (u32)PZ - 1u ? fp + 1u : (u32)PZ - 1u;
			const u32 chm = fpm >> 2, wim = (fpm & 3u) * 4u, chp = fpp >> 2, wip = (fpp & 3u) * 4u;
			const u32 dmask = (int)fp == dead_p ? 0u : 0xFFFFFFFFu;
#pragma unroll
			for (int f = 0; f < 2; f++)
			{
				const u32 row = f ? 32u : 1u;
				const u32 w = *reinterpret_cast<const u32 *>(lds + slab_chunk_off(row, fx, ch, NCH) + wi);
				const u32 ym = *reinterpret_cast<const u32 *>(lds + slab_chunk_off(row - 1u, fx, ch, NCH) + wi);
				const u32 yp = *reinterpret_cast<const u32 *>(lds + slab_chunk_off(row + 1u, fx, ch, NCH) + wi);
				const u32 *sd = side + (f ? 32u : 0u) + fx;
				const u32 below = (fp ? *reinterpret_cast<const u32 *>(lds + slab_chunk_off(row, fx, chm, NCH) + wim) : sd[0]) & dmask;
				const u32 above = fp < (u32)PZ - 1u ? *reinterpret_cast<const u32 *>(lds + slab_chunk_off(row, fx, chp, NCH) + wip) : sd[64];
				// every lane of the wave takes part in the lane exchanges (PZ * 32 is a multiple of 64)
				const u32 o = res_rule<LS, LB>(w, left_of(w), right_of(w), ym, yp, below, above);
				res_store_granule(mailbox(npar, tile, f ? RES_FACE_YHI : RES_FACE_YLO) + tl + (u32)kSlabThreads * (u32)k, ntag, o);
			}
		}
		u32 ym[NCH * 4u], yp[NCH * 4u];
		auto load_chunk = [&](int c) {
			const uint4 m = *reinterpret_cast<const uint4 *>(lds + slab_chunk_off(yl, x, (u32)c, NCH));
			const uint4 q = *reinterpret_cast<const uint4 *>(lds + slab_chunk_off(yl + 2u, x, (u32)c, NCH));
			ym[4 * c] = m.x; ym[4 * c + 1] = m.y; ym[4 * c + 2] = m.z; ym[4 * c + 3] = m.w;
			yp[4 * c] = q.x; yp[4 * c + 1] = q.y; yp[4 * c + 2] = q.z; yp[4 * c + 3] = q.w;
		};
		if (kLate)
		{
			load_chunk(0); // planes 0 .. 3: the low z face, and the pass's first planes
			// the last plane's two words for the high z face (its chunk is read when the pass gets there)
			ym[PZ - 1] = *reinterpret_cast<const u32 *>(lds + slab_chunk_off(yl, x, (u32)(PZ - 1) >> 2, NCH) + ((u32)(PZ - 1) & 3u) * 4u);
			yp[PZ - 1] = *reinterpret_cast<const u32 *>(lds + slab_chunk_off(yl + 2u, x, (u32)(PZ - 1) >> 2, NCH) + ((u32)(PZ - 1) & 3u) * 4u);
		}
		else
		{
#pragma unroll
			for (int c = 0; c < (int)NCH; c++) load_chunk(c);
			__syncthreads(); // every read of the image is done: the new rows may go in at the end of the step
		}

		// ---- one sub-step in place; planes 0 and PZ-1 first: the z faces of state t + 1
		auto below_of = [&](int p, u32 v) { return p == dead_p ? 0u : v; }; // p is a compile-time index after unrolling: one scalar compare + select
		const u32 n0 = res_rule<LS, LB>(s[0], left_of(s[0]), right_of(s[0]), ym[0], yp[0], below_of(0, zlo), s[1]);
		const u32 nl = res_rule<LS, LB>(s[PZ - 1], left_of(s[PZ - 1]), right_of(s[PZ - 1]), ym[PZ - 1], yp[PZ - 1], below_of(PZ - 1, s[PZ - 2]), zhi);
		if (!last)
		{
			res_store_granule(mailbox(npar, tile, RES_FACE_ZLO) + tl, ntag, n0);
			res_store_granule(mailbox(npar, tile, RES_FACE_ZHI) + tl, ntag, nl);
		}
		__builtin_amdgcn_sched_barrier(0);
#if CA3D_SLAB_LOOKAHEAD
		if (kLate && NCH > 1u) load_chunk(1);
#endif
		u32 below = s[0];
#pragma unroll
		for (int p = 1; p < PZ - 1; p++)
		{
			if (kLate && (p & 3) == 0)
			{
				// the rows of these four planes (pinned: hoisted to the head of the pass they would all be live at once again; not asked
				// for a chunk ahead either — eight more registers spill, and three other waves of the SIMD cover the round trip)
				__builtin_amdgcn_sched_barrier(0);
#if CA3D_SLAB_LOOKAHEAD
				if (p / 4 + 1 < (int)NCH) load_chunk(p / 4 + 1);
#else
				load_chunk(p / 4);
#endif
				__builtin_amdgcn_sched_barrier(0);
			}
			u32 w = s[p];
			if (kLate) asm volatile("" : "+v"(w)); // opaque: otherwise the lane exchanges of ALL planes are hoisted in front of the pass and their results spill
			s[p] = res_rule<LS, LB>(w, left_of(w), right_of(w), ym[p], yp[p], below_of(p, below), s[p + 1]);
			if (kLate) asm volatile("" : "+v"(s[p])); // ... and the arithmetic is NOT sunk behind the whole pass's row reads (which would have to stay live for it)
			below = w;
			if (p == kSlabPrefetchPlane && !last)
			{
				// ask for the neighbours' faces of state t + 1 part-way through the pass (see the full-grid form; later in the pass the
				// requests push the allocation over 128 VGPRs)
				const unsigned long long done = (unsigned long long)ntag << 32;
				pre[0] = end_zlo ? done : __hip_atomic_load((const gu64 *)(mailbox(npar, t_zlo, RES_FACE_ZHI) + tl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				pre[1] = end_zhi ? done : __hip_atomic_load((const gu64 *)(mailbox(npar, t_zhi, RES_FACE_ZLO) + tl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
				for (int k = 0; k < (int)FE; k++)
				{
					pre[2 + 2 * k] = face_entry((u32)k) ? __hip_atomic_load((const gu64 *)(mailbox(npar, t_ylo, RES_FACE_YHI) + tl + (u32)kSlabThreads * (u32)k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					pre[3 + 2 * k] = face_entry((u32)k) ? __hip_atomic_load((const gu64 *)(mailbox(npar, t_yhi, RES_FACE_YLO) + tl + (u32)kSlabThreads * (u32)k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
				}
				have_pre = true;
			}
		}
		s[0] = n0;
		s[PZ - 1] = nl;
		if (kLate) __syncthreads(); // every wave has read its rows: the new ones may go in
		to_image();
		if (tid == 0) __hip_atomic_store((gu32 *)a.status + 4u + tile, t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	u32 *dst = a.out + ((size_t)z0 * G + (y0 + yl)) * C + x;
#pragma unroll
	for (int p = 0; p < PZ; p++) dst[(size_t)p * G * C] = s[p];
}

template <int PZ>
struct ResidentSlabLds
{
	static constexpr u32 bytes = 34u * ((PZ + 3) / 4) * 32u * 16u + 2u * 2u * 32u * 4u + 16u;
};

#ifdef CA3D_JIT_SLAB_PZ
extern "C" __global__ __launch_bounds__(1024, 4) void ca3d_jit_resident_slab(ResidentSlabArgs a)
{
	__shared__ __attribute__((aligned(16))) char slab_lds[ResidentSlabLds<CA3D_JIT_SLAB_PZ>::bytes];
	resident_slab_run<CA3D_JIT_LS, CA3D_JIT_LB, CA3D_JIT_SLAB_PZ>(a, slab_lds);
}
#endif
