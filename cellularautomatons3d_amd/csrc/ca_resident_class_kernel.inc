// Resident multi-step kernel for the rules that need the diagonal neighbour classes (Moore main list, live edges / corners
// rule-sets: compute_clustered.wgsl:88-163 with all three counts in play) at 512^3. Same organisation as ca_resident_vn
// (ca_resident_kernel.inc: 256 tiles of 32 rows x 32 planes, one 512-thread workgroup per CU, a thread owns word x of row
// y for the 32 planes of its tile, state in registers for the whole launch, tile faces handed over as tagged granules),
// with what the 26-neighbourhood adds:
//   * per plane the thread forms the partial sums of ca_packed_roll_kernel.inc — A = l + r + c(y-1) + c(y+1),
//     B = l(y-1) + r(y-1) + l(y+1) + r(y+1) (x shifts by DPP inside the 16-lane row, y rows from the LDS image) — and
//     sweeps its planes with a three-plane window of them;
//   * the sums of the planes just outside the tile need THEIR y neighbours too, so the LDS image carries the halo planes
//     (34 planes x 34 rows x 16 words) and a tile also reads the four rows at its y/z corners from the DIAGONAL tiles — they
//     are entries of those tiles' y faces, nothing extra is published; a tile waits for all eight neighbours;
//   * the rule is the synthesised function of ca_jit_rule.inc (rule_synth.cpp) or the truth tables.
// Run-time compiled only (ca_jit.cpp). Needs ca_bitslice.inc, ca_packed_roll_kernel.inc, ca_resident_kernel.inc.

#ifndef CA3D_RC_PIN_SWEEP
#define CA3D_RC_PIN_SWEEP 1 // 0: the sweep's arithmetic is free to sink behind the request for the next faces
#endif
#ifndef CA3D_RC_PREFETCH_K
#define CA3D_RC_PREFETCH_K 9 // 512^3: sweep iteration at which the next faces are asked for (see there; 3 - 10 measure 9.4 - 9.7 us per step for the clustered rule-set, from 11 on the allocation spills: 10.3 us and up)
#endif
// Geometry of a tile, by grid: CW words per row, PZ planes per tile (32 rows always): 16 / 32 at 512^3 (256 tiles, 512 threads),
// 8 / 8 at 256^3 (256 tiles of 8 words x 32 rows x 8 planes, 256 threads — the tiling of ca_resident_vn256). The LDS image holds
// planes -1 .. PZ as slots 0 .. PZ + 1, four slots per 16-byte chunk.
template <int CW, int PZ>
struct RcGeom
{
	static constexpr u32 C = (u32)CW, G = 32u * C, RY = 32u, NT = C * RY;
	static constexpr u32 TPAY = G / RY, TPAZ = G / (u32)PZ;
	static constexpr u32 slots = (u32)PZ + 2u, chunks = (slots + 3u) / 4u;
	static constexpr u32 image_bytes = 34u * chunks * C * 16u;   // 34 rows x chunks x C words x 16 B (512^3: 76.5 KiB)
	static constexpr u32 lds_bytes = 2u * image_bytes + 16u;     // two images + the abort word
	static constexpr u32 YF = C * (u32)PZ;                       // words of a y face
	static constexpr u32 FW = NT > YF ? NT : YF;                 // mailbox words per face (as ca_resident_vn: resident_mail_bytes)
	static __device__ __forceinline__ u32 off(u32 row, u32 x, u32 slot) { return ((row * chunks + (slot >> 2)) * C + x) * 16u + (slot & 3u) * 4u; }
	static __device__ __forceinline__ u32 chunk(u32 row, u32 x, u32 ch) { return ((row * chunks + ch) * C + x) * 16u; }
};

// partial sums of one plane for one word: c = own row, ym / yp = rows y-1 / y+1 (x neighbours come from the lanes)
template <int CW>
__device__ __forceinline__ void rc_plane_sums(u32 c, u32 ym, u32 yp, u32 xmask, bool xlast, RollSumsT<1> &s)
{
	const u32 vs = ym ^ yp, vk = ym & yp; // the two rows as a 2-bit column sum
	u32 t;
	fa(res_left_w<CW>(c, xmask), res_right_w<CW>(c, xlast), vs, s.a[0][0], t);
	ha(t, vk, s.a[0][1], s.a[0][2]);
	ha(res_left_w<CW>(vs, xmask), res_right_w<CW>(vs, xlast), s.b[0][0], t);
	fa(res_left_w<CW>(vk, xmask), res_right_w<CW>(vk, xlast), t, s.b[0][1], s.b[0][2]);
	s.c[0] = c;
}

template <int MAIN, bool E, bool C_>
__device__ __forceinline__ u32 rc_output(const RollSumsT<1> &dn, const RollSumsT<1> &ct, const RollSumsT<1> &up)
{
	u32 res[1];
	roll_output<MAIN, E, C_, 1>(dn, ct, up, res);
	return res[0];
}

// ZS = z groups of a tile: the threads of group zg own planes zg * PZ / ZS .. of their column (512^3: 1 — the registers of a
// second group do not exist; 256^3: 2 — 512 threads, two waves per SIMD instead of one, which is what a step made of dependent
// instructions wants). Whatever a thread needs from outside its planes it reads from the LDS image, which holds every plane of
// the tile and, after phase B, the halo: for ZS > 1 that includes its own row's planes just below and above its range.
template <int MAIN, bool E, bool C_, int CW, int PZ, int ZS>
__device__ __forceinline__ void resident_class_run(const ResidentArgs &a, char *lds)
{
	typedef RcGeom<CW, PZ> Gm;
	constexpr u32 C = Gm::C, G = Gm::G, RY = Gm::RY, NT1 = Gm::NT, NT = NT1 * (u32)ZS, TPAY = Gm::TPAY, TPAZ = Gm::TPAZ, YF = Gm::YF, FW = Gm::FW;
	constexpr u32 kImage = Gm::image_bytes;
	constexpr int PZT = PZ / ZS;                                   // planes of a thread
	constexpr int kChunksT = ZS == 1 ? (int)Gm::chunks : (PZT + 2 + 3) / 4; // 16-byte chunks that cover its PZT + 2 slots
	constexpr int kPrefetchK = PZ >= 32 ? CA3D_RC_PREFETCH_K : 2;
	constexpr bool kSplitFaces = 2u * YF <= NT;                    // enough threads to give each y-face word its own
	constexpr bool kChunkReads = ZS == 1 || PZT % 4 == 0;         // a z group's slots start on a chunk boundary (else: word by word)
	static_assert(PZ % ZS == 0 && PZT >= 2 && (ZS > 1 || (PZT % 2 == 0 && PZT >= 4)), "one group: the sweep runs from both ends and meets between two planes");
	static_assert(NT1 % 64u == 0, "a wave belongs to one z group");
	const u32 tile = blockIdx.x;
	if (res_must_skip(a, tile)) return;
	const u32 ty = tile % TPAY, tz = tile / TPAY;
	const u32 tid = threadIdx.x, tid1 = ZS == 1 ? tid : tid % NT1, zg = ZS == 1 ? 0u : tid / NT1, x = tid1 % C, yl = tid1 / C;
	const u32 y0 = ty * RY, z0 = tz * (u32)PZ, zb = zg * (u32)PZT;
	const bool zfirst = zg == 0, zlast = zg == (u32)ZS - 1u;
	// static issue priority for the older wave of every SIMD, as in the von Neumann row-pair form (ca_resident_kernel.inc): 512^3
	// 9.46 -> 9.26 us per step; the 256^3 form (two z groups) measured SLOWER with it (2.25 -> 2.33) and runs without
	if (ZS == 1 && tid < NT / 2u) __builtin_amdgcn_s_setprio(1);
	u32 xmask = x == 0u ? 0u : 0xFFFFFFFFu; // rows of 8 words: x-1 is dead at x == 0 (two grid rows share a DPP row)
	asm volatile("" : "+v"(xmask));
	const bool xlast = x == C - 1u;
	u32 *abort_lds = reinterpret_cast<u32 *>(lds + 2u * kImage);

	// the eight neighbour tiles; a coordinate of -1 is dead (its data reads as zero, its tile is still waited for: the
	// mailbox argument of ca_resident_kernel.inc), a coordinate of G wraps to tile 0 of that axis
	const bool dead_y = ty == 0, dead_z = tz == 0;
	const u32 tym = ty == 0 ? TPAY - 1u : ty - 1u, typ = ty + 1u == TPAY ? 0u : ty + 1u;
	const u32 tzm = tz == 0 ? TPAZ - 1u : tz - 1u, tzp = tz + 1u == TPAZ ? 0u : tz + 1u;
	auto mailbox = [&](u32 parity, u32 t, u32 face) { return a.mail + (((size_t)parity * (TPAY * TPAZ) + t) * 4u + face) * FW; };
	// y faces hold YF words: the first YF threads fetch word `tid` of both (whole waves: YF is a multiple of 64)
	const bool yface_thread = NT <= YF || tid < YF;
	// corner k of the first 4 C threads: (row -1 | 32) x (plane -1 | PZ), C words each = entries of the diagonal tile's y face
	const u32 ck = (tid / C) & 3u, cyhi = ck & 1u, czhi = ck >> 1;
	const u32 ct_tile = (cyhi ? typ : tym) + (czhi ? tzp : tzm) * TPAY;
	const u32 ct_face = cyhi ? RES_FACE_YLO : RES_FACE_YHI;             // the row of that tile that touches mine
	const u32 ct_entry = (czhi ? 0u : (u32)PZ - 1u) * C + x;             // its plane that touches mine
	const bool corner_thread = tid < 4u * C;
	const bool corner_dead = (!cyhi && dead_y) || (!czhi && dead_z);     // "zero wins"

	u32 s[PZT];
	{
		const u32 *src = a.in + ((size_t)(z0 + zb) * G + (y0 + yl)) * C + x;
#pragma unroll
		for (int p = 0; p < PZT; p++) s[p] = src[(size_t)p * G * C];
	}
	if (tid == 0) *abort_lds = 0;

	auto to_image = [&](u32 img) {
		char *base = lds + img * kImage;
		if (ZS == 1)
		{
			// slots 1 .. PZ of my row as whole chunks: chunk k holds planes 4k-1 .. 4k+2, so the first and the last chunk also
			// cover the halo slots 0 and PZ + 1 (and padding slots) — those are written again, with the neighbours' words, in
			// phase B of the step that reads this image
#pragma unroll
			for (int k = 0; k < (int)Gm::chunks; k++)
			{
				const int p0 = 4 * k - 1;
				uint4 v;
				v.x = (p0 >= 0 && p0 < PZT) ? s[(p0 >= 0 && p0 < PZT) ? p0 : 0] : 0u;
				v.y = (p0 + 1 < PZT) ? s[(p0 + 1 < PZT) ? p0 + 1 : 0] : 0u;
				v.z = (p0 + 2 < PZT) ? s[(p0 + 2 < PZT) ? p0 + 2 : 0] : 0u;
				v.w = (p0 + 3 < PZT) ? s[(p0 + 3 < PZT) ? p0 + 3 : 0] : 0u;
				*reinterpret_cast<uint4 *>(base + Gm::chunk(yl + 1u, x, (u32)k)) = v;
			}
		}
		else
		{
			// a chunk is shared with the group below / above: word by word
#pragma unroll
			for (int p = 0; p < PZT; p++) *reinterpret_cast<u32 *>(base + Gm::off(yl + 1u, x, zb + (u32)p + 1u)) = s[p];
		}
	};
	to_image(0);
	{
		const u32 tag0 = a.epoch0 + 1u, par0 = tag0 & 1u;
		if (zfirst) res_store_granule(mailbox(par0, tile, RES_FACE_ZLO) + tid1, tag0, s[0]);
		if (zlast) res_store_granule(mailbox(par0, tile, RES_FACE_ZHI) + tid1, tag0, s[PZT - 1]);
		if (yl == 0)
		{
#pragma unroll
			for (int p = 0; p < PZT; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YLO) + (zb + (u32)p) * C + x, tag0, s[p]);
		}
		if (yl == RY - 1)
		{
#pragma unroll
			for (int p = 0; p < PZT; p++) res_store_granule(mailbox(par0, tile, RES_FACE_YHI) + (zb + (u32)p) * C + x, tag0, s[p]);
		}
	}

	unsigned long long pre[5] = {0, 0, 0, 0, 0};
	bool have_pre = false;
#ifdef CA3D_RES_STAMPS
	// diagnostic build (tools/run_class_probe.py): cycles per phase, averaged over the steps, for every wave of tile 37
	unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = 0;
#define RC_STAMP(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); st_acc[i] += now_ - st_prev; st_prev = now_; } while (0)
#else
#define RC_STAMP(i) do { } while (0)
#endif
	for (u32 t = 0; t < a.steps; t++)
	{
		const u32 tag = a.epoch0 + t + 1u, par = tag & 1u, img = t & 1u;
		const bool last = t + 1u == a.steps;
#ifdef CA3D_RES_STAMPS
		st_prev = __builtin_amdgcn_s_memtime();
		__builtin_amdgcn_s_waitcnt(0xC07F);
#endif
		// ---- A. faces of state t from the four face neighbours (as ca_resident_vn; the z faces by the groups that touch them)
		// and, for 4 C threads, a corner row
		const gu64 *g_zlo = (const gu64 *)(mailbox(par, ty + tzm * TPAY, RES_FACE_ZHI) + tid1);
		const gu64 *g_zhi = (const gu64 *)(mailbox(par, ty + tzp * TPAY, RES_FACE_ZLO) + tid1);
		const gu64 *g_ylo = (const gu64 *)(mailbox(par, tym + tz * TPAY, RES_FACE_YHI) + tid);
		const gu64 *g_yhi = (const gu64 *)(mailbox(par, typ + tz * TPAY, RES_FACE_YLO) + tid);
		const gu64 *g_cor = (const gu64 *)(mailbox(par, ct_tile, ct_face) + ct_entry);
		u32 zlo = 0, zhi = 0, hlo = 0, hhi = 0, cor = 0;
		{
			const unsigned long long done = (unsigned long long)tag << 32;
			unsigned long long q0 = pre[0], q1 = pre[1], q2 = pre[2], q3 = pre[3], q4 = pre[4];
			unsigned long long t_start = 0;
			for (u32 spins = 0;; spins++)
			{
				if (spins || !have_pre)
				{
					q0 = zfirst ? __hip_atomic_load(g_zlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					q1 = zlast ? __hip_atomic_load(g_zhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					q2 = yface_thread ? __hip_atomic_load(g_ylo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					q3 = yface_thread ? __hip_atomic_load(g_yhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
					q4 = corner_thread ? __hip_atomic_load(g_cor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
				}
				zlo = dead_z ? 0u : (u32)q0; zhi = (u32)q1; hlo = dead_y ? 0u : (u32)q2; hhi = (u32)q3; cor = corner_dead ? 0u : (u32)q4;
				const bool ok = (u32)(q0 >> 32) == tag && (u32)(q1 >> 32) == tag && (u32)(q2 >> 32) == tag && (u32)(q3 >> 32) == tag && (u32)(q4 >> 32) == tag;
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
						if (expired && !other && (tid & 63u) == 0) res_report_timeout(a, tile);
						if ((tid & 63u) == 0) *abort_lds = 1;
						break;
					}
				}
				if (spins) __builtin_amdgcn_s_sleep(1);
			}
		}
		RC_STAMP(0);
		// ---- B. the halo of the image: rows -1 / 32 (planes 0 .. PZ-1), planes -1 / PZ (my row), the four corner rows
		{
			char *base = lds + img * kImage;
			if (yface_thread)
			{
				const u32 hp = tid / C, hx = tid % C;
				*reinterpret_cast<u32 *>(base + Gm::off(0u, hx, hp + 1u)) = hlo;
				*reinterpret_cast<u32 *>(base + Gm::off(33u, hx, hp + 1u)) = hhi;
			}
			if (zfirst) *reinterpret_cast<u32 *>(base + Gm::off(yl + 1u, x, 0u)) = zlo;
			if (zlast) *reinterpret_cast<u32 *>(base + Gm::off(yl + 1u, x, (u32)PZ + 1u)) = zhi;
			if (corner_thread) *reinterpret_cast<u32 *>(base + Gm::off(cyhi ? 33u : 0u, x, czhi ? (u32)PZ + 1u : 0u)) = cor;
		}
		__syncthreads();
		if (*abort_lds) return;
		RC_STAMP(1);

		const char *im = lds + img * kImage;
		const u32 ntag = tag + 1u, npar = ntag & 1u;
		// ---- C. the y faces of state t + 1 first: rows 0 and 31 of every plane. With threads to spare each face word has its
		// own (word w of face f = thread f * YF + w), otherwise a thread forms word `tid` of both faces.
		if (!last && (kSplitFaces ? tid < 2u * YF : yface_thread))
		{
			const u32 fw = kSplitFaces ? tid % YF : tid, fp = fw / C, fx = fw % C;
#pragma unroll
			for (int ff = 0; ff < (kSplitFaces ? 1 : 2); ff++)
			{
				const u32 f = kSplitFaces ? tid / YF : (u32)ff;
				const u32 row = f ? 32u : 1u; // image row of tile row 0 / 31
				RollSumsT<1> w3[3];
#pragma unroll
				for (int d = 0; d < 3; d++) // planes fp - 1, fp, fp + 1 = slots fp, fp + 1, fp + 2
				{
					const u32 slot = fp + (u32)d;
					const u32 c = *reinterpret_cast<const u32 *>(im + Gm::off(row, fx, slot));
					const u32 ym = *reinterpret_cast<const u32 *>(im + Gm::off(row - 1u, fx, slot));
					const u32 yp = *reinterpret_cast<const u32 *>(im + Gm::off(row + 1u, fx, slot));
					rc_plane_sums<CW>(c, ym, yp, xmask, xlast, w3[d]);
				}
				const u32 o = rc_output<MAIN, E, C_>(w3[0], w3[1], w3[2]);
				res_store_granule(mailbox(npar, tile, f ? RES_FACE_YHI : RES_FACE_YLO) + fw, ntag, o);
			}
		}

		RC_STAMP(2);
		// ---- rows y-1 and y+1 of my PZT + 2 slots (zb .. zb + PZT + 1; the last chunk's upper part is padding / not mine)
		u32 ym[4 * kChunksT], yp[4 * kChunksT];
		if (kChunkReads)
		{
#pragma unroll
			for (int c = 0; c < kChunksT; c++)
			{
				const uint4 m = *reinterpret_cast<const uint4 *>(im + Gm::chunk(yl, x, zb / 4u + (u32)c));
				const uint4 q = *reinterpret_cast<const uint4 *>(im + Gm::chunk(yl + 2u, x, zb / 4u + (u32)c));
				ym[4 * c] = m.x; ym[4 * c + 1] = m.y; ym[4 * c + 2] = m.z; ym[4 * c + 3] = m.w;
				yp[4 * c] = q.x; yp[4 * c + 1] = q.y; yp[4 * c + 2] = q.z; yp[4 * c + 3] = q.w;
			}
		}
		else
		{
#pragma unroll
			for (int sl = 0; sl < PZT + 2; sl++)
			{
				ym[sl] = *reinterpret_cast<const u32 *>(im + Gm::off(yl, x, zb + (u32)sl));
				yp[sl] = *reinterpret_cast<const u32 *>(im + Gm::off(yl + 2u, x, zb + (u32)sl));
			}
		}
		// my own row just below and above my planes: the neighbour tiles' faces (ZS == 1: still in registers) or the other group's planes
		const u32 clo = ZS == 1 ? zlo : *reinterpret_cast<const u32 *>(im + Gm::off(yl + 1u, x, zb));
		const u32 chi = ZS == 1 ? zhi : *reinterpret_cast<const u32 *>(im + Gm::off(yl + 1u, x, zb + (u32)PZT + 1u));

		RC_STAMP(3);
		// ---- D. the sweep over my slots with a three-slot window of plane sums
		auto ask_ahead = [&]() {
			// The neighbours published their faces of state t + 1 when I did: half way through the sweep they are visible —
			// asked for right after publishing, the loads come back with the old tags (ca_resident_kernel.inc). Not later
			// than this: the requests bound the compiler's scheduling region, and placed near the end of the sweep the
			// allocation spills.
			const unsigned long long done = (unsigned long long)ntag << 32;
			pre[0] = zfirst ? __hip_atomic_load((const gu64 *)(mailbox(npar, ty + tzm * TPAY, RES_FACE_ZHI) + tid1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
			pre[1] = zlast ? __hip_atomic_load((const gu64 *)(mailbox(npar, ty + tzp * TPAY, RES_FACE_ZLO) + tid1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
			pre[2] = yface_thread ? __hip_atomic_load((const gu64 *)(mailbox(npar, tym + tz * TPAY, RES_FACE_YHI) + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
			pre[3] = yface_thread ? __hip_atomic_load((const gu64 *)(mailbox(npar, typ + tz * TPAY, RES_FACE_YLO) + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
			pre[4] = corner_thread ? __hip_atomic_load((const gu64 *)(mailbox(npar, ct_tile, ct_face) + ct_entry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : done;
			have_pre = true;
		};
		if (ZS == 1)
		{
			// One group: from BOTH ends inwards. Slots 0, 1, 2 give plane 0 and slots PZ+1, PZ, PZ-1 give plane PZ-1 — the two z
			// faces of state t + 1 — within the first three iterations, and no plane's sums are formed twice (a one-ended sweep
			// has to compute the far face ahead of time). The lower window climbs (slot i yields plane i - 2), the upper one
			// descends (slot j yields plane j), they meet between planes PZ/2 - 1 and PZ/2, which take slots from both windows. A
			// raw word is last read when the slot above it (lower) / below it (upper) is formed: registers are updated in place.
			RollSumsT<1> lo[3], hi[3];
#pragma unroll
			for (int k = 0; k <= PZT / 2; k++)
			{
				const int i = k, j = PZT + 1 - k;
				rc_plane_sums<CW>(i == 0 ? clo : s[i > 0 ? i - 1 : 0], ym[i], yp[i], xmask, xlast, lo[i % 3]);
				if (i >= 2) s[i - 2] = rc_output<MAIN, E, C_>(lo[(i - 2) % 3], lo[(i - 1) % 3], lo[i % 3]);
				rc_plane_sums<CW>(j == PZT + 1 ? chi : s[j < PZT + 1 ? j - 1 : 0], ym[j], yp[j], xmask, xlast, hi[j % 3]);
				if (j <= PZT - 1) s[j] = rc_output<MAIN, E, C_>(hi[j % 3], hi[(j + 1) % 3], hi[(j + 2) % 3]);
				if (k == 2 && !last)
				{
					if (zfirst) res_store_granule(mailbox(npar, tile, RES_FACE_ZLO) + tid1, ntag, s[0]);
					if (zlast) res_store_granule(mailbox(npar, tile, RES_FACE_ZHI) + tid1, ntag, s[PZT - 1]);
				}
				if (k == (kPrefetchK > 2 ? kPrefetchK : 2) && !last)
				{
					// the planes formed so far stay in front of the request: nothing but the image write reads them, and the compiler
					// sank their arithmetic behind this branch — the request then left right after the z faces (the order up to round 5)
					if (CA3D_RC_PIN_SWEEP)
					{
#pragma unroll
						for (int q = 0; q <= i - 2; q++) asm volatile("" : "+v"(s[q]));
#pragma unroll
						for (int q = j < PZT ? j : PZT; q <= PZT - 1; q++) asm volatile("" : "+v"(s[q]));
					}
					ask_ahead();
				}
			}
			{
				// the two planes in the middle: slots from both windows (plane p needs slots p, p + 1, p + 2)
				constexpr int m = PZT / 2 - 1;
				const u32 om = rc_output<MAIN, E, C_>(lo[m % 3], lo[(m + 1) % 3], hi[(m + 2) % 3]);
				const u32 om1 = rc_output<MAIN, E, C_>(lo[(m + 1) % 3], hi[(m + 2) % 3], hi[(m + 3) % 3]);
				s[m] = om;
				s[m + 1] = om1;
			}

		}
		else if (zlast)
		{
			// With several groups a group has ONE outer face, and what the neighbour tile waits for is that plane: the last group
			// sweeps downwards from it (slot n' = PZT + 1 - n yields plane n', from slots n', n' + 1, n' + 2), every other group
			// upwards. The face plane is the first output, after three slots.
			RollSumsT<1> w[3];
#pragma unroll
			for (int n = 0; n <= PZT + 1; n++)
			{
				const int sl = PZT + 1 - n;
				rc_plane_sums<CW>(sl == PZT + 1 ? chi : sl == 0 ? clo : s[sl > 0 && sl <= PZT ? sl - 1 : 0], ym[sl], yp[sl], xmask, xlast, w[n % 3]);
				if (n >= 2) s[sl] = rc_output<MAIN, E, C_>(w[n % 3], w[(n + 2) % 3], w[(n + 1) % 3]);
				if (n == 2 && !last) res_store_granule(mailbox(npar, tile, RES_FACE_ZHI) + tid1, ntag, s[PZT - 1]);
				if (n == 3 && !last) ask_ahead();
			}
		}
		else
		{
			RollSumsT<1> w[3];
#pragma unroll
			for (int n = 0; n <= PZT + 1; n++)
			{
				rc_plane_sums<CW>(n == 0 ? clo : n == PZT + 1 ? chi : s[n > 0 && n <= PZT ? n - 1 : 0], ym[n], yp[n], xmask, xlast, w[n % 3]);
				if (n >= 2) s[n - 2] = rc_output<MAIN, E, C_>(w[(n + 1) % 3], w[(n + 2) % 3], w[n % 3]);
				if (n == 2 && !last && zfirst) res_store_granule(mailbox(npar, tile, RES_FACE_ZLO) + tid1, ntag, s[0]);
				if (n == 3 && !last) ask_ahead();
			}
		}
		RC_STAMP(4);
		to_image(img ^ 1u);
		RC_STAMP(5);
		if (tid == 0) __hip_atomic_store((gu32 *)a.status + 4u + tile, t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (t + 2u == a.steps)
		{
			u32 *dst = a.out_prev + ((size_t)(z0 + zb) * G + (y0 + yl)) * C + x;
			asm volatile("" : "+v"(dst)); // opaque: otherwise the store addresses are hoisted out of the step loop and live (spilled) through it
#pragma unroll
			for (int p = 0; p < PZT; p++) dst[(size_t)p * G * C] = s[p];
		}
	}
#ifdef CA3D_RES_STAMPS
	if (tile == 37u && (tid & 63u) == 0)
		for (int i = 0; i < 6; i++) a.status[600 + (tid >> 6) * 8 + i] = (u32)(st_acc[i] / a.steps);
#endif
	u32 *dst = a.out_last + ((size_t)(z0 + zb) * G + (y0 + yl)) * C + x;
#pragma unroll
	for (int p = 0; p < PZT; p++) dst[(size_t)p * G * C] = s[p];
}

#ifdef CA3D_JIT
extern "C" __global__ __launch_bounds__(512, 2) void ca3d_jit_resident_class(ResidentArgs a)
{
	__shared__ __attribute__((aligned(16))) char rc_lds[RcGeom<16, 32>::lds_bytes];
	resident_class_run<CA3D_JIT_MAIN, CA3D_JIT_E, CA3D_JIT_C, 16, 32, 1>(a, rc_lds);
}
// 256^3: 8 words x 32 rows x 8 planes per tile; two z groups (512 threads: shipped) / four / one (CA3D_RC256_ZS, for comparison)
extern "C" __global__ __launch_bounds__(512, 1) void ca3d_jit_resident_class256(ResidentArgs a)
{
	__shared__ __attribute__((aligned(16))) char rc_lds[RcGeom<8, 8>::lds_bytes];
	resident_class_run<CA3D_JIT_MAIN, CA3D_JIT_E, CA3D_JIT_C, 8, 8, 2>(a, rc_lds);
}
extern "C" __global__ __launch_bounds__(1024, 1) void ca3d_jit_resident_class256_z4(ResidentArgs a)
{
	__shared__ __attribute__((aligned(16))) char rc_lds[RcGeom<8, 8>::lds_bytes];
	resident_class_run<CA3D_JIT_MAIN, CA3D_JIT_E, CA3D_JIT_C, 8, 8, 4>(a, rc_lds);
}
extern "C" __global__ __launch_bounds__(256, 1) void ca3d_jit_resident_class256_z1(ResidentArgs a)
{
	__shared__ __attribute__((aligned(16))) char rc_lds[RcGeom<8, 8>::lds_bytes];
	resident_class_run<CA3D_JIT_MAIN, CA3D_JIT_E, CA3D_JIT_C, 8, 8, 1>(a, rc_lds);
}
#endif
