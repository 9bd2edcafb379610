// The pass over the 48 orientations of a universe that lies in LDS as the turn image (ca_turn_image.inc): for every o the thread
// assembles ITS four rows of T_o — the state turned by o, the turned box's minimum at the origin —, the wave's share of T_o's ca3d_summary
// digest goes to dig[o][wave], and bit o of `differs` says that one of the wave's rows of T_o is not its row of T_0 (DESIGN.md 12.10).
//
// A FRAGMENT, not a header and not a function: no include guard, and it is included only inside the function whose text it is, at the
// place where the text stood — ca_ensemble_canon64 (ca_canon.hip) and, inside the loop over the phases, canon_period_run
// (ca_canon_period.hip). As a __forceinline__ function the same text changed both kernels' register allocation and instruction counts;
// as text it leaves their listings as they were measured (DESIGN.md 12.10, 12.15).
//
// The contract with the place of inclusion:
//  - it reads   img (the image, complete behind a barrier and not written while the pass runs), dig, mn[3] and mx[3] (the box of the
//               state, workgroup-uniform; all zero for an empty universe), row, wave (wave-uniform);
//  - it declares and leaves   T0[kPT][2] (the thread's rows of T_0), t0_any, differs (both wave-uniform);
//  - it holds NO barrier, and every loop bound is a constant, or uniform over the workgroup or the wave;
//  - it needs ca_turn_image.inc, ca_digest.h and kOrientations of the including file.
//
// THE MAP AND THE ROW ASSEMBLY are compose's (ca_compose.hip's header; DESIGN.md 12.9) with at = 0, so that the intervals are
// [0, e'[i] - 1] and nothing is clipped. Compose clips by `at` (lo and hi on every axis): that is another text, and it stays there.
	u32 T0[kPT][2]; // the thread's rows of T_0, from o = 0
#pragma unroll
	for (u32 p = 0; p < kPT; p++) T0[p][0] = T0[p][1] = 0u;
	bool t0_any = false; // wave-uniform: the wave holds a cell of T_0
	u64 differs = 0;     // wave-uniform

	// WHICH ROWS OF T_o A THREAD ASSEMBLES is free, since they come out of the image: not planes 4 w .. 4 w + 3, load_universe's, but
	// planes w, w + 16, w + 32, w + 48. An ash object, two or three planes thick, then lies in two or three waves on different SIMDs
	// with ONE plane each, where the other layout would give all of it to wave 0: the launch is bound by that one wave's digest_mix.
	// A wave whose planes lie above the LARGEST extent of the box lies above every turned box: all its rows of every T_o are zero. It
	// writes its 48 zeros at once and leaves the loop to the others (wave-uniform, and no barrier inside either branch).
	const int reach = max(mx[0] - mn[0], max(mx[1] - mn[1], mx[2] - mn[2]));
	if ((int)wave > reach)
	{
		if (row < kOrientations) dig[row * kWaves + wave] = 0ull;
	}
	else
	{
#pragma nounroll
	for (u32 o = 0; o < kOrientations; o++) // compile-time bounds, the same for every thread; no barrier inside
	{
		// ---- the map, workgroup-uniform: compose's with at = 0
		const u32 m = o % 6u, f = o / 6u;
		const u32 pj[3] = {(kPerm0 >> 2u * m) & 3u, (kPerm1 >> 2u * m) & 3u, (kPerm2 >> 2u * m) & 3u};
		int s[3], k[3], hi[3];
#pragma unroll
		for (int d = 0; d < 3; d++)
		{
			const int lo_c = pick(pj[d], mn[0], mn[1], mn[2]), ext = pick(pj[d], mx[0], mx[1], mx[2]) - lo_c + 1;
			const bool flip = (f >> d) & 1u;
			s[d] = flip ? -1 : 1;
			k[d] = lo_c + (flip ? ext - 1 : 0);
			hi[d] = ext - 1; // the turned box is [0, hi] on every axis: inside the cube
		}
		u64 sum = 0;
		bool row_differs;
		if ((int)wave > hi[2]) // wave-uniform: the wave's planes lie above the turned box, its rows of T_o are zero
			row_differs = t0_any;
		else
		{
			u32 ch = 0;
			// this thread's row y, clamped into the turned box: the address stays inside the image, the result is dropped below
			const int y = (int)row, yc = min(y, hi[1]);
			const int cy_from = s[1] * yc + k[1]; // the universe's coordinate on axis pj[1]
#pragma unroll
			for (u32 p = 0; p < kPT; p++)
			{
				const int z = (int)(p * kWaves + wave);
				if (z > hi[2]) // wave-uniform: this plane lies above the turned box, its row of T_o is zero (and so is T_0's at o = 0)
				{
					ch |= T0[p][0] | T0[p][1];
					continue;
				}
				const int cz_from = s[2] * z + k[2]; // the universe's coordinate on axis pj[2]
				const bool inside = y == yc;
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
					// the universe's x comes from y or z: one bit of one word plane; its other coordinate, and pj[0]'s, which x walks
					const int cx = pj[1] == 0u ? cy_from : cz_from;
					const int other = pj[1] == 0u ? cz_from * (pj[2] == 1u ? 1 : (int)kImgPlane) : cy_from * (pj[1] == 1u ? 1 : (int)kImgPlane);
					const int step = pj[0] == 1u ? 1 : (int)kImgPlane;
					const u32 bit = (u32)cx & 31u;
					const int w0 = (cx >> 5) * (int)kImgHalf + other + k[0] * step, dw = s[0] * step;
					u32 r0 = 0, r1 = 0;
#pragma unroll 8
					for (int x = 0; x <= min(hi[0], 31); x++) r0 |= ((img[w0 + x * dw] >> bit) & 1u) << x;
#pragma unroll 8
					for (int x = 32; x <= hi[0]; x++) r1 |= ((img[w0 + x * dw] >> bit) & 1u) << (x - 32);
					r64 = (u64)r1 << 32 | r0;
				}
				if (!inside) r64 = 0;
				const u32 w0r = (u32)r64, w1r = (u32)(r64 >> 32);
				const u64 index = (u64)(((u32)z * 64u + row) * 2u); // the word's index in the packed state
				if (w0r) sum += digest_mix(index, w0r);
				if (w1r) sum += digest_mix(index + 1u, w1r);
				if (o == 0u) { T0[p][0] = w0r; T0[p][1] = w1r; }
				ch |= (w0r ^ T0[p][0]) | (w1r ^ T0[p][1]);
			}
			if (o == 0u) t0_any = __ballot((T0[0][0] | T0[0][1] | T0[1][0] | T0[1][1] | T0[2][0] | T0[2][1] | T0[3][0] | T0[3][1]) != 0u) != 0ull;
			row_differs = __ballot(ch != 0u) != 0ull;
			// the wave's sum, in lane 0: rows above the turned box hold zero, so the butterfly's steps across more than hi[1] lanes would
			// add nothing there (a wave-uniform bound: an ash object takes two or three of the six steps)
#pragma unroll
			for (int off = 32; off > 0; off >>= 1)
				if (off <= hi[1]) sum += __shfl_xor(sum, off);
		}
		if (row == 0u) dig[o * kWaves + wave] = sum;
		if (row_differs) differs |= 1ull << o;
	}
	}
