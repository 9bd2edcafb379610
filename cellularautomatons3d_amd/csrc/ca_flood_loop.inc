// The flood loop on the ensemble's register layout: F <- R & dilate(F) until an iteration changes nothing anywhere (ca_flood.inc's head
// and the comment at flood there; DESIGN.md 12.7, 12.13).
//
// A FRAGMENT, not a header and not a function: no include guard, and it is included only inside the function whose text it is — as the
// whole body of flood<Torus> (ca_flood.inc), and in ca_ensemble_census64 (ca_census.hip) inside a block that sets
// constexpr bool Torus = false. Called as flood(...), the same text changed the census kernel's register allocation, and the census
// measured slower; as text it leaves the listing as it was measured (DESIGN.md 12.7, 12.15).
//
// The contract with the place of inclusion:
//  - it reads   R[kPT][2] (the cells the object may take; F is a part of R), xch (kXchWords) and flg (kFlgWords) in LDS, row, wave
//               (wave-uniform), Torus (a constant expression: false closes all six faces, true joins every face to the opposite one);
//  - it updates   F[kPT][2], the object being filled;
//  - it holds ONE barrier an iteration, reached by all 1024 threads: the place of inclusion is reached by all of them, under no
//    condition that differs within the workgroup. The loop's exit is read from LDS behind that barrier: every thread leaves, or none;
//  - xch and flg are dead behind it (the comment at flood).
	u32 changed = 1u; // wave-uniform
	for (u32 it = 0;; it++)
	{
		const u32 buf = it & 1u;
		u32 Y[kPT][2]; // x and y of the dilation
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				const u32 w = F[p][h], other = F[p][h ^ 1u];
				const u32 l = from_left(w, Torus || h ? other : 0u);  // cell x - 1: word 0's comes from nowhere, word 1's from word 0
				const u32 r = from_right(Torus || !h ? other : 0u, w); // cell x + 1: word 0's from word 1, word 1's from nowhere (closed: no wrap)
				const u32 x = w | l | r;
				// row y - 1 (zero into row 0), row y + 1 (zero into row 63: wave_shl, not the step's wave_rol); the torus rotates
				Y[p][h] = x | dpp_mov<Torus ? kDppWaveRor1 : kDppWaveShr1>(x) | dpp_mov<Torus ? kDppWaveRol1 : kDppWaveShl1>(x);
			}
		xch[slot(buf, wave, 0u, 0u, row)] = Y[0][0];
		xch[slot(buf, wave, 0u, 1u, row)] = Y[0][1];
		xch[slot(buf, wave, 1u, 0u, row)] = Y[kPT - 1][0];
		xch[slot(buf, wave, 1u, 1u, row)] = Y[kPT - 1][1];
		if (row == 0u) flg[buf * kWaves + wave] = changed;
		// (a wave writes this parity's buffer again two iterations on, behind the next iteration's barrier, which no wave passes
		// before it has read this one's)
		__syncthreads();
		const uint4 *f4 = reinterpret_cast<const uint4 *>(flg + buf * kWaves);
		uint4 m = f4[0];
#pragma unroll
		for (u32 i = 1; i < kWaves / 4u; i++) { const uint4 v = f4[i]; m.x |= v.x; m.y |= v.y; m.z |= v.z; m.w |= v.w; }
		if (__builtin_amdgcn_readfirstlane((int)(m.x | m.y | m.z | m.w)) == 0) break; // from LDS behind the barrier: workgroup-uniform
		u32 below[2], above[2];
#pragma unroll
		for (u32 h = 0; h < 2u; h++)
		{
			below[h] = Torus || wave ? xch[slot(buf, Torus ? (wave - 1u) & (kWaves - 1u) : wave - 1u, 1u, h, row)] : 0u; // z == -1: closed
			above[h] = Torus || wave + 1u < kWaves ? xch[slot(buf, (wave + 1u) & (kWaves - 1u), 0u, h, row)] : 0u; // z == 64: closed (the step wraps here)
		}
		u32 ch = 0;
#pragma unroll
		for (u32 p = 0; p < kPT; p++)
#pragma unroll
			for (u32 h = 0; h < 2u; h++)
			{
				const u32 z = Y[p][h] | (p ? Y[p ? p - 1u : 0u][h] : below[h]) | (p + 1u < kPT ? Y[p + 1u < kPT ? p + 1u : p][h] : above[h]);
				const u32 f = R[p][h] & z; // F is part of R and of its own dilation: f holds F
				ch |= f ^ F[p][h];
				F[p][h] = f;
			}
		changed = __ballot(ch != 0u) ? 1u : 0u;
	}
