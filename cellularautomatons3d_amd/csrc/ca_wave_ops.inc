// Reductions over a wave of 64 lanes and over a row of 16 lanes, shared by the kernels that are compiled ahead of time (ca_ensemble.hip,
// ca_census.hip, ca_isolate.hip, ca_summary.hip). Not a run-time compiler source: nothing here is hashed into a cache key. Device code
// only; include inside namespace ca3d { namespace { ... } }, after ca_bitops.inc (u32, dpp_mov).
#pragma once

// ---- butterflies (__shfl_xor): the result in every lane ---------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_add(T v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ u32 wave_or(u32 v)
{
	for (int o = 32; o > 0; o >>= 1) v |= (u32)__shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ u32 wave_min(u32 v)
{
	for (int o = 32; o > 0; o >>= 1) v = min(v, (u32)__shfl_xor(v, o));
	return v;
}
__device__ __forceinline__ u32 wave_max(u32 v)
{
	for (int o = 32; o > 0; o >>= 1) v = max(v, (u32)__shfl_xor(v, o));
	return v;
}

// ---- DPP: a row of 16 lanes, and the four rows joined by the scalar unit -----------------------------------------
// The trace's sum over a wave, wave-uniform: four DPP adds leave every row of 16 lanes with its sum (lane ^ 1, lane ^ 2, the other quad
// pair, the other half), four v_readlane and three scalar adds join the rows. No LDS, and no lane-address registers that would stay
// alive across the steps, where the Moore step has none to spare (__shfl_xor's do).
__device__ __forceinline__ u32 row16_sum(u32 v)
{
	v += dpp_mov<1 | (0 << 2) | (3 << 4) | (2 << 6)>(v); // quad_perm:[1,0,3,2]
	v += dpp_mov<2 | (3 << 2) | (0 << 4) | (1 << 6)>(v); // quad_perm:[2,3,0,1]
	v += dpp_mov<0x141>(v);                              // row_half_mirror
	v += dpp_mov<0x140>(v);                              // row_mirror
	return v;
}
__device__ __forceinline__ u32 wave_sum_uniform(u32 v)
{
	v = row16_sum(v);
	return (u32)__builtin_amdgcn_readlane((int)v, 0) + (u32)__builtin_amdgcn_readlane((int)v, 16) + (u32)__builtin_amdgcn_readlane((int)v, 32) +
	       (u32)__builtin_amdgcn_readlane((int)v, 48);
}

// The same for an OR (the *_moving kernels' x-occupancy words).
__device__ __forceinline__ u32 row16_or(u32 v)
{
	v |= dpp_mov<1 | (0 << 2) | (3 << 4) | (2 << 6)>(v); // quad_perm:[1,0,3,2]
	v |= dpp_mov<2 | (3 << 2) | (0 << 4) | (1 << 6)>(v); // quad_perm:[2,3,0,1]
	v |= dpp_mov<0x141>(v);                              // row_half_mirror
	v |= dpp_mov<0x140>(v);                              // row_mirror
	return v;
}
__device__ __forceinline__ u32 wave_or_uniform(u32 v)
{
	v = row16_or(v);
	return (u32)__builtin_amdgcn_readlane((int)v, 0) | (u32)__builtin_amdgcn_readlane((int)v, 16) | (u32)__builtin_amdgcn_readlane((int)v, 32) |
	       (u32)__builtin_amdgcn_readlane((int)v, 48);
}
