// One term of the state digest (include/ca3d.h, "digest"): the splitmix64 finaliser of (word index << 32 | word). Shared by every
// kernel that produces a ca3d_summary (ca_summary.hip, ca_ensemble.hip). Device code only.
#pragma once

__device__ __forceinline__ unsigned long long digest_mix(unsigned long long index, unsigned int w)
{
	unsigned long long z = ((index << 32) | (unsigned long long)w) + 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
