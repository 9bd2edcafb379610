// A universe as an LDS image that can be read turned, and the constants of the 48 turns: shared by the kernels that assemble rows of a
// turned universe (ca_compose.hip, ca_canon.hip, ca_canon_period.hip; DESIGN.md 12.9 - 12.11). Device code only; include inside
// namespace ca3d { namespace { ... } }, after ca_flood.inc (u64).
//
// The image is two planes of words, [word][z][y] with 65 words a plane of rows: lanes that run along the universe's y are 1 word apart,
// lanes that run along its z 65 — both reach 32 different banks; with the natural [z][y][2] they would be 128 words apart, one bank.
// Orientation o = 6 f + m: m picks the axis permutation PERMS[m], bit d of f mirrors output axis d.
#pragma once

constexpr u32 kImgPlane = 65u;                 // words from one plane of rows to the next: odd, so lanes along z spread over the banks
constexpr u32 kImgHalf = 64u * kImgPlane;      // words of one of the two word planes
constexpr u32 kImgWords = 2u * kImgHalf;       // 33 280 B
constexpr u32 kPerm0 = 0u | 0u << 2 | 1u << 4 | 1u << 6 | 2u << 8 | 2u << 10; // PERMS[m][i], two bits an m
constexpr u32 kPerm1 = 1u | 2u << 2 | 0u << 4 | 2u << 6 | 0u << 8 | 1u << 10;
constexpr u32 kPerm2 = 2u | 1u << 2 | 2u << 4 | 0u << 6 | 1u << 8 | 0u << 10;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int pick(u32 j, int a, int b, int c) { return j == 0u ? a : j == 1u ? b : c; }
// v shifted left by t (right by -t), zero from |t| >= 64 on
__device__ __forceinline__ u64 shifted(u64 v, int t) { return t >= 64 || t <= -64 ? 0ull : t >= 0 ? v << (u32)t : v >> (u32)-t; }
