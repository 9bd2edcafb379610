// Window kernels behind ca3d_cut_windows and ca3d_stamp_windows (include/ca3d.h): 64^3 regions of a packed G^3 grid, addressed as a
// torus, against 64^3 universes of an ensemble. Every window of a call in one launch.
//
// Layout. A grid word is x / 32 + y C + z C G with C = G / 32; a universe row (y, z) is two words at (z 64 + y) 2. Window row (j, k) at
// origin (ox, oy, oz) is the 64 bits at bit offset s = ox & 31 of THREE consecutive grid words wx, wx + 1, wx + 2 (wx = ox / 32, taken
// modulo C) of grid row ((oy + j) mod G, (oz + k) mod G). To and from the universe's two words is two funnel shifts; with s = 0 the third
// word takes no bit. At G = 64 (C = 2) with s != 0 the first and the third word are THE SAME grid word: a cut reads it twice and takes
// the low s bits of the row's end from its second reading; a stamp reaches it with two atomics that carry disjoint bits.
//
// Threads. One thread a row, 256 threads a workgroup, 16 workgroups a window: lane l of a wave has j = l, so a wave's universe side is
// 512 contiguous bytes, one 8-byte access a lane, and its grid side is 64 consecutive rows of one plane — G / 8 bytes apart, 12 bytes
// used of each, which is what the layout allows: a grid row IS the contiguous unit, and the rows of a window lie a whole grid row
// apart (at G = 64 the wave's rows are contiguous too). A wave that wraps in y touches two runs of rows.
//
// Overlaps. Windows of a stamp may overlap, and neighbouring windows share grid words even when they do not: every write to the grid
// is an atomicOr / atomicAnd whose result is not used (the compiler emits the vector global atomics without return). Zero words are
// skipped, and a universe row that is empty costs its 8-byte read alone. A cut writes universe words only, each exactly once: no atomics.
// No workgroup waits on another, nothing spins, no LDS, no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kRowsPerWindow = 64u * 64u;
constexpr u32 kWindowThreads = 256u;
constexpr u32 kGroupsPerWindow = kRowsPerWindow / kWindowThreads;

struct WindowArgs
{
	u32 *grid;
	u32 *state, *prev;
	const ca3d_window *windows;
	u32 G, C;
};

// where the thread's window row lies: the universe's row and the three grid words
struct WindowRow
{
	size_t uni;     // word offset of the universe row in the ensemble's state array
	size_t w[3];    // word offsets of the three grid words
	u32 s;          // bit offset of the row in the first
};

__device__ __forceinline__ WindowRow window_row(const WindowArgs &a)
{
	const u32 k = blockIdx.x / kGroupsPerWindow;
	const u32 row = (blockIdx.x % kGroupsPerWindow) * kWindowThreads + threadIdx.x; // z 64 + y of the universe
	const ca3d_window win = a.windows[k]; // the host has checked universe and origin
	u32 gy = win.origin[1] + (row & 63u), gz = win.origin[2] + (row >> 6); // below 2 G, since G >= 64
	gy -= gy >= a.G ? a.G : 0u;
	gz -= gz >= a.G ? a.G : 0u;
	WindowRow r;
	r.uni = (size_t)win.universe * kEnsembleWords + (size_t)row * 2u;
	r.s = win.origin[0] & 31u;
	const size_t base = ((size_t)gz * a.G + gy) * a.C; // the grid row: below G G C, the grid's words
	u32 wx = win.origin[0] >> 5; // below C
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
		r.w[i] = base + wx;
		wx = wx + 1u == a.C ? 0u : wx + 1u;
	}
	return r;
}

// (hi:lo) >> s, low word; s in 0 .. 31
__device__ __forceinline__ u32 funnel_r(u32 lo, u32 hi, u32 s) { return (u32)(((u64)hi << 32 | lo) >> s); }
// (hi:lo) << s, high word; s in 0 .. 31
__device__ __forceinline__ u32 funnel_l(u32 lo, u32 hi, u32 s) { return (u32)((((u64)hi << 32 | lo) << s) >> 32); }

__global__ __launch_bounds__(kWindowThreads) void ca_window_cut(WindowArgs a)
{
	const WindowRow r = window_row(a);
	const u32 w0 = a.grid[r.w[0]], w1 = a.grid[r.w[1]], w2 = a.grid[r.w[2]];
	const uint2 o = make_uint2(funnel_r(w0, w1, r.s), funnel_r(w1, w2, r.s));
	*reinterpret_cast<uint2 *>(a.state + r.uni) = o;
	*reinterpret_cast<uint2 *>(a.prev + r.uni) = o;
}

// the universe row's bits, where they fall in the three grid words
__device__ __forceinline__ void spread(uint2 v, u32 s, u32 out[3])
{
	out[0] = v.x << s;
	out[1] = funnel_l(v.x, v.y, s);
	out[2] = funnel_l(v.y, 0u, s);
}

template <bool kErase> __global__ __launch_bounds__(kWindowThreads) void ca_window_stamp(WindowArgs a)
{
	const WindowRow r = window_row(a);
	const uint2 v = *reinterpret_cast<const uint2 *>(a.state + r.uni);
	if ((v.x | v.y) == 0u) return;
	u32 bits[3];
	spread(v, r.s, bits);
#pragma unroll
	for (int i = 0; i < 3; i++)
		if (bits[i])
		{
			if (kErase) atomicAnd(a.grid + r.w[i], ~bits[i]);
			else atomicOr(a.grid + r.w[i], bits[i]);
		}
}

__global__ __launch_bounds__(kWindowThreads) void ca_window_clear(WindowArgs a)
{
	const WindowRow r = window_row(a);
	u32 bits[3];
	spread(make_uint2(~0u, ~0u), r.s, bits);
#pragma unroll
	for (int i = 0; i < 3; i++)
		if (bits[i]) atomicAnd(a.grid + r.w[i], ~bits[i]);
}

} // namespace

hipError_t launch_windows(const WindowLaunch &l, hipStream_t stream)
{
	static_assert(sizeof(ca3d_window) == 16, "a window is four words");
	if (l.n == 0 || l.n > kWindowsMax || l.G < 64u || l.G % 32u || !l.grid || !l.state || !l.windows) return hipErrorInvalidValue;
	if (l.op == kWindowCut && !l.prev) return hipErrorInvalidValue;
	WindowArgs a;
	a.grid = l.grid;
	a.state = l.state;
	a.prev = l.prev;
	a.windows = l.windows;
	a.G = l.G;
	a.C = l.G / 32u;
	const dim3 grid(l.n * kGroupsPerWindow), block(kWindowThreads);
	switch (l.op)
	{
	case kWindowCut: hipLaunchKernelGGL(ca_window_cut, grid, block, 0, stream, a); break;
	case kWindowOr: hipLaunchKernelGGL(ca_window_stamp<false>, grid, block, 0, stream, a); break;
	case kWindowErase: hipLaunchKernelGGL(ca_window_stamp<true>, grid, block, 0, stream, a); break;
	case kWindowClear: hipLaunchKernelGGL(ca_window_clear, grid, block, 0, stream, a); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

} // namespace ca3d
