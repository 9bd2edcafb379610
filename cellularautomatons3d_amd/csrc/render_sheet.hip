// Contact sheet of an ensemble for gfx950: universes first .. first + count - 1 of a ca3d_ensemble, each drawn as one tile of a sheet,
// in one launch (ca3d_ensemble_render_sheet). Tile k is, bit for bit, the converged frame ca3d_render draws of that universe at the
// tile's size with the cell-by-cell walk ("render_skip" 0): every sample goes through shade_sample_with (render_device.inc), the
// walk is walk_from — the plain kernel's walk body — and the pixel's sums and stores are ca_render_packed's.
//
// What is new is where the walk reads the volume. A 64^3 universe is 8192 words, 32 KiB: a workgroup copies its universe into LDS
// once and walks every view and shadow ray of its pixels there (four workgroups a CU: 128 of the 160 KiB). The one cell_state read
// per sample stays on global memory (P.cells).
//
// Built with -ffp-contract=off like the other renderer files: without it the frame is no longer the plain kernel's.
#include <hip/hip_fp16.h>

#include "ca3d_internal.h"

namespace ca3d
{
namespace
{

#include "render_device.inc"

constexpr u32 kSheetWords = kEnsembleWords; // of one universe

// ... or the workgroup's copy of it in LDS
struct LdsWords
{
	const u32 *vol;
	__device__ __forceinline__ u32 operator()(const RenderParams &, int key) const { return vol[key]; }
};

// WalkTracer<false> with the volume's words read from LDS
struct LdsTracer
{
	static constexpr bool kSkipBox = false, kStopAfterPrimary = false, kStopAfterShadow = false;
	LdsWords words;
	u32 &pvis, &svis;
	__device__ __forceinline__ bool primary(const RenderParams &P, v3 cam, v3 ray, v3 enter, v3 dir, float len, v3 vhalf, float &tnear)
	{
		return walk_from<false, false>(P, enter, dir, 0.0f, len, vhalf, 0, 0, 0, tnear, pvis, words);
	}
	__device__ __forceinline__ bool shadow(const RenderParams &P, v3 p, v3 dir, float len, v3 vhalf, int cx, int cy, int cz)
	{
		float dummy = 0.0f;
		return walk_from<true, false>(P, p, dir, 0.0025f, len, vhalf, cx, cy, cz, dummy, svis, words);
	}
};

struct SheetParams
{
	RenderParams base; // W, H: the TILE's size (a sample's vu, vv are those of the tile's own frame); cells: universe `first`; targets: the sheet's
	u32 columns;       // tiles per sheet row
	u32 sheet_w;       // columns * W: pixels per sheet row
	u32 shares;        // S: workgroups per universe; workgroup b draws universe b / S, blocks b % S, b % S + S, ... of its tile
};

// One workgroup = one universe (and one share of its tile's 16 x 16-pixel blocks). (256, 4): four workgroups a CU is what the LDS
// copy allows (4 x 32 KiB) and 128 VGPRs is what the plain kernel is compiled for.
__global__ __launch_bounds__(256, 4) void ca_render_sheet64(SheetParams S)
{
	__shared__ __attribute__((aligned(16))) u32 vol[kSheetWords];
	const u32 k = blockIdx.x / S.shares, share = blockIdx.x % S.shares;
	// what the compiler may know of this kernel's volume: 64^3 packed, no legacy shading, no indirect term, nothing to skip by
	RenderParams P = S.base;
	P.cells = S.base.cells + (size_t)k * kSheetWords;
	P.G = 64u;
	P.cols = 2u;
	P.legacy = 0u;
	P.indirect = 0u;
	P.occ = nullptr;
	P.live_box = nullptr;
	{
		const uint4 *src = reinterpret_cast<const uint4 *>(P.cells);
		uint4 *dst = reinterpret_cast<uint4 *>(vol);
#pragma unroll
		for (u32 i = 0; i < kSheetWords / 4u / 256u; i++) dst[i * 256u + threadIdx.x] = src[i * 256u + threadIdx.x];
	}
	__syncthreads();
	const u32 bw = P.W / 16u, nblocks = bw * (P.H / 16u); // (tile sizes are multiples of 16: ca3d_ensemble_render_sheet)
	const u32 x0 = (k % S.columns) * P.W, y0 = (k / S.columns) * P.H; // the tile's corner in the sheet
	u32 shadow = 0, pvis = 0, svis = 0;
	LdsTracer tr{LdsWords{vol}, pvis, svis};
	for (u32 blk = share; blk < nblocks; blk += S.shares)
	{
		const u32 px = (blk % bw) * 16u + (threadIdx.x & 15u);
		const u32 py = (blk / bw) * 16u + (threadIdx.x >> 4);
		float r = 0.0f, g = 0.0f, b = 0.0f, a = 0.0f, d0 = 0.0f;
		for (u32 s4 = 0; s4 < P.spp; s4++)
		{
			const float ox = P.spp == 1u ? 0.5f : ((s4 & 1u) ? 0.75f : 0.25f);
			const float oy = P.spp == 1u ? 0.5f : ((s4 & 2u) ? 0.75f : 0.25f);
			const float vu = ((float)px + ox) / (float)P.W, vv = 1.0f - ((float)py + oy) / (float)P.H;
			const Sample s = shade_sample_with(P, vu, vv, tr);
			r += s.r; g += s.g; b += s.b; a += s.a;
			if (s4 == 0) d0 = s.depth;
			shadow += s.shadow_ray;
		}
		const float inv = 1.0f / (float)P.spp;
		r *= inv; g *= inv; b *= inv; a *= inv;
		const size_t i = (size_t)(y0 + py) * S.sheet_w + (x0 + px);
		if (P.light)
		{
			const __half2 rg = __floats2half2_rn(r, g), ba = __floats2half2_rn(b, 1.0f);
			uint2 v;
			v.x = *reinterpret_cast<const u32 *>(&rg);
			v.y = *reinterpret_cast<const u32 *>(&ba);
			P.light[i] = v;
		}
		if (P.depth)
		{
			const __half2 d = __floats2half2_rn(d0, 1.0f);
			P.depth[i] = *reinterpret_cast<const u32 *>(&d);
		}
		if (P.presentation)
		{
			const float ig = 1.0f / P.u[U_GAMMA];
			P.presentation[i] = unorm8(powf(r, ig)) | (unorm8(powf(g, ig)) << 8) | (unorm8(powf(b, ig)) << 16) | (unorm8(a) << 24);
		}
	}
	if (P.counters && (shadow | pvis | svis) != 0u)
	{
		atomicAdd(&P.counters[0], (unsigned long long)shadow);
		atomicAdd(&P.counters[1], (unsigned long long)pvis);
		atomicAdd(&P.counters[2], (unsigned long long)svis);
	}
}

} // namespace

// S: a universe's blocks are dealt to as few workgroups as still fill the chip's kSheetPerCu x CUs workgroup slots — each one pays for
// a 32 KiB copy — and to no more than it has blocks. `count` universes >= slots: one workgroup a universe.
uint32_t sheet_shares(uint32_t count, uint32_t blocks, uint32_t slots)
{
	const uint32_t want = (slots + count - 1u) / count;
	return want < 1u ? 1u : (want > blocks ? blocks : want);
}

hipError_t launch_render_sheet(const SheetLaunch &l, hipStream_t stream)
{
	SheetParams S{};
	RenderParams &P = S.base;
	P.cells = l.state + (size_t)l.first * kEnsembleWords;
	P.G = 64u;
	P.cols = 2u;
	P.W = l.tile_w;
	P.H = l.tile_h;
	P.spp = l.spp;
	P.cot_half_fov = (float)(1.0 / tan(37.5 * 3.14159265359 / 180.0)); // COT_HALF_FOV :70 (launch_render's)
	for (int i = 0; i < U_LIVE; i++) P.u[i] = l.uniforms[i];
	P.presentation = l.presentation;
	P.light = reinterpret_cast<uint2 *>(l.light);
	P.depth = l.depth;
	P.counters = l.counters;
	S.columns = l.columns;
	S.sheet_w = l.columns * l.tile_w;
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	S.shares = sheet_shares(l.count, (l.tile_w / 16u) * (l.tile_h / 16u), (uint32_t)cus * 4u);
	// the tile slots past `count` in the last sheet row: that row of tiles is one piece of memory in each target, cleared in front of the launch
	if (l.count % l.columns)
	{
		const size_t row_px = (size_t)S.sheet_w * l.tile_h, at = (size_t)(l.count / l.columns) * row_px;
		hipError_t e = hipSuccess;
		if (l.presentation) e = hipMemsetAsync(l.presentation + at, 0, row_px * 4u, stream);
		if (e == hipSuccess && l.light) e = hipMemsetAsync(reinterpret_cast<uint2 *>(l.light) + at, 0, row_px * 8u, stream);
		if (e == hipSuccess && l.depth) e = hipMemsetAsync(l.depth + at, 0, row_px * 4u, stream);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(ca_render_sheet64, dim3(l.count * S.shares), dim3(256), 0, stream, S);
	return hipGetLastError();
}

} // namespace ca3d
