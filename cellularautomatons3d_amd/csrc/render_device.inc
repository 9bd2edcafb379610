// Device code shared by the renderer's translation units (render.hip: plain / in-wave scheduled / literal-frame kernels;
// render_stream.hip: the ray-stream pipeline; render_sheet.hip: the ensemble's contact sheet): vector helpers, the launch parameters, the reference's slab test / sdBox /
// face normal / Cook-Torrance BRDF (shaders/pathtraced_fragment_clustered.wgsl:182-254, 537-633), occupancy helpers, the exact
// cell walk, and shade_sample — the ONE statement of a sample's arithmetic that every kernel instantiates.
// Included inside `namespace ca3d { namespace {`; built with -ffp-contract=off (the parity target is a plain-float CPU restatement).
using u32 = uint32_t;

struct v3
{
	float x, y, z;
};
__device__ __forceinline__ v3 V(float x, float y, float z) { return v3{x, y, z}; }
__device__ __forceinline__ v3 operator+(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 operator-(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 operator*(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ v3 operator*(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot3(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float len3(v3 a) { return sqrtf(dot3(a, a)); }
__device__ __forceinline__ v3 norm3(v3 a) { const float l = len3(a); return V(a.x / l, a.y / l, a.z / l); }

// float indices of the 128-float uniform block (MemoryManager allocation order, main_pathtraced.js:166,
// 467-478 == struct CommonBufferLayout, pathtraced_fragment_clustered.wgsl:17-34)
enum
{
	U_LIGHT = 0, U_VIEW = 4, U_PROJVIEWINV = 20, U_PREVVIEW = 36, U_PREVPROJVIEWINV = 52, U_WINDOW = 68, U_TIME = 70,
	U_DEPTHSAMPLES = 71, U_SHADOWSAMPLES = 72, U_CELLSIZE = 73, U_SHOWDEPTH = 74, U_TEMPORALALPHA = 75,
	U_REFLECTIVITY = 76, U_ROUGHNESS = 79, U_MATERIALCOLOR = 80, U_GAMMA = 83, U_LIVE = 84
};

struct RenderParams
{
	const u32 *cells;
	u32 G, cols; // cols = G / 32
	u32 W, H, spp;
	float cot_half_fov;
	float u[U_LIVE];
	u32 *presentation;         // RGBA8
	uint2 *light;              // RGBA16F
	u32 *depth;                // RG16F
	unsigned long long *counters; // [0] shadow rays, [1] primary cell visits, [2] shadow cell visits
	u32 legacy; // 1: one-u32-per-cell volume + the shading of shaders/pathtraced_fragment.wgsl (R-legacy)
	const unsigned long long *occ; // block occupancy (ca_occupancy) or null; the word after the bits counts the set bits
	u32 occ_words;                 // 64-bit words of (fine) occupancy bits
	u32 occ_coarse;                // != 0: coarse bits (blocks of 128 x 32 x 32 cells) follow the count word
	u32 row0, row1; // only image rows [row0, row1) are rendered (a rank's band of a frame shared between GPUs); row0 is a multiple of 16
	u32 indirect;   // add calculateIndirectLighting (:307-377), the term the reference leaves commented out at :424
	u32 trace;      // diagnostics (CA3D_RENDER_TRACE): counters + 8 + 4 * tile receives {start, end (s_memrealtime), HW_ID, cell visits}
	// The volume's screen rectangle, pixels [rx0, rx1) x [ry0, ry1) (x a multiple of 32, y of 16 from row0; clipped to the band): the
	// scheduled kernel takes the wave tiles inside it from a queue (counters[3]); the plain kernel, launched with
	// outside_only, renders the 16 x 16 tiles outside it (view rays that miss the volume: no walk to schedule).
	u32 rx0, rx1, ry0, ry1, outside_only;
	// Box around the occupied blocks (32 x 8 x 8 cells each), in cells (ca_occupancy): [0] x1, [1] ~x0, [2] y1, [3] ~y0, [4] z1, [5] ~z0, each the
	// maximum over the occupied blocks (zero-initialised: an empty volume gives x0 > x1), or null. A view ray that misses it cannot
	// meet a live cell: the sparse-volume kernels answer "no hit" without walking.
	const u32 *live_box;
	// Round 5: pixels NOTHING can be seen in are not traced. bg != 0: ca_render_background fills the 16 x 16 tiles outside the volume's
	// rectangle with the constant a missed view ray gives, except the tiles of the light gizmo's rectangle [gx0, gx1) x [gy0, gy1) (16-aligned),
	// which it traces; in a small-live-box frame the tiles outside the live box's rectangle get the one thing a miss leaves (the depth
	// of the volume's far side, from sample 0) and ca_render_packed_spread walks the rest.
	u32 bg, gx0, gx1, gy0, gy1;
	u32 spread; // the launch includes ca_render_packed_spread: a small live box is its frame, not the plain kernel's
	u32 park;   // scheduled kernel: lanes that stand on a live cell park until this many wait for the hit test (0: test at once)
};

constexpr float kPi = 3.14159265359f;
constexpr float kHalf = 0.5f;
constexpr float kOcclusion = 0.0095f;

// (v + 0.5) / cellSize, the shaders' `(p + 0.5) / cs` — for a power-of-two grid cs = 2^-k and the division is a multiplication by
// G, bit for bit (scaling by a power of two is exact); other grids keep the division. Wave-uniform choice.
__device__ __forceinline__ float to_cells(const RenderParams &P, float v)
{
	const float cs = 1.0f / (float)P.G;
	return (P.G & (P.G - 1u)) == 0u ? (v + kHalf) * (float)P.G : (v + kHalf) / cs;
}

__device__ __forceinline__ u32 cell_state(const RenderParams &P, u32 x, u32 y, u32 z)
{
	// legacy: cellStates[x + y*G + z*G*G], no wrap (pathtraced_fragment.wgsl:157-168). A point on the volume's
	// boundary can floor to G or -1: the reference then indexes outside its buffer, which WebGPU's robust buffer
	// access turns into a harmless read; here such a cell is simply dead.
	if (P.legacy)
	{
		if (x >= P.G || y >= P.G || z >= P.G) return 0u;
		return P.cells[(size_t)x + (size_t)y * P.G + (size_t)z * P.G * P.G] == 1u ? 1u : 0u;
	}
	// :268-290 — every coordinate wraps modulo the grid
	if ((P.G & (P.G - 1u)) == 0u) // power-of-two grid: the three modulo operations are masks (a u32 % by a run-time value is ~25 instructions)
	{
		const u32 idx = ((x >> 5) & (P.cols - 1u)) + (y & (P.G - 1u)) * P.cols + (z & (P.G - 1u)) * P.cols * P.G;
		return (P.cells[idx] >> (x & 31u)) & 1u;
	}
	const u32 idx = ((x >> 5) % P.cols) + (y % P.G) * P.cols + (z % P.G) * P.cols * P.G;
	return (P.cells[idx] >> (x & 31u)) & 1u;
}

__device__ __forceinline__ void ray_cube(v3 o, v3 d, v3 center, v3 half, float &tnear, float &tfar)
{
	// :212-225
	const v3 inv = V(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const v3 tmin = ((center - half) - o) * inv;
	const v3 tmax = ((center + half) - o) * inv;
	const v3 t1 = V(fminf(tmin.x, tmax.x), fminf(tmin.y, tmax.y), fminf(tmin.z, tmax.z));
	const v3 t2 = V(fmaxf(tmin.x, tmax.x), fmaxf(tmin.y, tmax.y), fmaxf(tmin.z, tmax.z));
	tnear = fmaxf(fmaxf(t1.x, t1.y), t1.z);
	tfar = fminf(fminf(t2.x, t2.y), t2.z);
}

// The same test with 1 / d handed in (bit-identical: ray_cube forms exactly this `inv` first). A walk tests many cells along
// one ray: three correctly rounded divisions (~10 instructions each) per live cell become three per ray.
__device__ __forceinline__ void ray_cube_inv(v3 o, v3 inv, v3 center, v3 half, float &tnear, float &tfar)
{
	const v3 tmin = ((center - half) - o) * inv;
	const v3 tmax = ((center + half) - o) * inv;
	const v3 t1 = V(fminf(tmin.x, tmax.x), fminf(tmin.y, tmax.y), fminf(tmin.z, tmax.z));
	const v3 t2 = V(fmaxf(tmin.x, tmax.x), fmaxf(tmin.y, tmax.y), fmaxf(tmin.z, tmax.z));
	tnear = fmaxf(fmaxf(t1.x, t1.y), t1.z);
	tfar = fminf(fminf(t2.x, t2.y), t2.z);
}

__device__ __forceinline__ float sd_box(v3 p, v3 b)
{
	// :182-186
	const v3 q = V(fabsf(p.x) - b.x, fabsf(p.y) - b.y, fabsf(p.z) - b.z);
	const v3 m = V(fmaxf(q.x, 0.0f), fmaxf(q.y, 0.0f), fmaxf(q.z, 0.0f));
	return len3(m) + fminf(fmaxf(q.x, fmaxf(q.y, q.z)), 0.0f);
}

__device__ __forceinline__ v3 face_normal(v3 p, v3 origin)
{
	// :227-254
	const v3 d = p - origin;
	const v3 a = V(fabsf(d.x), fabsf(d.y), fabsf(d.z));
	const float m = fmaxf(fmaxf(a.x, a.y), a.z);
	v3 n;
	if (a.x == m) n = V(d.x, 0.0f, 0.0f);
	else if (a.y == m) n = V(0.0f, d.y, 0.0f);
	else n = V(0.0f, 0.0f, d.z);
	return norm3(n);
}

__device__ __forceinline__ v3 cell_origin(float cs, int x, int y, int z)
{
	return V((float)x * cs + cs * 0.5f - kHalf, (float)y * cs + cs * 0.5f - kHalf, (float)z * cs + cs * 0.5f - kHalf);
}

__device__ v3 surface_brdf(v3 L, v3 Vd, v3 N, float roughness, v3 albedo, v3 F0)
{
	// :537-592
	const v3 Hh = norm3(L + Vd);
	const v3 fL = V(albedo.x / kPi, albedo.y / kPi, albedo.z / kPi);
	const float a2 = roughness * roughness;
	const float NoH = dot3(N, Hh);
	const float NoH2 = NoH * NoH;
	const float f = NoH2 * (a2 - 1.0f) + 1.0f;
	const float D = a2 / (kPi * f * f);
	const float n = roughness + 1.0f;
	const float k = (n * n) / 8.0f;
	const float NoV = fmaxf(0.0f, dot3(N, Vd));
	const float gv = NoV / (NoV * (1.0f - k) + k);
	const float NoL = fmaxf(0.0f, dot3(N, L));
	const float gl = NoL / (NoL * (1.0f - k) + k);
	const float Gm = gv * gl;
	const float p = powf(1.0f - dot3(Hh, Vd), 5.0f);
	const v3 F = V(F0.x + (1.0f - F0.x) * p, F0.y + (1.0f - F0.y) * p, F0.z + (1.0f - F0.z) * p);
	const float denom = 4.0f * dot3(Vd, N) * dot3(L, N);
	return V(fL.x + (D * Gm * F.x) / denom, fL.y + (D * Gm * F.y) / denom, fL.z + (D * Gm * F.z) / denom);
}

// calculateLightingAt :594-633 with a vec3 incident light arriving from `light_pos` (the direct term passes the light
// source's magnitude and position, the indirect term a neighbour cell's reflected light and the point it leaves from)
__device__ v3 lighting_from(const RenderParams &P, v3 p, v3 origin, u32 cx, u32 cy, v3 eye, v3 incident, v3 light_pos)
{
	const float *u = P.u;
	const v3 N = face_normal(p, origin);
	const float Gf = (float)P.G;
	const float cxn = (float)cx / Gf, cyn = (float)cy / Gf;
	v3 albedo = V(cxn, cyn, 1.0f - cxn);
	if (u[U_MATERIALCOLOR] != 0.0f || u[U_MATERIALCOLOR + 1] != 0.0f || u[U_MATERIALCOLOR + 2] != 0.0f)
		albedo = V(u[U_MATERIALCOLOR], u[U_MATERIALCOLOR + 1], u[U_MATERIALCOLOR + 2]);
	const v3 Vd = norm3(eye - p);
	const v3 L = norm3(light_pos - p);
	const v3 F0 = V(u[U_REFLECTIVITY], u[U_REFLECTIVITY + 1], u[U_REFLECTIVITY + 2]);
	const v3 brdf = surface_brdf(L, Vd, N, u[U_ROUGHNESS], albedo, F0);
	const float LoN = dot3(L, N);
	return V(fmaxf(0.0f, brdf.x * incident.x * LoN), fmaxf(0.0f, brdf.y * incident.y * LoN), fmaxf(0.0f, brdf.z * incident.z * LoN));
}

// ---- empty-space skipping ------------------------------------------------------------------------------------
// One occupancy bit per block of 32 x 8 x 8 cells (ca_occupancy below). When the walk enters an empty block it
// jumps to the block's exit face and re-seeds its boundary times in closed form there. Used only on sparse volumes
// (< 1/4 of the blocks occupied, decided per frame from the bit count): there it visits the same cells as the
// cell-by-cell walk except where a ray grazes a cell corner within rounding (re-seeded times are not the accumulated
// ones) — inside the renderer's stated tolerance, not bit-identical to the unskipped walk.
__device__ __forceinline__ bool occ_skip_enabled(const RenderParams &P)
{
	if (!P.occ) return false;
	const unsigned long long set = P.occ[P.occ_words];
	return set * 4ull < (unsigned long long)P.cols * (P.G >> 3) * (P.G >> 3);
}

// true: the ray o + t d (t >= 0) stays outside the box of the occupied blocks, grown by one cell — it cannot enter a live cell, and
// the walk along it would come back empty-handed. A NaN in the slab test (a zero direction component on a slab face) reads as
// "may hit".
__device__ __forceinline__ bool misses_live_box(const RenderParams &P, v3 o, v3 d)
{
	if (!P.live_box) return false;
	const u32 x1 = P.live_box[0], x0 = ~P.live_box[1], y1 = P.live_box[2], y0 = ~P.live_box[3], z1 = P.live_box[4], z0 = ~P.live_box[5];
	if (x0 >= x1) return true; // nothing alive
	const float cs = 1.0f / (float)P.G;
	const v3 lo = V((float)x0 * cs - kHalf - cs, (float)y0 * cs - kHalf - cs, (float)z0 * cs - kHalf - cs);
	const v3 hi = V((float)x1 * cs - kHalf + cs, (float)y1 * cs - kHalf + cs, (float)z1 * cs - kHalf + cs);
	float tn, tf;
	ray_cube(o, d, V(0.5f * (lo.x + hi.x), 0.5f * (lo.y + hi.y), 0.5f * (lo.z + hi.z)), V(0.5f * (hi.x - lo.x), 0.5f * (hi.y - lo.y), 0.5f * (hi.z - lo.z)), tn, tf);
	return tn > tf || tf < 0.0f;
}

// A sparse volume whose live cells sit in a small box (under an eighth of the grid: the reference's start-up seed) is rendered by
// the plain kernel alone: nearly every ray is answered by misses_live_box, and the few tiles that walk are next to each other —
// per-wave ray scheduling has nothing to schedule there and its 256-job tiles serialise the only work there is (measured on the
// start-up scene, 1080p 4 spp: 2.2 ms scheduled, 0.76 ms plain; volumes with live cells everywhere: 5.0 vs 6.3 ms).
__device__ __forceinline__ bool live_box_small(const RenderParams &P)
{
	if (!P.live_box) return false;
	const u32 x1 = P.live_box[0], x0 = ~P.live_box[1], y1 = P.live_box[2], y0 = ~P.live_box[3], z1 = P.live_box[4], z0 = ~P.live_box[5];
	if (x0 >= x1) return true;
	return (unsigned long long)(x1 - x0) * (y1 - y0) * (z1 - z0) * 8ull < (unsigned long long)P.G * P.G * P.G;
}

__device__ __forceinline__ bool block_occupied(const RenderParams &P, int ix, int iy, int iz)
{
	const int bk = (ix >> 5) + ((iy >> 3) + (iz >> 3) * ((int)P.G >> 3)) * (int)P.cols;
	return (P.occ[bk >> 6] >> (bk & 63)) & 1ull;
}

// second level: blocks of 128 x 32 x 32 cells (4 x 4 x 4 fine blocks), grids that are multiples of 128 only
__device__ __forceinline__ bool coarse_occupied(const RenderParams &P, int ix, int iy, int iz)
{
	const int ck = (ix >> 7) + ((iy >> 5) + (iz >> 5) * ((int)P.G >> 5)) * ((int)P.cols >> 2);
	return (P.occ[P.occ_words + 1u + (u32)(ck >> 6)] >> (ck & 63)) & 1ull;
}

// The ray is in cell (ix, iy, iz) of an empty block: move to the first cell past the block. false: the ray ends or
// leaves the volume first.
template <int LX, int LY, int LZ> // log2 of the block's extent in cells
__device__ __forceinline__ bool block_jump(const RenderParams &P, v3 start, v3 dir, v3 inv, float tmax, int &ix, int &iy, int &iz, float &t,
                                           float &tx, float &ty, float &tz)
{
	constexpr int BX = 1 << LX, BY = 1 << LY, BZ = 1 << LZ;
	const int G = (int)P.G;
	const float cs = 1.0f / (float)P.G, big = 3.0e38f;
	const int sx = dir.x > 0.0f ? 1 : -1, sy = dir.y > 0.0f ? 1 : -1, sz = dir.z > 0.0f ? 1 : -1;
	const int bx0 = ix & ~(BX - 1), by0 = iy & ~(BY - 1), bz0 = iz & ~(BZ - 1);
	const float tex = dir.x != 0.0f ? (((float)(sx > 0 ? bx0 + BX : bx0) * cs - kHalf) - start.x) * inv.x : big;
	const float tey = dir.y != 0.0f ? (((float)(sy > 0 ? by0 + BY : by0) * cs - kHalf) - start.y) * inv.y : big;
	const float tez = dir.z != 0.0f ? (((float)(sz > 0 ? bz0 + BZ : bz0) * cs - kHalf) - start.z) * inv.z : big;
	const bool mx = tex <= tey && tex <= tez, my = !mx && tey <= tez;
	const float te = mx ? tex : (my ? tey : tez);
	if (te >= tmax) return false;
	const v3 p = start + dir * te;
	int nx = min(max((int)floorf(to_cells(P, p.x)), bx0), bx0 + BX - 1);
	int ny = min(max((int)floorf(to_cells(P, p.y)), by0), by0 + BY - 1);
	int nz = min(max((int)floorf(to_cells(P, p.z)), bz0), bz0 + BZ - 1);
	if (mx) nx = sx > 0 ? bx0 + BX : bx0 - 1;
	else if (my) ny = sy > 0 ? by0 + BY : by0 - 1;
	else nz = sz > 0 ? bz0 + BZ : bz0 - 1;
	if ((u32)nx >= (u32)G || (u32)ny >= (u32)G || (u32)nz >= (u32)G) return false;
	ix = nx; iy = ny; iz = nz;
	t = te;
	tx = dir.x != 0.0f ? (((float)(ix + (sx > 0 ? 1 : 0)) * cs - kHalf) - start.x) * inv.x : big;
	ty = dir.y != 0.0f ? (((float)(iy + (sy > 0 ? 1 : 0)) * cs - kHalf) - start.y) * inv.y : big;
	tz = dir.z != 0.0f ? (((float)(iz + (sz > 0 ? 1 : 0)) * cs - kHalf) - start.z) * inv.z : big;
	return true;
}

// Round 5: a sparse-volume walk is clipped to the box of the occupied blocks grown by one cell (misses_live_box's box) — no live cell
// lies outside it, so what the walk finds is unchanged. The start-up scene's rays crossed some 200 empty cells (25 block jumps, each a
// dependent occupancy read and three divisions) before they reached the blob and as many behind it: now a ray enters the box in
// ONE jump (re-seeded in closed form like block_jump; not counted as a visit) and ends where it leaves the box. A NaN in the slab
// test (a zero direction component on a slab face) fails every comparison below: such a ray is walked unclipped.
// false: the ray stays outside the box — no walk. Shared by walk() and the scheduled kernel's walk_begin (render.hip): same cells, same counts.
__device__ __forceinline__ bool live_box_clip(const RenderParams &P, v3 start, v3 dir, v3 inv, float t0, float &tmax, int &ix, int &iy, int &iz,
                                              float &t, float &tx, float &ty, float &tz)
{
	const int G = (int)P.G;
	const float cs = 1.0f / (float)P.G, big = 3.0e38f;
	const u32 bx1 = P.live_box[0], bx0 = ~P.live_box[1], by1 = P.live_box[2], by0 = ~P.live_box[3], bz1 = P.live_box[4], bz0 = ~P.live_box[5];
	if (bx0 >= bx1) return false; // nothing alive
	const v3 lo = V((float)bx0 * cs - kHalf - cs, (float)by0 * cs - kHalf - cs, (float)bz0 * cs - kHalf - cs);
	const v3 hi = V((float)bx1 * cs - kHalf + cs, (float)by1 * cs - kHalf + cs, (float)bz1 * cs - kHalf + cs);
	float bn, bf;
	ray_cube_inv(start, inv, V(0.5f * (lo.x + hi.x), 0.5f * (lo.y + hi.y), 0.5f * (lo.z + hi.z)), V(0.5f * (hi.x - lo.x), 0.5f * (hi.y - lo.y), 0.5f * (hi.z - lo.z)), bn, bf);
	if (bn > bf || bf < t0) return false;
	if (bf < tmax) tmax = bf;
	if (bn > t0 + cs)
	{
		if (bn >= tmax) return false;
		const int sx = dir.x > 0.0f ? 1 : -1, sy = dir.y > 0.0f ? 1 : -1, sz = dir.z > 0.0f ? 1 : -1;
		const v3 q = start + dir * bn;
		ix = min(max((int)floorf(to_cells(P, q.x)), 0), G - 1);
		iy = min(max((int)floorf(to_cells(P, q.y)), 0), G - 1);
		iz = min(max((int)floorf(to_cells(P, q.z)), 0), G - 1);
		t = bn;
		tx = dir.x != 0.0f ? (((float)(ix + (sx > 0 ? 1 : 0)) * cs - kHalf) - start.x) / dir.x : big;
		ty = dir.y != 0.0f ? (((float)(iy + (sy > 0 ? 1 : 0)) * cs - kHalf) - start.y) / dir.y : big;
		tz = dir.z != 0.0f ? (((float)(iz + (sz > 0 ? 1 : 0)) * cs - kHalf) - start.z) / dir.z : big;
	}
	return true;
}

// Where a walk gets the packed word `key` of the volume from: the state in global memory ...
struct GlobalWords
{
	__device__ __forceinline__ u32 operator()(const RenderParams &P, int key) const { return P.cells[key]; }
};

// Exact cell walk (Amanatides-Woo) from `start` along unit `dir` over (t0, tmax). SHADOW selects the visit test.
// Returns true on a hit; `tnear_out` is the slab entry of the hit cube (primary only). `fetch` reads a packed word (GlobalWords, or a
// copy of the volume somewhere closer: render_sheet.hip) — the ONE walk body whatever the words come from.
template <bool SHADOW, bool SKIP, class Fetch>
__device__ __forceinline__ bool walk_from(const RenderParams &P, v3 start, v3 dir, float t0, float tmax, v3 half, int sx0, int sy0, int sz0,
                                          float &tnear_out, u32 &visits, const Fetch &fetch)
{
	const int G = (int)P.G;
	const float cs = 1.0f / (float)P.G;
	const v3 p = start + dir * t0;
	int ix = (int)floorf(to_cells(P, p.x)), iy = (int)floorf(to_cells(P, p.y)), iz = (int)floorf(to_cells(P, p.z));
	ix = min(max(ix, 0), G - 1);
	iy = min(max(iy, 0), G - 1);
	iz = min(max(iz, 0), G - 1);
	const int sx = dir.x > 0.0f ? 1 : -1, sy = dir.y > 0.0f ? 1 : -1, sz = dir.z > 0.0f ? 1 : -1;
	const float big = 3.0e38f;
	float tx = dir.x != 0.0f ? (((float)(ix + (sx > 0 ? 1 : 0)) * cs - kHalf) - start.x) / dir.x : big;
	float ty = dir.y != 0.0f ? (((float)(iy + (sy > 0 ? 1 : 0)) * cs - kHalf) - start.y) / dir.y : big;
	float tz = dir.z != 0.0f ? (((float)(iz + (sz > 0 ? 1 : 0)) * cs - kHalf) - start.z) / dir.z : big;
	const float dx = dir.x != 0.0f ? cs / fabsf(dir.x) : big, dy = dir.y != 0.0f ? cs / fabsf(dir.y) : big,
	            dz = dir.z != 0.0f ? cs / fabsf(dir.z) : big;
	float t = t0;
	const v3 inv = V(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z); // what ray_cube forms first: once per ray, not once per live cell
	if (SKIP && P.live_box && !live_box_clip(P, start, dir, inv, t0, tmax, ix, iy, iz, t, tx, ty, tz)) return false;
	// one packed word covers 32 x-cells of a row: keep it in a register while the walk stays inside it
	u32 word = 0;
	int wkey = -1, okey = -1;
	for (int guard = 0; guard < 3 * G + 3; guard++)
	{
		if (t >= tmax) return false;
		visits++;
		if (SKIP)
		{
			// (the block the last cell was found occupied in is remembered: the cells of one 32 x 8 x 8 block ask the two occupancy words —
			// two dependent reads in front of the cell's own — once, not once per cell; same answers, a third of the memory round trips
			// of a walk through the start-up scene's blob, where a lone wave's chain of them is what a frame waits for)
			const int bk = (ix >> 5) + ((iy >> 3) + (iz >> 3) * (G >> 3)) * (int)P.cols;
			if (bk != okey)
			{
				if (P.occ_coarse && !coarse_occupied(P, ix, iy, iz))
				{
					if (!block_jump<7, 5, 5>(P, start, dir, inv, tmax, ix, iy, iz, t, tx, ty, tz)) return false;
					continue;
				}
				if (!block_occupied(P, ix, iy, iz))
				{
					if (!block_jump<5, 3, 3>(P, start, dir, inv, tmax, ix, iy, iz, t, tx, ty, tz)) return false;
					continue;
				}
				okey = bk;
			}
		}
		bool alive;
		if (P.legacy) alive = P.cells[(size_t)ix + ((size_t)iy + (size_t)iz * G) * G] == 1u; // `== 1` (pathtraced_fragment.wgsl:530)
		else
		{
			const int key = (ix >> 5) + (iy + iz * G) * (int)P.cols;
			if (key != wkey) { word = fetch(P, key); wkey = key; }
			alive = (word >> (ix & 31)) & 1u;
		}
		if (alive)
		{
			if (!(SHADOW && ix == sx0 && iy == sy0 && iz == sz0)) // any(cell != startCell) :664
			{
				float tn, tf;
				ray_cube_inv(start, inv, cell_origin(cs, ix, iy, iz), half, tn, tf);
				if (SHADOW ? (tn <= tf && tn >= 0.0f) /* :668 */ : (tf >= 0.0f && tn <= tf) /* :722-729 */)
				{
					tnear_out = tn;
					return true;
				}
			}
		}
		// advance along the axis whose boundary comes first — selects, not a three-way branch: the lanes of a wave
		// step along different axes almost every time
		const bool mx = tx <= ty && tx <= tz, my = !mx && ty <= tz, mz = !mx && !my;
		t = mx ? tx : (my ? ty : tz);
		tx += mx ? dx : 0.0f;
		ty += my ? dy : 0.0f;
		tz += mz ? dz : 0.0f;
		ix += mx ? sx : 0;
		iy += my ? sy : 0;
		iz += mz ? sz : 0;
		if ((u32)ix >= (u32)G || (u32)iy >= (u32)G || (u32)iz >= (u32)G) return false;
	}
	return false;
}

template <bool SHADOW, bool SKIP>
__device__ bool walk(const RenderParams &P, v3 start, v3 dir, float t0, float tmax, v3 half, int sx0, int sy0, int sz0,
                     float &tnear_out, u32 &visits)
{
	return walk_from<SHADOW, SKIP>(P, start, dir, t0, tmax, half, sx0, sy0, sz0, tnear_out, visits, GlobalWords{});
}

struct Sample
{
	float r, g, b, a, depth;
	u32 shadow_ray;
};

// A tracer that KNOWS its view ray meets no live cell and only wants what such a sample leaves behind (its depth): shade_sample_with
// returns right after the depth (specialised for MissTracer below).
template <class T>
struct TracerKnowsMiss
{
	static constexpr bool value = false;
};

// The two walks of a sample, as the kernel at hand performs them. `Tracer` supplies
//   primary(P, cam, ray, enter, dir, len, vhalf, tnear) -> hit        the view ray's walk over (0, len) from `enter`
//   shadow(P, p, dir, len, vhalf, cx, cy, cz) -> occluded             the shadow ray's walk over (0.0025, len) from p in cell (cx, cy, cz)
//   kSkipBox            view rays that miss the box of the occupied blocks are answered "no hit" without a walk (sparse-volume kernels)
//   kStopAfterPrimary   the caller only wanted the view ray (the ray-stream pipeline's first pass captures it and leaves)
//   kStopAfterShadow    ... or the shadow ray (its second pass)
// WalkTracer walks on the spot (plain kernels); the ray-stream passes capture a ray or look a finished walk's answer up. Every kernel
// goes through this one function, so a sample's arithmetic — and with it the frame — is the same bit for bit whichever form drew it.
template <bool SKIP>
struct WalkTracer
{
	static constexpr bool kSkipBox = SKIP, kStopAfterPrimary = false, kStopAfterShadow = false;
	u32 &pvis, &svis;
	__device__ __forceinline__ bool primary(const RenderParams &P, v3 cam, v3 ray, v3 enter, v3 dir, float len, v3 vhalf, float &tnear)
	{
		return walk<false, SKIP>(P, enter, dir, 0.0f, len, vhalf, 0, 0, 0, tnear, pvis);
	}
	__device__ __forceinline__ bool shadow(const RenderParams &P, v3 p, v3 dir, float len, v3 vhalf, int cx, int cy, int cz)
	{
		float dummy = 0.0f;
		return walk<true, SKIP>(P, p, dir, 0.0025f, len, vhalf, cx, cy, cz, dummy, svis);
	}
};

template <class Tracer>
__device__ __forceinline__ Sample shade_sample_with(const RenderParams &P, float vu, float vv, Tracer &tr)
{
	const float *u = P.u;
	const float *view = u + U_VIEW;
	Sample s{0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0u};
	const v3 cam = V(view[12], view[13], view[14]);
	// getRay :188-197, then viewMat * vec4(ray, 0)
	const float r = u[U_WINDOW] / u[U_WINDOW + 1];
	const v3 rl = norm3(V((vu - 0.5f) * r, vv - 0.5f, -(0.5f * P.cot_half_fov)));
	const v3 ray = V(view[0] * rl.x + view[4] * rl.y + view[8] * rl.z, view[1] * rl.x + view[5] * rl.y + view[9] * rl.z,
	                 view[2] * rl.x + view[6] * rl.y + view[10] * rl.z);
	const v3 half = V(kHalf, kHalf, kHalf);
	float tn, tf;
	ray_cube(cam, ray, V(0.0f, 0.0f, 0.0f), half, tn, tf);
	const float cam_dist = sd_box(cam, half);
	if (tn <= tf && tf >= 0.0f) // :822
	{
		v3 enter = cam;
		const v3 exitp = cam + ray * tf;
		if (cam_dist >= 0.0f) enter = cam + ray * tn;
		const v3 seg = exitp - enter;
		const v3 dir = norm3(seg);
		const float depth_len = len3(seg);
		const float cs = 1.0f / (float)P.G;
		const float vis = cs * u[U_CELLSIZE] * 0.5f;
		const v3 vhalf = V(vis, vis, vis);
		float tnear = 0.0f;
		const bool hit = (Tracer::kSkipBox && misses_live_box(P, cam, ray)) ? false : tr.primary(P, cam, ray, enter, dir, depth_len, vhalf, tnear);
		if (Tracer::kStopAfterPrimary) return s;
		const v3 final_point = hit ? enter + dir * tnear : exitp;
		s.depth = len3(final_point - cam);  // :762, 774
		if (TracerKnowsMiss<Tracer>::value) return s; // colour 0, alpha 1 (the clamp below changes neither)
		const v3 p = cam + ray * s.depth;   // moreAccurateSamplePoint :840
		// calculateLightingAndOcclusionAt :379-427
		const v3 f = V(floorf(to_cells(P, p.x)), floorf(to_cells(P, p.y)), floorf(to_cells(P, p.z)));
		const v3 origin = V(f.x * cs + cs * 0.5f - kHalf, f.y * cs + cs * 0.5f - kHalf, f.z * cs + cs * 0.5f - kHalf);
		const int cx = (int)f.x, cy = (int)f.y, cz = (int)f.z;
		const u32 st = cell_state(P, (u32)cx, (u32)cy, (u32)cz);
		const float dist = sd_box(p - origin, vhalf);
		if (st == 1u && !(dist > 0.001f))
		{
			const v3 light_pos = V(u[U_LIGHT], u[U_LIGHT + 1], u[U_LIGHT + 2]);
			const v3 ldir = norm3(light_pos - p);
			float vn, vf;
			ray_cube(p, ldir, V(0.0f, 0.0f, 0.0f), half, vn, vf);
			const v3 vexit = p + ldir * vf;
			const v3 sseg = vexit - p;
			const v3 sdir = norm3(sseg);
			const float slen = len3(sseg);
			const bool occluded = tr.shadow(P, p, sdir, slen, vhalf, cx, cy, cz);
			if (Tracer::kStopAfterShadow) return s;
			const float occ = occluded ? (P.legacy ? 0.095f : kOcclusion) : 1.0f; // pathtraced_fragment.wgsl:67 / clustered :72
			if (P.legacy)
			{
				// calculateLigtingAt (pathtraced_fragment.wgsl:338-365): mirror-reflection term + flat term, 1/d^2 to light and eye
				const v3 N = face_normal(p, origin);
				const float Gf = (float)P.G;
				const v3 colr = V(f.x / Gf, f.y / Gf, 1.0f - f.x / Gf);
				const v3 view_dir = norm3(p - cam);
				const float dl = len3(light_pos - p), dc = len3(cam - p);
				const float fl = fmaxf(1.0f, powf(dl, 2.0f)), fc = fmaxf(1.0f, powf(dc, 2.0f));
				const float incident = u[U_LIGHT + 3] / fl;
				const v3 inc_dir = norm3(p - light_pos);
				const float ndi = dot3(N, inc_dir);
				const v3 refl = V(inc_dir.x - 2.0f * ndi * N.x, inc_dir.y - 2.0f * ndi * N.y, inc_dir.z - 2.0f * ndi * N.z);
				const float reflected = incident * dot3(refl, V(-view_dir.x, -view_dir.y, -view_dir.z));
				s.r = occ * ((colr.x * reflected + incident * colr.x) / fc);
				s.g = occ * ((colr.y * reflected + incident * colr.y) / fc);
				s.b = occ * ((colr.z * reflected + incident * colr.z) / fc);
				s.a = occ; // the vec4 colour (alpha 1) is scaled as a whole (:226)
				s.shadow_ray = 1u;
			}
			else
			{
			// calculateLightingAt :594-633
			const v3 N = face_normal(p, origin);
			const float Gf = (float)P.G;
			const float cxn = (float)(u32)cx / Gf, cyn = (float)(u32)cy / Gf;
			v3 albedo = V(cxn, cyn, 1.0f - cxn);
			if (u[U_MATERIALCOLOR] != 0.0f || u[U_MATERIALCOLOR + 1] != 0.0f || u[U_MATERIALCOLOR + 2] != 0.0f)
				albedo = V(u[U_MATERIALCOLOR], u[U_MATERIALCOLOR + 1], u[U_MATERIALCOLOR + 2]);
			const v3 Vd = norm3(cam - p);
			const v3 L = norm3(light_pos - p);
			const v3 F0 = V(u[U_REFLECTIVITY], u[U_REFLECTIVITY + 1], u[U_REFLECTIVITY + 2]);
			const v3 brdf = surface_brdf(L, Vd, N, u[U_ROUGHNESS], albedo, F0);
			const float mag = u[U_LIGHT + 3];
			const float LoN = dot3(L, N);
			s.r = occ * fmaxf(0.0f, brdf.x * mag * LoN);
			s.g = occ * fmaxf(0.0f, brdf.y * mag * LoN);
			s.b = occ * fmaxf(0.0f, brdf.z * mag * LoN);
			s.shadow_ray = 1u;
			if (P.indirect)
			{
				// calculateIndirectLighting :307-377 — one bounce off the four neighbour cells of the layer the face looks
				// into (tables :117-169): each live neighbour is hit along the integer offset direction, lit from the light
				// source (own shadow walk), and what it reflects towards p is p's incident light from that point
				int ox[4], oy[4], oz[4];
				if (N.x != 0.0f) { const int sx = N.x < 0.0f ? -1 : 1; ox[0] = ox[1] = ox[2] = ox[3] = sx; oy[0] = 1; oy[1] = -1; oy[2] = oy[3] = 0; oz[0] = oz[1] = 0; oz[2] = 1; oz[3] = -1; }
				else if (N.y != 0.0f) { const int sy = N.y < 0.0f ? -1 : 1; oy[0] = oy[1] = oy[2] = oy[3] = sy; ox[0] = -1; ox[1] = 1; ox[2] = ox[3] = 0; oz[0] = oz[1] = 0; oz[2] = 1; oz[3] = -1; }
				else { const int sz = N.z < 0.0f ? -1 : 1; oz[0] = oz[1] = oz[2] = oz[3] = sz; ox[0] = ox[1] = 0; ox[2] = -1; ox[3] = 1; oy[0] = 1; oy[1] = -1; oy[2] = oy[3] = 0; }
				for (int i = 0; i < 4; i++)
				{
					const u32 nx = (u32)(cx + ox[i]), ny = (u32)(cy + oy[i]), nz = (u32)(cz + oz[i]); // vec3u(vec3i) :345
					if (!cell_state(P, nx, ny, nz)) continue;
					const v3 norigin = V((float)nx * cs + cs * 0.5f - kHalf, (float)ny * cs + cs * 0.5f - kHalf, (float)nz * cs + cs * 0.5f - kHalf);
					const v3 ndir = V((float)ox[i], (float)oy[i], (float)oz[i]);
					float qn, qf;
					ray_cube(p, ndir, norigin, vhalf, qn, qf);
					if (!(qn <= qf && qf >= 0.0f)) continue;
					const v3 np = p + ndir * qn;
					const v3 nl = norm3(light_pos - np);
					float wn, wf;
					ray_cube(np, nl, V(0.0f, 0.0f, 0.0f), half, wn, wf);
					const v3 nseg = (np + nl * wf) - np;
					const bool nocc = tr.shadow(P, np, norm3(nseg), len3(nseg), vhalf, (int)nx, (int)ny, (int)nz);
					const v3 refl = lighting_from(P, np, norigin, nx, ny, p, V(mag, mag, mag), light_pos) * (nocc ? kOcclusion : 1.0f);
					const v3 ind = lighting_from(P, p, origin, (u32)cx, (u32)cy, cam, refl, np);
					s.r += ind.x; s.g += ind.y; s.b += ind.z;
				}
			}
			}
		}
		// fixed point of clamp(mix(prev, cur, alpha), 0, 1) under a static camera :468
		s.r = fminf(fmaxf(s.r, 0.0f), 1.0f);
		s.g = fminf(fmaxf(s.g, 0.0f), 1.0f);
		s.b = fminf(fmaxf(s.b, 0.0f), 1.0f);
		s.a = fminf(fmaxf(s.a, 0.0f), 1.0f);
	}
	{
		// light gizmo :866-874
		const v3 light_pos = V(u[U_LIGHT], u[U_LIGHT + 1], u[U_LIGHT + 2]);
		float ln, lf;
		ray_cube(cam, ray, light_pos, V(0.005f, 0.005f, 0.005f), ln, lf);
		if (ln <= lf && lf >= 0.0f && s.r == 0.0f && s.g == 0.0f && s.b == 0.0f) { s.r = s.g = s.b = 1.0f; s.a = 1.0f; }
	}
	if (u[U_SHOWDEPTH] == 1.0f && vu < 0.5f) { s.r = s.depth; s.g = 0.0f; s.b = 0.0f; s.a = 1.0f; } // :880-883
	return s;
}

struct MissTracer
{
	static constexpr bool kSkipBox = false, kStopAfterPrimary = false, kStopAfterShadow = false;
	__device__ __forceinline__ bool primary(const RenderParams &, v3, v3, v3, v3, float, v3, float &) { return false; }
	__device__ __forceinline__ bool shadow(const RenderParams &, v3, v3, float, v3, int, int, int) { return false; }
};
template <>
struct TracerKnowsMiss<MissTracer>
{
	static constexpr bool value = true;
};

// Screen rectangle of the axis-aligned box [lo, hi] (volume space): its eight corners projected (the inverse of getRay :188-197, in
// double), two pixels of margin, aligned outwards to 16 pixels, clipped to the band [row0, row1). A view ray that meets the box goes
// through a pixel of the rectangle (the projection of a convex body is the hull of its projected corners). A box wholly behind the
// camera's plane gets the empty rectangle. false: the box straddles that plane or a corner lies in it (or the view matrix is
// singular) — no rectangle can be given, the caller takes the whole frame.
struct PixRect
{
	u32 x0, x1, y0, y1; // [x0, x1) x [y0, y1); empty when x1 <= x0
};
__host__ __device__ inline bool box_pix_rect(const float *u, float cot_half_fov, u32 W, u32 H, u32 row0, u32 row1, const double lo[3], const double hi[3], PixRect &r)
{
	const float *v = u + U_VIEW;
	const double m[3][3] = {{v[0], v[4], v[8]}, {v[1], v[5], v[9]}, {v[2], v[6], v[10]}}; // world dir = m * camera dir
	const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
	                   m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
	const double aspect = (double)u[U_WINDOW] / (double)u[U_WINDOW + 1];
	r.x0 = r.x1 = r.y0 = r.y1 = 0u;
	if (!(fabs(det) > 1e-12) || !(aspect > 0.0)) return false;
	double lo_x = 1e30, hi_x = -1e30, lo_y = 1e30, hi_y = -1e30;
	int behind = 0;
	for (int c = 0; c < 8; c++)
	{
		const double d[3] = {(c & 1 ? hi[0] : lo[0]) - v[12], (c & 2 ? hi[1] : lo[1]) - v[13], (c & 4 ? hi[2] : lo[2]) - v[14]};
		// camera-space position: m^-1 * d (Cramer)
		const double q0 = (d[0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (d[1] * m[2][2] - m[1][2] * d[2]) + m[0][2] * (d[1] * m[2][1] - m[1][1] * d[2])) / det;
		const double q1 = (m[0][0] * (d[1] * m[2][2] - m[1][2] * d[2]) - d[0] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * d[2] - d[1] * m[2][0])) / det;
		const double q2 = (m[0][0] * (m[1][1] * d[2] - d[1] * m[2][1]) - m[0][1] * (m[1][0] * d[2] - d[1] * m[2][0]) + d[0] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])) / det;
		if (q2 > 1e-3) { behind++; continue; } // behind the camera's plane (every view ray looks down -z)
		if (!(q2 < -1e-3)) return false;
		const double vu = 0.5 - 0.5 * cot_half_fov * (q0 / q2) / aspect, vv = 0.5 - 0.5 * cot_half_fov * (q1 / q2);
		const double x = vu * W, y = (1.0 - vv) * H;
		lo_x = fmin(lo_x, x); hi_x = fmax(hi_x, x); lo_y = fmin(lo_y, y); hi_y = fmax(hi_y, y);
	}
	if (behind == 8) return true; // the whole box lies behind the camera's plane: no view ray meets it — the empty rectangle
	if (behind) return false;     // it straddles the plane
	const double x0 = fmax(0.0, floor(lo_x) - 2.0), x1 = fmin((double)W, ceil(hi_x) + 2.0);
	const double y0 = fmax((double)row0, floor(lo_y) - 2.0), y1 = fmin((double)row1, ceil(hi_y) + 2.0);
	if (!(x1 > x0) || !(y1 > y0)) return true; // off screen (or outside the band): the empty rectangle
	r.x0 = ((u32)x0 / 16u) * 16u;
	r.x1 = (((u32)x1 + 15u) / 16u) * 16u;
	r.y0 = row0 + (((u32)y0 - row0) / 16u) * 16u;
	r.y1 = row0 + (((u32)y1 - row0 + 15u) / 16u) * 16u;
	return true;
}

// ... of the box of the occupied blocks grown by one cell (misses_live_box's box). false: no rectangle (take the whole frame).
__device__ inline bool live_box_pix_rect(const RenderParams &P, PixRect &r)
{
	r.x0 = r.x1 = r.y0 = r.y1 = 0u;
	if (!P.live_box) return false;
	const u32 x1 = P.live_box[0], x0 = ~P.live_box[1], y1 = P.live_box[2], y0 = ~P.live_box[3], z1 = P.live_box[4], z0 = ~P.live_box[5];
	if (x0 >= x1) return true; // nothing alive: the empty rectangle
	// A view ray that misses every live cell still looks the cell of its EXIT point up (:379-427), and that point lies on the volume's
	// boundary: a coordinate that floors to -1 or G wraps the way the reference's u32 modulo does (cell_state) — to G - 1 and 0 on a
	// power-of-two grid, to (2^27 - 1) % cols words into the row (x) or (2^32 - 1) % G (y, z) on the others: at G = 160 x = -1 reads
	// cell x = 95, in the middle of the grid, and the reference lights a stray pixel if that cell lives. "Outside the live box's
	// rectangle nothing is lit" therefore needs the box to keep clear of every plane such a look-up can land on.
	{
		const u32 G = P.G;
		const u32 xa = ((0x7FFFFFFu % P.cols) << 5) + 31u, ya = 0xFFFFFFFFu % G;
		const u32 sx[3] = {0u, G - 1u, xa}, syz[3] = {0u, G - 1u, ya};
		for (int k = 0; k < 3; k++)
			if ((sx[k] >= x0 && sx[k] < x1) || (syz[k] >= y0 && syz[k] < y1) || (syz[k] >= z0 && syz[k] < z1)) return false;
	}
	const double cs = 1.0 / (double)P.G;
	// (a little wider than misses_live_box's float box: a cell more on every side)
	const double lo[3] = {(double)x0 * cs - 0.5 - 2.0 * cs, (double)y0 * cs - 0.5 - 2.0 * cs, (double)z0 * cs - 0.5 - 2.0 * cs};
	const double hi[3] = {(double)x1 * cs - 0.5 + 2.0 * cs, (double)y1 * cs - 0.5 + 2.0 * cs, (double)z1 * cs - 0.5 + 2.0 * cs};
	return box_pix_rect(P.u, P.cot_half_fov, P.W, P.H, P.row0, P.row1, lo, hi, r);
}
__device__ __forceinline__ bool in_pix_rect(const PixRect &r, u32 x, u32 y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }
// The live box's rectangle is worked out ONCE per frame (ca_live_rect, one lane: eight corners in double precision are ~2 000
// instructions — per thread of every workgroup that was most of a 124 us background pass) and left in words 4-5 of the frame's
// counters; the kernels that test tiles against it read it from there. [0]: 1 a rectangle follows, 2 none can be given (whole frame).
__device__ __forceinline__ bool live_rect_load(const RenderParams &P, PixRect &r)
{
	const u32 *w = reinterpret_cast<const u32 *>(P.counters + 4);
	r.x0 = w[1] & 0xFFFFu; r.x1 = w[1] >> 16; r.y0 = w[2] & 0xFFFFu; r.y1 = w[2] >> 16;
	return w[0] == 1u;
}

template <bool SKIP>
__device__ Sample shade_sample(const RenderParams &P, float vu, float vv, u32 &pvis, u32 &svis)
{
	WalkTracer<SKIP> tr{pvis, svis};
	return shade_sample_with(P, vu, vv, tr);
}

__device__ __forceinline__ u32 unorm8(float x) { return (u32)__float2int_rn(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f); }

// ================================================================================================ literal frame
// One frame exactly as fragment_main (800-890) produces it — jittered fixed-step marches, history look-ups,
// depth repair, temporal blend — for hosts that want the reference's own accumulation behaviour
// (ca3d_set_option("render_mode", 1)). sin() of the jitter hash is evaluated in double precision and rounded to
// f32 (WGSL leaves it implementation-defined); history fetches outside the target or at NaN coordinates read 0.
struct FrameParams
{
	RenderParams base;
	const uint2 *prev_light; // RGBA16F written by the previous frame
	const u32 *prev_depth;   // RG16F
};

__device__ __forceinline__ float fract1(float x) { return x - floorf(x); }

__device__ __attribute__((unused)) float n1rand(const RenderParams &P, float u, float v)
{
	const float t = 0.07f * fract1(P.u[U_TIME]);
	const float d = (t + u) * 12.9898f + (t + v) * 78.233f;
	const float s = (float)sin((double)d);
	return fract1(s * 43758.5453f);
}

__device__ __forceinline__ u32 f2u(float f) { return !(f >= 0.0f) ? 0u : (f >= 4294967296.0f ? 0xFFFFFFFFu : (u32)f); }

__device__ __attribute__((unused)) void reprojected_uv(const RenderParams &P, v3 p, float &ux, float &uy)
{
	const float *m = P.u + U_PREVPROJVIEWINV;
	const float q0 = m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12];
	const float q1 = m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13];
	const float q3 = m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15];
	const float cx = q0 / q3, cy = q1 / q3;
	ux = cx * 0.5f + 0.5f;
	uy = -cy * 0.5f + 0.5f;
}

__device__ __attribute__((unused)) bool texel_xy(const RenderParams &P, float fx, float fy, size_t &idx)
{
	if (!(fx == fx) || !(fy == fy)) return false;
	if (fx <= -1.0f || fy <= -1.0f || fx >= (float)P.W || fy >= (float)P.H) return false;
	const int x = (int)fx, y = (int)fy;
	if (x < 0 || y < 0 || x >= (int)P.W || y >= (int)P.H) return false;
	idx = (size_t)y * P.W + (size_t)x;
	return true;
}

struct CellU
{
	v3 origin;
	u32 x, y, z, idx;
};

__device__ __attribute__((unused)) CellU cell_u(const RenderParams &P, v3 p)
{
	const float cs = 1.0f / (float)P.G;
	const v3 f = V(floorf(to_cells(P, p.x)), floorf(to_cells(P, p.y)), floorf(to_cells(P, p.z)));
	CellU r;
	r.origin = V(f.x * cs + cs * 0.5f - kHalf, f.y * cs + cs * 0.5f - kHalf, f.z * cs + cs * 0.5f - kHalf);
	r.x = f2u(f.x); r.y = f2u(f.y); r.z = f2u(f.z);
	r.idx = r.x + r.y * P.G + r.z * (u32)((float)P.G * (float)P.G);
	return r;
}

