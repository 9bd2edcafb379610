// Internal declarations shared by the C-ABI layer and the HIP kernels. Not installed; the public surface is
// include/ca3d.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "ca3d.h"
#include "ca_device_types.h"

namespace ca3d
{

constexpr int kMaxOffsets = 26; // per list; a count must stay inside its 27-slot LUT slice

struct OffsetLists
{
	uint32_t n[3];
	uint8_t code[3][32]; // (dx+1) | (dy+1) << 2 | (dz+1) << 4
};

struct CanonRules
{
	bool valid = false;
	// packed layout
	MainKind main = MAIN_GENERIC;
	bool need[3] = {false, false, false}; // whether the rule-set's count influences the result at all
	bool fast = false;                    // the three lists are the named class unions -> class kernels
	OffsetLists lists{};
	PackedRuleArgs prog{};
	uint32_t onset_survive[3]{}, onset_born[3]{}; // bit k: LUT slot k of the rule-set == 1
	// unpacked layout: main list + slots 0..26 with `> 0`
	uint32_t unpacked_survive = 0, unpacked_born = 0; // bit k = LUT[k] > 0
	RuleSetProg unpacked_prog{};                        // the same as cube programs over the main list's count
	bool unpacked_fast = false;                         // main list is a named class union (ballot kernel applies)
	// raw copies (returned for diagnostics)
	uint32_t survive_raw[CA3D_LUT_LEN]{}, born_raw[CA3D_LUT_LEN]{};
};

// rules.cpp
int canonicalize_rules(const int32_t *main_offs, uint32_t n_main, const int32_t *edge_offs, uint32_t n_edge,
                       const int32_t *corner_offs, uint32_t n_corner, const uint32_t *survive,
                       const uint32_t *born, CanonRules *out, std::string *err);
// Minimal OR-of-cubes cover of `onset` over `nvars` count planes; counts > max_count are don't-cares.
void compile_rule_prog(uint32_t onset_mask, uint32_t max_count, RuleProg *out);

// ---------------------------------------------------------------------------------------------- launch params

// Run-time compiled (hiprtc) von Neumann kernels for one (grid, survive table, born table): ca_jit.cpp
struct VnJit
{
	void *zr1 = nullptr, *zr2 = nullptr, *zr4 = nullptr, *zr8 = nullptr; // hipFunction_t of the 1-, 2-, 4- and (grids of 2048 and up) 8-planes-per-thread entry points
	int cvl = -1;
	uint32_t lut_s = 0, lut_b = 0;
};

// Run-time compiled rows kernel (ca_packed_rows_kernel.inc) for one (grid, main table, live rule-sets, rule): any multiple of 32
struct RowsJit
{
	void *deep = nullptr, *flat = nullptr; // zrun planes per thread / 1 plane per thread
	uint32_t G = 0;
	int zrun = 0, main = -1;
	bool e = false, c = false;
};

// Run-time compiled class kernels (rule as compile-time truth tables) for one (main table, live rule-sets, rule)
struct ClassJit
{
	void *deep = nullptr, *deep_za = nullptr, *flat = nullptr; // hipFunction_t: ZRUN planes per thread (general /
	                                                           // z-aligned ranges) / 1 plane per thread
	void *deep_np2 = nullptr, *flat_np2 = nullptr;             // the same for rows of whole uint4 that are not a power of two of them
	int main = -1;
	bool e = false, c = false;
};

// Run-time compiled rolling-window class kernels (ca_packed_roll_kernel.inc) for one (grid, main table, live rule-sets,
// rule): entry points with 2, 4 and 8 output planes per thread
struct RollJit
{
	void *z[3] = {nullptr, nullptr, nullptr}; // hipFunction_t for Z = 2, 4, 8
	void *tile[4] = {nullptr, nullptr, nullptr, nullptr}; // the tile form (x-shifted rows shared through LDS) for Z = 2, 4, 8, 16
	void *tile_x = nullptr; int zx = 0; // tuning (CA3D_ROLL_ZX=<planes>): one more depth of the tile form
	void *loop[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; // looped forms [tile][Z = 15, 30]: the plane loop rolled up in groups of three
	void *w2[2] = {nullptr, nullptr};    // two words per thread (five waves per SIMD) for Z = 8, 16; null on rows of 32 uint4 and more
	void *wtile[2] = {nullptr, nullptr}; // wave tiles (one wave per workgroup, LDS exchange without a barrier) for Z = 8, 16; null on rows of 64 uint4
	void *np2[3] = {nullptr, nullptr, nullptr}; // roll_step_np2 for Z = 2, 4, 8: the module of a grid with cv_np2 uint4 per row (not a power of two)
	int cv_np2 = 0;                            // uint4 per row of the np2 module; 0: none
	int cvl = -1;                              // log2(G / 128); -1: none
	int main = -1;
	bool e = false, c = false;
};

struct PackedLaunch
{
	const uint32_t *in;
	uint32_t *out;
	PlaneRange pr;
	const CanonRules *rules;
	int variant; // -1 auto
	const VnJit *vn_jit = nullptr; // specialised kernels for exactly these rules and this grid, or null
	const ClassJit *class_jit = nullptr;
	const RollJit *roll_jit = nullptr;
	int roll_z = 0; // 0: the launcher picks the planes per thread of the rolling-window kernel; 2 / 4 / 8 (tile form: 16 too): forced (tests, tuning)
	int roll_tile = 1; // 1: the tile form of the rolling-window kernel (ca_packed_roll_kernel.inc, tile_step); 0: every thread shifts its three rows itself;
	                   // 2: wave tiles (the tile form with one wave per workgroup: no barrier); 3: two words per thread, no LDS (roll_step_w2)
	const RowsJit *rows_jit = nullptr; // the rows kernel compiled for exactly this grid and these rules, or null
};

// One launch of the resident multi-step kernel (ca_resident.hip): `steps` steps from `in`, state on chip in between
struct ResidentLaunch
{
	const uint32_t *in;
	uint32_t *out_last, *out_prev; // state after `steps` steps / one step earlier (the two ping-pong buffers)
	uint32_t G;
	unsigned long long *mail;      // face mailboxes, resident_mail_bytes(G)
	uint32_t *status;              // device words: [0] != 0 when a wait timed out, [4 + tile] steps finished by that tile
	uint32_t *host_flag;           // pinned host word the kernel sets on a timeout
	uint32_t steps, epoch0, timeout_ticks;
	uint32_t lut_s, lut_b;         // von Neumann truth tables (vn_tables)
	void *jit_fn = nullptr;        // hipFunction_t of the run-time compiled kernel for these tables, or null (pre-built rule)
	uint32_t rows = 32;            // rows per tile: 32 (one 512-thread workgroup per CU) or 16 (two 256-thread workgroups per CU)
	uint32_t fault_tile = 0;       // diagnostics: tile + 1 that leaves at once (a workgroup that never became resident), 0: none
	uint32_t zsplit = 1;           // thread groups along z: 2 = twice the threads per tile, four waves per SIMD (ca_resident_kernel.inc, ZS)
	int pair = 0;                  // 512^3 von Neumann form: a thread owns two adjacent rows x 16 planes; rows = 32, zsplit = 1 (resident_pair_run)
};

struct UnpackedLaunch
{
	const uint32_t *in;
	uint32_t *out;
	PlaneRange pr;
	const CanonRules *rules;
	bool binary_state; // every cell is 0 or 1 (true after any step; checked on upload)
};

struct RenderLaunch
{
	const uint32_t *cells; // packed state, current buffer
	uint32_t G, W, H, spp;
	const float *uniforms; // host pointer, >= 84 floats
	uint32_t *presentation; // device RGBA8 or null
	void *light;            // device RGBA16F or null
	uint32_t *depth;        // device RG16F or null
	unsigned long long *counters; // device, 3 counters, or null
	bool legacy;                  // unpacked volume + legacy shading (shaders/pathtraced_fragment.wgsl)
	int mode;                     // 0 converged frame (exact walk), 1 one literal reference frame with history
	const void *prev_light;       // previous frame's RGBA16F (mode 1)
	const uint32_t *prev_depth;   // previous frame's RG16F (mode 1)
	int sched = 1;                // mode 0: dynamic ray scheduling inside each wave (same frame, bit for bit)
	unsigned long long *occ = nullptr; // mode 0, packed: scratch for the block-occupancy bits + their count,
	                                   // sized by ca3d_render (null: no empty-space skipping)
	uint32_t row0 = 0, row1 = 0;  // mode 0: render image rows [row0, row1) only (row1 == 0: all); row0 % 16 == 0
	bool indirect = false;        // mode 0, packed: add the one-bounce neighbour lighting term (wgsl :307-377)
	bool trace = false;           // diagnostics: per-wave {start, end, HW_ID, visits} after the counters (the buffer must hold them)
	// mode 0, scheduled kernel: a second stream (+ two events) for the plain kernel that renders the tiles AROUND the volume's screen
	// rectangle — it then runs beside the persistent scheduled launch (whose tail leaves CUs idle) instead of after it. Null: one stream.
	hipStream_t aux = nullptr;
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	// mode 0, packed, scheduled: scratch of the ray-stream pipeline (render_stream.hip; stream_scratch_bytes(W, H, spp) bytes) — with it the
	// dense-volume part of the frame is drawn by the stream passes instead of ca_render_packed_sched (same frame, bit for bit). Null: not used.
	uint32_t *bricks = nullptr; // room for the bricked copy of the volume (frame_bricks_bytes(G)); with it (any grid that is a multiple of 32 up to 2048) mode 1's frame is
	                            // drawn by render_frame.hip's batched march instead of ca_render_frame_packed, and mode 0's stream walks read the bricks
	                            // (same frames, bit for bit)
	// The occupancy bits / the bricks in those buffers were built from exactly this state by an earlier frame (the engine tracks what the
	// state is: step count, uploads, buffers handed out): the passes that rebuild them are skipped. A static scene — a camera moving
	// around a paused automaton — pays for them once (512^3: 30 us of a 0.87 ms frame; 2048^3: 2 ms of 3.7).
	bool occ_valid = false, bricks_valid = false;
	// ... and told back: set by the passes that (re)build them in THIS call — the engine takes a buffer for current only then (a frame in
	// the literal mode builds no occupancy bits, a frame whose volume is off screen no bricks: taking either for built would leave the
	// next frame of the same state with stale ones — a converged frame right after literal ones came out black that way)
	bool *occ_built = nullptr, *bricks_built = nullptr;
	void *stream_scratch = nullptr;
	// two frames in flight (ca3d_engine.h, FrameLane): the frame before this one runs on another stream; everything of THIS frame that
	// writes a target both share (the presentation surface) waits for this event first. Null: nothing to wait for.
	hipEvent_t after = nullptr;
	int walk_share_pct = 100; // frames in flight: the share of the chip's wave slots each persistent walk launch of this frame asks for (100: the frame has the chip to itself)
	bool stream_check = false; // diagnostics: every live-cell decision of the interval filter is checked against the slab test and contradictions counted
};

// ca_summary.hip: one pass over the owned planes of the current buffer (and of `prev`, the same planes of the buffer that holds the
// state one step earlier, or null) into a zeroed result block of kSummaryHeaderWords + nz words:
//   u64 [0] population, [1] births, [2] deaths, [3] digest; u32 [8..10] ~box_min x y z (complemented: zero means "none yet"),
//   [11..13] box_max, [14..15] unused, [16 + k] live cells of owned plane k
constexpr uint32_t kSummaryHeaderWords = 16;
struct SummaryLaunch
{
	const uint32_t *cur, *prev; // first OWNED plane of each buffer
	uint32_t *result;
	uint32_t G;
	int layout;
	uint32_t z0, nz; // owned planes [z0, z0 + nz) of the grid
};
hipError_t launch_summary(const SummaryLaunch &l, hipStream_t stream);
// ca_summary.hip: ORs 1 into *flag (a device word the caller has zeroed) when the two arrays of n_words words (a multiple of 4, both
// 16-byte aligned) differ anywhere
hipError_t launch_state_equal(const uint32_t *a, const uint32_t *b, size_t n_words, uint32_t *flag, hipStream_t stream);
// ca_ensemble.hip: one launch over universes [first, first + count) of an ensemble of independent 64^3 grids, one workgroup each;
// every array is indexed by universe (ca3d_ensemble.cpp owns them)
constexpr uint32_t kEnsembleWords = 8192;      // words of one 64^3 universe
constexpr uint32_t kEnsembleMaxSteps = 65536;  // steps of one launch at most: a call that wants more is cut into launches
struct EnsembleLaunch
{
	uint32_t *state, *prev;   // [B][8192] current state / the state one step earlier
	const uint32_t *rules;    // von Neumann: [B] lut_s | lut_b << 8 (7 bits each, vn_tables); Moore: [B][2] born, survive (27 bits each);
	                          // clustered: [B][6] born, survive of the main (27 bits), edges (13) and corners (9) rule-sets
	int neighbourhood;        // CA3D_ENSEMBLE_VON_NEUMANN / CA3D_ENSEMBLE_MOORE: which kernel, and how `rules` reads
	bool clustered;           // Moore only: three table pairs a universe (ca_ensemble_clustered64)
	int boundary;             // CA3D_ENSEMBLE_BOUNDARY_*: what lies behind a universe's faces in this launch's steps (0: the reference's)
	ca3d_summary *records;    // [B] what the last launch left of each universe
	uint32_t *steps_done;     // [B] steps taken in the current step-until call (written when stop_mask != 0)
	uint32_t *reason;         // [B] stop bits that fired in the current call; a universe whose word is set leaves at once
	uint32_t *anchor;         // [B][8192] the state at each universe's anchor check point; [B][4] anchor step, anchor hash, period, unused —
	uint32_t *cycle;          // both only when stop_mask holds CA3D_STOP_PERIODIC (the *_cycle kernels), else unused and may be null.
	                          // stop_mask holds CA3D_STOP_MOVING (the *_moving kernels): both as well, `cycle` then [B][8] — anchor step, anchor
	                          // hash, period, shift (dx, dy, dz as signed bytes), the anchor's population, packed box_min, packed box_max, unused
	uint32_t *samples;        // [B][sample_stride][3] population, births, deaths per check point of the call (the *_trace kernels); null: no trace.
	uint32_t sample_stride;   // Every check point is then reached whatever stop_mask holds, CA3D_STOP_PERIODIC is refused
	uint32_t first, count;
	uint32_t steps;           // <= kEnsembleMaxSteps
	uint32_t base;            // steps the earlier launches of the same call took
	uint32_t check_every, stop_mask; // stop_mask 0: plain stepping, nothing is checked
	bool final;               // the call ends with this launch: the conditions are checked after its last step whatever the count
	bool reset;               // after an upload: records are rebuilt with step 0 and no previous state (steps == 0)
};
hipError_t launch_ensemble(const EnsembleLaunch &l, hipStream_t stream);
// ca_ensemble_boundary.hip: the kernel of a kind (0 von Neumann, 1 Moore, 2 clustered) and form (0 plain, 1 *_cycle, 2 *_trace, 3 *_moving)
// under CA3D_ENSEMBLE_BOUNDARY_TORUS or _CLOSED, for ca_ensemble.hip's kernel_of alone; null for anything else
const void *ensemble_boundary_kernel(int boundary, int kind, int form);
int ensemble_workgroups_per_cu(int neighbourhood, bool clustered = false); // what the runtime says of that kind's kernel (0: it cannot tell)
constexpr uint32_t ensemble_rule_words(int neighbourhood, bool clustered = false) // per universe
{
	return clustered ? 6u : neighbourhood == CA3D_ENSEMBLE_MOORE ? 2u : 1u;
}
// ca_census.hip: the connected components of universes [first, first + count) of an ensemble's state array (ca3d_ensemble_census), one
// workgroup of ca_ensemble_census64 each; out, n_components and remaining are indexed by universe - first. The caller has checked the range.
constexpr uint32_t kCensusMaxComponents = 1024;
struct CensusLaunch
{
	const uint32_t *state; // [B][8192], the ensemble's current states
	uint32_t first, count;
	uint32_t max_components; // 1 .. kCensusMaxComponents
	ca3d_component *out;     // device, [count][max_components]: every slot is written
	uint32_t *n_components, *remaining; // device, [count]
	uint32_t connectivity;   // CA3D_CONNECT_CLOSED: ca_ensemble_census64; CA3D_CONNECT_TORUS: ca_ensemble_census64_torus (ca_objects_torus.hip)
};
hipError_t launch_census(const CensusLaunch &l, hipStream_t stream);       // picks the kernel by l.connectivity
hipError_t launch_census_torus(const CensusLaunch &l, hipStream_t stream); // ca_objects_torus.hip
// ca_isolate.hip: job k makes the connected component of source universe jobs[k].universe that holds jobs[k].cell the only thing in
// destination universe dst_first + k (ca3d_ensemble_isolate), translated as `placement` says, in both buffers; one workgroup of
// ca_ensemble_isolate64 a job. The caller has checked every universe, cell and range, and that no source universe is a destination.
struct IsolateLaunch
{
	const uint32_t *src_state;      // [Bs][8192], the source ensemble's current states
	uint32_t *dst_state, *dst_prev; // [Bd][8192], the destination ensemble's two buffers
	const uint32_t *src_rules;      // [Bs][rule_words] / [Bd][rule_words]: copied universe to universe when rule_words != 0
	uint32_t *dst_rules;
	const ca3d_isolate_job *jobs;   // device, [n_jobs]
	ca3d_isolated *out;             // device, [n_jobs]: every entry is written
	uint32_t dst_first, n_jobs;
	uint32_t placement;             // CA3D_ISOLATE_KEEP / CENTRE / ORIGIN
	uint32_t rule_words;            // 0: rules stay; else ensemble_rule_words() of both ensembles
	uint32_t connectivity;          // CA3D_CONNECT_CLOSED: ca_ensemble_isolate64; CA3D_CONNECT_TORUS: ca_ensemble_isolate64_torus (ca_objects_torus.hip)
};
hipError_t launch_isolate(const IsolateLaunch &l, hipStream_t stream);       // picks the kernel by l.connectivity
hipError_t launch_isolate_torus(const IsolateLaunch &l, hipStream_t stream); // ca_objects_torus.hip
// ca_compose.hip: destination universe dst_first + k becomes the union of parts part_begin[k] .. part_begin[k + 1] - 1, each the whole
// state of a source universe turned and shifted (ca3d_ensemble_compose), in both buffers; one workgroup of ca_ensemble_compose64 a
// destination. The caller has checked every universe, orientation, `at` and range, and that no source universe is a destination.
struct ComposeLaunch
{
	const uint32_t *src_state;      // [Bs][8192], the source ensemble's current states
	uint32_t *dst_state, *dst_prev; // [Bd][8192], the destination ensemble's two buffers
	const uint32_t *src_rules;      // [Bs][rule_words] / [Bd][rule_words]: a destination with parts takes its first part's when rule_words != 0
	uint32_t *dst_rules;
	const ca3d_compose_part *parts; // device, [part_begin[n_dst]]
	const uint32_t *part_begin;     // device, [n_dst + 1]
	ca3d_composed *out;             // device, [n_dst]: every entry is written
	uint32_t dst_first, n_dst;
	bool over;                      // start from the destination's current state
	uint32_t rule_words;            // 0: rules stay; else ensemble_rule_words() of both ensembles
};
hipError_t launch_compose(const ComposeLaunch &l, hipStream_t stream);
// ca_window.hip: 64^3 windows of a packed full grid of G cells a side (a torus, G a multiple of 32 from 64 up), one per entry of
// `windows`, against the universes those entries name (ca3d_cut_windows / ca3d_stamp_windows). kWindowCut writes both ensemble buffers
// from the grid and never the grid; the other three read `state` and edit the grid with atomics, so windows may overlap. The caller has
// checked every universe and origin, n (1 .. kWindowsMax) and, for a cut, that the universes are distinct.
constexpr uint32_t kWindowsMax = 1u << 20;
enum WindowOp { kWindowCut, kWindowOr, kWindowErase, kWindowClear };
struct WindowLaunch
{
	uint32_t *grid;             // [G][G][G / 32], the engine's current buffer
	uint32_t G;
	uint32_t *state, *prev;     // [B][8192], the ensemble's two buffers (`prev`: a cut only)
	const ca3d_window *windows; // device, [n]
	uint32_t n;
	WindowOp op;                // kWindowClear: every cell of every window's box is cleared (the first phase of CA3D_STAMP_REPLACE)
};
hipError_t launch_windows(const WindowLaunch &l, hipStream_t stream);
// ca_canon.hip: the key, orientation and symmetry group of universes [first, first + count) of an ensemble's state array
// (ca3d_ensemble_canon), one workgroup of ca_ensemble_canon64 each; out and digests are indexed by universe - first. The caller has
// checked the range. The states are only read.
struct CanonLaunch
{
	const uint32_t *state; // [B][8192], the ensemble's current states
	uint32_t first, count;
	ca3d_canon *out;       // device, [count]: every entry is written
	uint64_t *digests;     // device, [count][48], or null: the digest of every orientation
};
hipError_t launch_canon(const CanonLaunch &l, hipStream_t stream);
// ca_canon_period.hip: canon over periods[k] steps of universe first + k, for universes [first, first + count) of an ensemble's state
// and rule arrays (ca3d_ensemble_canon_period), one workgroup each of ca_ensemble_canon_period_vn64, _moore64 or _clustered64 by the
// ensemble's kind; out, keys and periods are indexed by universe - first. The caller has checked the range, every period (1 ..
// CA3D_CANON_MAX_PERIOD) and keys_stride >= max(periods). States and rules are only read.
struct CanonPeriodLaunch
{
	const uint32_t *state;   // [B][8192], the ensemble's current states
	const uint32_t *rules;   // [B][ensemble_rule_words()]
	int neighbourhood;       // CA3D_ENSEMBLE_*
	bool clustered;
	uint32_t first, count;
	const uint32_t *periods; // device, [count]
	ca3d_canon_period *out;  // device, [count]: every entry is written
	uint64_t *keys;          // device, [count][keys_stride], or null: every slot is written, those past the period with zero
	uint32_t keys_stride;
};
hipError_t launch_canon_period(const CanonPeriodLaunch &l, hipStream_t stream);
// ca_envelope.hip: envelope, stator, rotor and heat over periods[k] steps of universe first + k, for universes [first, first + count) of
// a source ensemble's state and rule arrays (ca3d_ensemble_envelope), one workgroup each of ca_ensemble_envelope_{vn,moore,clustered}64
// [_torus|_closed] by the source's kind and boundary; out and periods are indexed by universe - first. With n = popcount(images) != 0,
// source k writes its images in bit order into both buffers of destination universes dst_first + k n + i. The caller has checked every
// range and period, and that no source universe is a destination. The source's states and rules are only read.
struct EnvelopeLaunch
{
	const uint32_t *state;          // [Bs][8192], the source ensemble's current states
	const uint32_t *rules;          // [Bs][ensemble_rule_words()]
	int neighbourhood;              // CA3D_ENSEMBLE_*, of the source
	bool clustered;
	int boundary;                   // CA3D_ENSEMBLE_BOUNDARY_*, of the source
	uint32_t first, count;
	const uint32_t *periods;        // device, [count]
	ca3d_envelope *out;             // device, [count]: every entry is written
	uint32_t images;                // CA3D_ENVELOPE_IMAGE_* bits; 0: nothing below is used
	uint32_t *dst_state, *dst_prev; // [Bd][8192], the destination ensemble's two buffers
	uint32_t *dst_rules;            // [Bd][rule_words]
	uint32_t dst_first;
	uint32_t rule_words;            // 0: rules stay; else ensemble_rule_words() of both ensembles
};
hipError_t launch_envelope(const EnvelopeLaunch &l, hipStream_t stream);
// ca_damage.hip: the Hamming distance between universe first + k and a perturbed twin over steps[k] steps, for universes [first, first +
// count) of a source ensemble's state and rule arrays (ca3d_ensemble_damage), one workgroup each of ca_ensemble_damage_{vn,moore,
// clustered}64[_torus|_closed] by the source's kind and boundary; out, steps, twins, flips and curve are indexed by universe - first.
// With the image, source k writes D_P into both buffers of destination universe dst_first + k. The caller has checked every range, step
// count, twin and flip, that curve_stride > max(steps) when there is a curve, and that no source or twin universe is a destination. The
// source's states and rules are only read.
struct DamageLaunch
{
	const uint32_t *state;          // [Bs][8192], the source ensemble's current states
	const uint32_t *rules;          // [Bs][ensemble_rule_words()]
	int neighbourhood;              // CA3D_ENSEMBLE_*, of the source
	bool clustered;
	int boundary;                   // CA3D_ENSEMBLE_BOUNDARY_*, of the source
	uint32_t first, count;
	const uint32_t *steps;          // device, [count]
	const uint32_t *twins;          // device, [count]: a universe of the source, or CA3D_DAMAGE_SELF
	const uint32_t *flips;          // device, [count][CA3D_DAMAGE_FLIPS]: x | y << 8 | z << 16, or CA3D_DAMAGE_NO_FLIP
	ca3d_damage *out;               // device, [count]: every entry is written
	uint32_t *curve;                // device, [count][curve_stride]: every word is written; or NULL
	uint32_t curve_stride;
	uint32_t image;                 // 0 or CA3D_DAMAGE_IMAGE_DAMAGE; 0: nothing below is used
	uint32_t *dst_state, *dst_prev; // [Bd][8192], the destination ensemble's two buffers
	uint32_t *dst_rules;            // [Bd][rule_words]
	uint32_t dst_first;
	uint32_t rule_words;            // 0: rules stay; else ensemble_rule_words() of both ensembles
};
hipError_t launch_damage(const DamageLaunch &l, hipStream_t stream);
// ca_usage.hip: the histograms of the neighbour counts that steps[k] steps of universe first + k look up in its rule tables, split by
// dead and alive, for universes [first, first + count) of an ensemble's state and rule arrays (ca3d_ensemble_usage), one workgroup each
// of ca_ensemble_usage_{vn,moore,clustered}64[_torus|_closed] by the ensemble's kind and boundary; out and steps are indexed by
// universe - first. The caller has checked the range and every step count. States and rules are only read.
struct UsageLaunch
{
	const uint32_t *state; // [B][8192], the ensemble's current states
	const uint32_t *rules; // [B][ensemble_rule_words()]
	int neighbourhood;
	bool clustered;
	int boundary;          // CA3D_ENSEMBLE_BOUNDARY_*
	uint32_t first, count;
	const uint32_t *steps; // device, [count]
	ca3d_usage *out;       // device, [count]: every word is written
};
hipError_t launch_usage(const UsageLaunch &l, hipStream_t stream);
// render_sheet.hip: universes [first, first + count) of an ensemble's state array drawn as tiles of one sheet, columns x
// ceil(count / columns) tiles of tile_w x tile_h pixels (multiples of 16), row-major, in one launch of ca_render_sheet64; the tile
// slots past `count` are zeroed in front of it. The caller has checked every size.
struct SheetLaunch
{
	const uint32_t *state;  // [B][8192], the ensemble's current states
	uint32_t first, count;
	uint32_t tile_w, tile_h, columns, spp;
	const float *uniforms;  // host pointer, >= 84 floats; windowSize as given
	uint32_t *presentation; // device RGBA8 sheet or null
	void *light;            // device RGBA16F sheet or null
	uint32_t *depth;        // device RG16F sheet or null
	unsigned long long *counters; // device, 3 counters (zeroed by the caller), or null
};
hipError_t launch_render_sheet(const SheetLaunch &l, hipStream_t stream);
// workgroups a universe's 16 x 16-pixel blocks are dealt to, for `count` universes of `blocks` blocks each on a chip with room for `slots` workgroups
uint32_t sheet_shares(uint32_t count, uint32_t blocks, uint32_t slots);
// ca_seed.hip: the counter-based fill of ca3d_seed (include/ca3d.h) written where the state lives. One launch covers the whole arrays of
// both ping-pong buffers: array plane a is global plane z0 - ghost + a; the `ghost` planes below and above the owned ones are zeroed.
struct SeedLaunch
{
	uint32_t *buf0, *buf1; // the two ping-pong arrays (ghosts included), nz + 2 * ghost planes each
	uint32_t G;
	int layout;
	uint32_t z0, nz, ghost; // owned planes [z0, z0 + nz) of the grid (full grid: 0, G, 0)
	ca3d_seed spec;         // validated by the caller (seed_spec_error)
};
hipError_t launch_seed(const SeedLaunch &l, hipStream_t stream);
// universes [first, first + count) of an ensemble: universe first + k takes specs[k] (a DEVICE array) or, when specs is null, `one`
hipError_t launch_seed_ensemble(uint32_t *state, uint32_t *prev, uint32_t first, uint32_t count, const ca3d_seed *specs, const ca3d_seed &one, hipStream_t stream);
// why a spec is refused for a grid of G cells an edge, or null (ca3d_api.cpp; one decision for engines, groups and ensembles)
const char *seed_spec_error(const ca3d_seed &s, uint32_t G);
// ca_diag.hip: float4 device-to-device copy (measurement only)
hipError_t launch_copy_f4(const void *in, void *out, size_t bytes, hipStream_t stream);
// ca_diag.hip: do two (idle) streams run side by side, i.e. sit on different hardware queues? (probe: ~2 ms)
hipError_t streams_concurrent(hipStream_t a, hipStream_t b, bool *out);
// render.hip
hipError_t launch_render(const RenderLaunch &l, hipStream_t stream);
// render_stream.hip: bytes of scratch a frame of this size needs at most (and where its three arrays start); the passes themselves
// (`params`: render.hip's launch parameters with the volume's screen rectangle filled in)
size_t stream_scratch_bytes(uint32_t W, uint32_t H, uint32_t spp, size_t *hit_off, size_t *occl_off, size_t *rays_off);
// render_frame.hip: the literal frame over a bricked copy of the volume (`frame_params`: render.hip's FrameParams)
size_t frame_bricks_bytes(uint32_t G);
bool frame_bricks_applies(uint32_t G);
hipError_t launch_render_frame_bricks(const void *frame_params, uint32_t *bricks, bool bricks_valid, hipStream_t stream, bool *bricks_built = nullptr);
hipError_t launch_brick_volume(const uint32_t *cells, uint32_t *bricks, uint32_t G, hipStream_t stream);
hipError_t launch_render_stream(const void *params, void *scratch, uint32_t W, uint32_t H, bool check, uint32_t *bricks, bool bricks_valid, hipStream_t stream, bool *bricks_built = nullptr, hipEvent_t before_resolve = nullptr, int walk_share_pct = 100,
                                bool *sparse_too = nullptr); // *sparse_too: the passes launched draw scattered sparse volumes as well (render.hip then leaves its scheduled kernel out)

// ca_packed.hip / ca_unpacked.hip
hipError_t launch_packed_step(const PackedLaunch &l, hipStream_t stream);
const char *packed_kernel_name(const CanonRules &r, uint32_t G, int variant);
// ca_packed_vn.hip: the specialised von Neumann kernel (truth-table rules, power-of-two grids)
bool vn_rule_applies(const CanonRules &r, int variant); // main list von Neumann, edges / corners rule-sets without effect
bool side_tables_silent(const CanonRules &r);           // class main list, edges / corners tables that cannot fire: the rule IS its main table pair
bool vn_kernel_applies(const CanonRules &r, uint32_t G, int variant);
hipError_t launch_packed_vn(const PackedLaunch &l, hipStream_t stream);
// Canonical truth tables of the von Neumann kernel for these rules (entry 7 is a don't-care: see ca_packed_vn.hip)
void vn_tables(const CanonRules &r, uint32_t *lut_s, uint32_t *lut_b);
// Whether ca_packed_vn.hip carries an ahead-of-time specialisation for these tables (then no JIT is needed)
bool vn_tables_prebuilt(uint32_t lut_s, uint32_t lut_b);
int vn_grid_log2(uint32_t G); // log2(G / 128)
// ca_jit.cpp: compile (or fetch from the cache) the kernels specialised for (grid 128 << cvl, tables)
uint64_t jit_sources_hash(); // of every device source the run-time compiler is given
int jit_vn_kernels(int device, int cvl, uint32_t lut_s, uint32_t lut_b, VnJit *out, std::string *log);
// Truth tables of the three rule-sets over their count planes, unreachable counts filled (class kernels, JIT)
void class_tables(const CanonRules &r, uint32_t tables[6]);
int class_zrun(const CanonRules &r); // planes per thread of the deep variant for these rules
bool use_class_kernel(const CanonRules &r, uint32_t G, int variant);
int jit_class_kernels(int device, const CanonRules &r, ClassJit *out, std::string *log);
int jit_rows_kernels(int device, const CanonRules &r, uint32_t G, RowsJit *out, std::string *log);
// Whether the rows kernel is the one to use for these rules on this grid: named classes, and no uint4 kernel with the rule compiled in
bool rows_kernel_applies(const CanonRules &r, uint32_t G, int variant);
int jit_roll_kernels(int device, const CanonRules &r, int cvl, RollJit *out, std::string *log);
// ... for a grid of `cv` uint4 per row, cv not a power of two (384, 640, 768, 896): out->np2, out->cv_np2
int jit_roll_np2_kernels(int device, const CanonRules &r, int cv, RollJit *out, std::string *log);
bool roll_np2_applies(const CanonRules &r, uint32_t G, int variant);
// Whether the rolling-window kernel is the one to use for these rules on this grid (diagonal neighbour classes in
// play, power-of-two grid of 256 and up)
bool roll_kernel_applies(const CanonRules &r, uint32_t G, int variant);
// rule_synth.cpp: device source of jit_rule_word() for these rules ("" when the self-check fails), ca_jit.cpp's wrapper
std::string synthesize_rule_source(const CanonRules &r, int *ops_out);
std::string rule_function_source(const CanonRules &r);
// ca_resident.hip
bool resident_kernel_applies(const CanonRules &r, uint32_t G, int variant);
size_t resident_mail_bytes(uint32_t G, uint32_t rows);
hipError_t launch_resident(const ResidentLaunch &l, hipStream_t stream);
// Workgroups a resident launch of this shape needs (`tiles`) and how many of them the device can hold at once on `stream`
// (occupancy of the kernel per CU x the CUs the stream may use): the launch only completes when capacity >= tiles.
// Returns false when the runtime cannot tell (the caller then relies on the kernel's bounded waits alone).
bool resident_capacity(uint32_t G, uint32_t rows, uint32_t zsplit, int pair, void *jit_fn, hipStream_t stream, uint32_t *tiles, uint32_t *capacity);
bool resident_slab_capacity(void *fn, hipStream_t stream, uint32_t *tiles, uint32_t *capacity);
int jit_resident_kernel(int device, uint32_t lut_s, uint32_t lut_b, uint32_t rows, uint32_t zsplit, int pair, void **fn, std::string *log);
// the resident kernel for rules with diagonal neighbour classes (ca_resident_class_kernel.inc; 512^3 and 256^3, run-time compiled)
bool resident_class_applies(const CanonRules &r, uint32_t G, int variant);
int jit_resident_class_kernel(int device, const CanonRules &r, uint32_t G, uint32_t zsplit, void **fn, std::string *log); // G: 512 (zsplit 1) or 256 (2 | 1)
uint32_t resident_class_zsplit(uint32_t G); // z groups of the class form's tiles
// Slab form (one rank's share of a 1024^3 grid, K sub-steps per launch): run-time compiled only, per planes-per-tile count
struct ResidentSlabLaunch
{
	const uint32_t *in;
	uint32_t *out;
	unsigned long long *mail; // resident_slab_mail_bytes()
	uint32_t *status, *host_flag;
	uint32_t steps, epoch0, timeout_ticks;
	int dead_plane; // array plane whose global z is 0, or -1
	void *fn;       // hipFunction_t from jit_resident_slab_kernel
};
// planes per tile of the slab form for an array of `nplanes` planes of a G-wide grid with these rules, or 0 when it does not apply
int resident_slab_planes(const CanonRules &r, uint32_t G, uint32_t nplanes, int variant);
size_t resident_slab_mail_bytes();
hipError_t launch_resident_slab(const ResidentSlabLaunch &l, hipStream_t stream);
void resident_stream_retired(hipStream_t stream); // call after waiting for a stream the engine stops using
int jit_resident_slab_kernel(int device, uint32_t lut_s, uint32_t lut_b, int pz, void **fn, std::string *log);
// Steps one fused launch advances for these rules / grid (0 = no fused kernel applies).
int packed_fused_steps(const CanonRules &r, uint32_t G, int variant);
hipError_t launch_packed_fused(const PackedLaunch &l, hipStream_t stream);
hipError_t launch_unpacked_step(const UnpackedLaunch &l, hipStream_t stream, const char **kernel_name);


// No C++ exception leaves an extern "C" entry point: each one is `int ca3d_x(...) CA3D_API_TRY { ... } CA3D_API_CATCH` — a
// function-try-block whose handler maps what was thrown to a status code and a ca3d_last_error() message (ca3d_api.cpp;
// tests/test_capi_cpu.py checks that every function include/ca3d.h declares is defined this way, and runs the handler on the CPU
// through ca3d_selftest_exception)
int exception_to_status() noexcept;
void jit_stats(ca3d_jit_stats *out); // ca_jit.cpp
#define CA3D_API_TRY try
#define CA3D_API_CATCH                          \
	catch (...)                                 \
	{                                           \
		return ca3d::exception_to_status();     \
	}

} // namespace ca3d
