// The engine object behind include/ca3d.h and what the files of the C-ABI layer share: ca3d_api.cpp (lifecycle, state, getters,
// options), ca3d_step.cpp (kernel selection, the step path), ca3d_slab.cpp (slab phases, RCCL transport), ca3d_render.cpp (renderer
// front end, frames in flight), ca3d_group.cpp. Not installed; the kernel-launch interface is ca3d_internal.h.
#pragma once

#include <map>
#include <string>
#include <vector>

#include "ca3d_internal.h"

struct ca3d_engine
{
	int device = 0;
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr; // active (own or caller's)
	hipEvent_t ev_start = nullptr, ev_stop = nullptr;
	bool ev_valid = false;

	bool configured = false;
	uint32_t G = 0;
	int layout = CA3D_LAYOUT_PACKED32;
	bool slab = false;
	uint32_t z0 = 0, nz = 0, ghost = 0;
	uint32_t nplanes = 0;   // planes per buffer including ghosts
	size_t plane_words = 0; // u32 per z-plane
	uint32_t *buf[2] = {nullptr, nullptr};
	bool has_state = false;
	bool binary_state = false; // unpacked layout: every cell is 0 or 1 (checked on upload, true after any step)
	uint64_t step = 0;
	uint32_t cur = 0; // physical buffer holding the current state (== step % 2 whenever control returns to the caller)

	ca3d::CanonRules rules;
	int variant = 0;
	int use_graph = 1;
	int render_mode = 0;
	int render_indirect = 0; // add calculateIndirectLighting (pathtraced_fragment_clustered.wgsl:307-377; commented out at the reference's call site)
	int render_sched = 1; // dynamic ray scheduling in the converged-frame renderer (render.hip); 0: one pixel per lane, in order
	uint32_t render_row0 = 0, render_row1 = 0; // rows [row0, row1) of the frame are rendered (0, 0: all): a rank's band
	int use_fused = 0; // the two-step fused kernel is bit-exact but measured slower than two single steps

	// captured batches of full-grid steps, keyed by (steps in the batch, buffer it starts from); invalidated on any
	// change of rules, kernels, stream or buffers
	struct StepGraph { hipGraphExec_t exec = nullptr; uint32_t launches = 0; };
	std::map<uint64_t, StepGraph> step_graphs;
	// Shorter batches are launched kernel by kernel: measured at 512^3 (tools/step_gap.py) back-to-back 20-step batches
	// run 6.48 us per step as graphs and 6.13 launched one by one, 64-step batches 5.96 / 5.85, 256-step batches 5.78 / 5.76
	// — a graph launch has a start-up and a completion cost of its own, worth paying once the host would fall behind.
	uint32_t graph_min = 128;
	int want_stats = 1; // record the event pair ca3d_get_stats reads (a marker packet each: costs ~1 us of GPU idle per call)
	std::map<uint64_t, hipGraphExec_t> slab_graphs; // (phase, start buffer, sub-steps) -> captured slab batch
	uint32_t pending_edges = 0;                     // sub-steps of an edge phase awaiting its interior phase
	bool pending_binary = true;                     // binary_state of the buffer that edge phase started from: its interior phase reads it again
	bool pending_resident = false;                  // that edge phase ran the whole batch (a slab too thin to split) as ONE resident launch
	int roll_z = 0;       // forced planes per thread of the rolling-window kernel (0: automatic)
	int roll_tile = 1;    // tile form of the rolling-window kernel (x-shifted rows shared through LDS)
	int use_roll = 1;     // rolling-window form of the class kernels where it applies (needs use_jit)
	int use_jit = 1;      // specialise kernels for the rule at run time (hiprtc) where a specialisation exists
	ca3d::VnJit vn_jit;    // valid when vn_jit.cvl >= 0
	ca3d::ClassJit class_jit;   // valid when class_jit.main >= 0
	ca3d::RowsJit rows_jit;    // valid when rows_jit.main >= 0: the rows kernel for this grid and these rules
	int use_rows = 1;     // option "rows"
	ca3d::RollJit roll_jit;    // valid when roll_jit.cvl >= 0
	std::string jit_log;  // why the last specialisation attempt failed (empty: none failed)

	// resident multi-step kernel (ca_resident.hip): face mailboxes, status word (device + pinned host copy), tag counter
	int use_resident = 1;
	bool res_ready = false;       // the current rules / grid have a resident kernel
	bool res_class = false;       // ... and it is the class form (ca_resident_class_kernel.inc)
	bool res_failed = false;      // a launch timed out: the path stays off until the next configure
	bool res_check = false;       // a resident launch has been issued since the status was last looked at
	void *res_jit_fn = nullptr;   // run-time compiled kernel for the current tables (null: the pre-built rule)
	void *res_slab_fn = nullptr;  // slab form for the current slab geometry and tables (run-time compiled), or null
	size_t res_mail_bytes = 0;
	unsigned long long *res_mail = nullptr;
	uint32_t *res_status = nullptr, *res_status_host = nullptr;
	uint32_t res_epoch = 0;
	uint32_t res_min = 8;                 // shorter batches take the per-step kernels
	uint32_t queue_max = 0;               // > 0: ca3d_step calls are encoded and submitted together (option "queue")
	uint32_t queued = 0;                  // steps encoded, not yet submitted
	uint64_t launches_total = 0;          // kernel launches the step calls issued since ca3d_create
	bool res_pair = true;                 // 512^3 von Neumann form: the row-pair kernel (option "resident_pair"; 2.48 against 2.52 us per step)
	uint32_t res_rows = 32;               // rows per tile of the von Neumann form (ca_resident_kernel.inc: 32 or 16)
	uint32_t res_zsplit = 1;              // thread groups along z of the von Neumann form (option "resident_zsplit"; 2 = twice the threads, four waves per
	                                      // SIMD: measured SLOWER with 32-row tiles — 2.61 vs 2.52 us per step at 512^3, 1.37 vs 1.26 at 256^3 — and faster
	                                      // only with 16-row tiles, 2.89 vs 3.31: profiles/r3_l_resident_zsplit.txt)
	uint32_t res_timeout_ticks = 20000000; // 200 ms of s_memrealtime per wait
	// Recovery of a resident launch that gave up (full-grid engines). A launch of n >= 2 steps never writes the buffer it reads:
	// the final state goes to a third buffer (`spare`), the state one step earlier to the other ping-pong buffer, and the three
	// pointers rotate, so that buf[step % 2] / buf[(step + 1) % 2] keep the reference's meaning. Launches whose completion the
	// host has not looked at yet are remembered; when one of them timed out (it, and every launch queued behind it, wrote
	// nothing: ca_resident_kernel.inc res_must_skip) the engine goes back to that launch's input and runs all their steps
	// through the per-step kernels.
	uint32_t *spare = nullptr;
	struct ResPending { uint32_t epoch0, n, cur_before; uint64_t step_before; uint32_t *in, *other, *spare; };
	std::vector<ResPending> res_pending;
	uint32_t res_fault_tile = 0;          // option "resident_fault_tile": applies to the next resident launch only
	uint32_t res_recovered = 0;           // launches recovered from since ca3d_create
	std::string res_note;                 // why the resident path is off although the rules / grid have a resident kernel

	// halo transport inside the engine (RCCL, loaded on first use): communicator over the ranks of the slab chain, a second
	// stream so that an exchange can run under the interior phase, the events that order the two
	void *comm = nullptr; // ncclComm_t
	int comm_rank = 0, comm_world = 0;
	hipStream_t comm_stream = nullptr;
	hipEvent_t ev_edges = nullptr, ev_comm = nullptr, ev_gather = nullptr;
	bool ghosts_valid = false; // the ghost planes hold the neighbours' planes of the current step

	ca3d_stats stats{};
	const char *unpacked_kernel = ""; // the kernel the unpacked launcher used last (ca_unpacked.hip); the packed layout's name is derived: reported_kernel_name

	// ca3d_summarize: result block on the device (ca_summary.hip), its pinned host copy, the event pair around clear + kernel
	uint32_t *sum_dev = nullptr, *sum_host = nullptr;
	size_t sum_words = 0;
	hipEvent_t sum_ev0 = nullptr, sum_ev1 = nullptr;
	bool sum_ev_valid = false;
	// ca3d_step_until_cycle: the anchor, a device copy of the state at an earlier check point of the call (state_words() words, allocated
	// at the first call, freed with the buffers)
	uint32_t *cycle_anchor = nullptr;
	// the owned planes of buffer [(step + 1) % 2] hold the state one step earlier: set by the step paths that guarantee it, cleared by
	// everything that writes a buffer any other way (upload, buffers handed out, gathers, the resident slab launch)
	bool prev_ok = false;

	// renderer targets: presentation + two history pairs (light RGBA16F, depth RG16F), swapped per frame
	uint32_t rw = 0, rh = 0;
	uint32_t *r_present = nullptr;
	void *r_light[2] = {nullptr, nullptr};
	uint32_t *r_depth[2] = {nullptr, nullptr};
	unsigned long long *r_counters = nullptr;
	size_t r_counter_words = 0;
	unsigned long long *r_occ = nullptr; // block-occupancy bits of the current state + count, rebuilt per frame (render.hip)
	size_t r_occ_words = 0;
	int render_skip = 1; // empty-space skipping on sparse volumes
	int render_stream = 1; // dense packed volumes: the ray-stream passes (render_stream.hip) instead of the in-wave scheduled kernel
	int render_stream_check = 0; // diagnostics: count filter / slab-test contradictions (ca3d_get_render_stats is unchanged; see "render_stream_contradictions")
	int render_frame_bricks = 1; // literal frame mode: the batched march over a bricked copy of the volume (render_frame.hip); 0: ca_render_frame_packed
	uint32_t *r_bricks = nullptr;
	size_t r_bricks_bytes = 0;
	// what the renderer's derived buffers (occupancy bits, bricks) were last built from: serial (bumped by everything that writes the state
	// other than a step: uploads, buffers handed out, gathers), step count, buffer
	uint64_t state_serial = 1, r_occ_key[3] = {0, 0, 0}, r_bricks_key[3] = {0, 0, 0};
	// ca3d_device_buffer handed a pointer out: until the call that ends its validity (step / upload / configure) the caller may write the
	// state at any time without telling the engine, so no frame may reuse what an earlier frame derived from it
	bool buffers_exposed = false;
	void *r_stream = nullptr;    // scratch of the stream passes
	size_t r_stream_bytes = 0;
	int r_swap = 0;
	hipEvent_t rev_start = nullptr, rev_stop = nullptr;
	hipStream_t r_aux = nullptr;             // renderer: the plain kernel around the volume's screen rectangle runs here, beside the scheduled launch
	hipEvent_t r_fork = nullptr, r_join = nullptr;
	bool rev_valid = false;
	ca3d_render_stats rstats{};
	// Converged frames in flight (option "render_pipeline", default 1: four of them up to 24 M samples a frame, three above). A frame's two persistent walk launches each end in a tail with
	// most of the chip idle (render_stream.hip: a third to a half of a 1080p launch) and its passes depend on each other — but not on
	// the frame before: a converged frame has no history. Frames that stay on the device (no host pointers) and are drawn by the stream
	// passes alternate between LANES — a stream, scratch, counters and events each — so that the next frames' walks
	// fill the tails of this one's. A lane waits for the engine's stream at the moment of the call (steps, uploads before the frame);
	// the engine's stream waits for the lanes LAZILY: the next call that touches the state, a target or the stream joins them
	// (bind_device). The presentation surface is shared: a frame's pixel-writing kernels wait for the frame before (RenderLaunch::after).
	// Only on the engine's own stream: a caller who set a stream of their own expects every frame ordered on it.
	static constexpr int kMaxLanes = 4;
	struct FrameLane
	{
		hipStream_t s = nullptr;
		hipEvent_t start = nullptr, stop = nullptr, done = nullptr;
		bool need_state = true; // the engine's stream has had work since this lane's last frame: wait for ev_state first
		void *scratch = nullptr;
		size_t scratch_bytes = 0;
		unsigned long long *counters = nullptr;
		bool pending = false; // frames on this lane the engine's stream has not been made to wait for
		bool used = false;    // `done` has been recorded at least once
	} lanes[kMaxLanes];
	int n_lanes = 0; // lanes created (streams on pairwise different hardware queues); 0: not tried yet
	hipEvent_t ev_state = nullptr; // "everything the engine's stream held when the frame was asked for"
	bool main_touched = true;      // an entry point other than a pipelined ca3d_render has run since ev_state was recorded (bind_device)
	bool state_touched = true;     // an entry point other than ca3d_render has run since the last frame: the next frame is not pipelined (ca3d_render)
	std::vector<hipStream_t> lane_spares; // streams that turned out to share a hardware queue with lane 0 (kept: destroying one hands its queue to the next)
	int render_pipeline = 1; // 0: off; 1: the default depth (render_default_lanes: by frame size); 2 .. kMaxLanes: that many
	int lane_next = 0;
	int lanes_in_use = 0; // depth of the last pipelined frame (ca3d_get_render_pipeline)
	bool lanes_exhausted = false; // the probe found fewer side-by-side streams than asked for
	int last_lane = -1; // the lane of the last frame (-1: it went down the engine's stream) — whose events and counters ca3d_get_render_stats reads

	size_t buffer_words() const { return plane_words * nplanes; }
	size_t state_words() const { return plane_words * (slab ? nz : G); }
	double cells_per_plane() const { return (double)G * G; }
	double bytes_per_cell_step() const { return layout == CA3D_LAYOUT_PACKED32 ? 0.25 : 8.0; }
};

namespace ca3d
{

// ca3d_api.cpp: the message slot of ca3d_last_error() (one per thread), shared by every file of the library
void set_last_error(const char *msg) noexcept;
int fail(int code, const char *fmt, ...); // formats the message into the slot, returns `code`

#define HIP_TRY(expr)                                                                                          \
	do                                                                                                         \
	{                                                                                                          \
		hipError_t e_ = (expr);                                                                                \
		if (e_ != hipSuccess)                                                                                  \
			return ca3d::fail(e_ == hipErrorOutOfMemory ? CA3D_ERR_OUT_OF_MEMORY : CA3D_ERR_DEVICE, "%s: %s", #expr, \
			                  hipGetErrorString(e_));                                                          \
	} while (0)

int bind_device(ca3d_engine *h, bool join = true);
int check_ready(ca3d_engine *h);
void drop_graph(ca3d_engine *h);
void engine_state_edited(ca3d_engine *h); // the current buffer was edited in place on the engine's stream: no previous state, derived render data stale
int engine_mark_state(ca3d_engine *h); // both buffers zeroed on the engine's stream, "has a state" — for engines whose state arrives by device copies
// ca3d_device_buffer for a writer inside the library (the group's peer copies): the state counts as rewritten by THIS call only — the
// public call must assume writes at any later time and makes every frame rebuild its derived buffers while the pointer is valid
int engine_state_buffer(ca3d_engine *h, int which, void **device_ptr, size_t *n_bytes);

// ca3d_step.cpp
// Longest captured batch: consecutive graph launches leave a few microseconds of idle GPU between them, negligible
// against 1024 steps; a batch of n < 1024 steps gets a graph of exactly n steps (cached per n and start buffer).
constexpr uint32_t kMaxGraphSteps = 1024;
constexpr size_t kResStatusBytes = (4 + 1024) * sizeof(uint32_t); // abort word + per-tile progress words
struct ResidentShape { uint32_t rows, zsplit; int pair; };
ResidentShape resident_shape(const ca3d_engine *h);
bool resident_wanted(const ca3d_engine *h, uint32_t n); // a batch of n steps goes to the resident kernel
void reported_kernel_name(const ca3d_engine *h, char *out, size_t n_bytes);
void refresh_kernels(ca3d_engine *h); // (re)select the kernels, check their residency, leave a note in ca3d_last_error when a specialisation failed
int enqueue_step(ca3d_engine *h, int src, uint32_t lo, uint32_t hi, hipStream_t s, bool fused = false, uint32_t lo2 = 0, uint32_t hi2 = 0);
bool graphs_allowed(const ca3d_engine *h);
int step_graph(ca3d_engine *h, uint32_t n, uint32_t start, ca3d_engine::StepGraph **out);
int resident_slab_steps(ca3d_engine *h, uint32_t n);
int check_resident(ca3d_engine *h);
int settle_resident(ca3d_engine *h);
int record_batch_stats(ca3d_engine *h, uint32_t steps, uint64_t launches, uint32_t planes);
int flush_queued(ca3d_engine *h);

#define FLUSH_QUEUED(h)                   \
	do                                    \
	{                                     \
		int rcq_ = ca3d::flush_queued(h); \
		if (rcq_) return rcq_;            \
	} while (0)

// Whatever `enqueue()` puts on the engine's stream, captured and instantiated as a graph.
template <class Enqueue> int capture_graph(ca3d_engine *h, Enqueue &&enqueue, hipGraphExec_t *exec)
{
	hipGraph_t graph = nullptr;
	HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
	int rc = enqueue();
	hipError_t e = hipStreamEndCapture(h->stream, &graph);
	if (rc != CA3D_OK) { if (graph) hipGraphDestroy(graph); return rc; }
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(e));
	e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
	hipGraphDestroy(graph);
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e));
	return CA3D_OK;
}

// ca3d_slab.cpp
void free_slab_comm(ca3d_engine *h); // communicator, its stream and events (ca3d_destroy)
int engines_rccl_init_all(ca3d_engine **engines, int n);
int engines_rccl_exchange_all(ca3d_engine **engines, int n);

// ca3d_render.cpp
void free_render_targets(ca3d_engine *h);
int join_frames(ca3d_engine *h);
int clear_render_history(ca3d_engine *h);

} // namespace ca3d
