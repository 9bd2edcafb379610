// The renderer's front end in the C-ABI layer: ca3d_render cut into its steps (targets, counters, lanes, derived buffers, launch,
// read-back), the frames in flight (ca3d_engine::FrameLane), the render targets and their getters. The kernels are render.hip,
// render_stream.hip and render_frame.hip.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ca3d_engine.h"

namespace ca3d
{

void free_render_targets(ca3d_engine *h)
{
	if (h->r_present) hipFree(h->r_present);
	for (int i = 0; i < 2; i++)
	{
		if (h->r_light[i]) hipFree(h->r_light[i]);
		if (h->r_depth[i]) hipFree(h->r_depth[i]);
		h->r_light[i] = nullptr;
		h->r_depth[i] = nullptr;
	}
	h->r_present = nullptr;
	h->rw = h->rh = 0;
}

// Converged frames in flight when option render_pipeline is 1, and the share of the chip's wave slots each frame's persistent walk launches
// ask for while other frames are in flight beside it. Measured on the bench's dense 512^3 scene (tools/sweep_stream_wgs.sh, ms per frame;
// lanes x share): 1080p 4 spp   3 x 100 % 0.485 | 3 x 34 % 0.393 | 4 x 25 % 0.367 | 4 x 17 % 0.397      (one frame at a time: 0.627)
//                 2560 x 1440   3 x 100 % 0.746 | 3 x 34 % 0.641 | 4 x 25 % 0.612
//                 3200 x 1800   3 x 100 % 1.054 | 3 x 34 % 0.968 | 4 x 25 % 0.936
//                 3840 x 2160   2 x 100 % 1.386 | 2 x 50 % 1.35-1.40 | 3 x 100 % 1.389 | 3 x 67 % 1.37-1.38 | 3 x 34 % 1.419 | 4 x 25 % 1.466   (one at a time: 1.539)
// — frames whose walks run SIDE BY SIDE on equal shares of the chip beat frames that fill the chip one after the other and overlap only
// tail to head; how many of them depends on the frame: small frames want many narrow ones (their walks are short against their tails),
// at 3840 x 2160 (33 M samples, 0.7 GB of scratch per frame in flight) narrow walks only get in the way of the frame's other, full-width
// passes and nothing is more than 2 % from anything else.
// So: up to 24 M samples a frame four frames on a quarter of the chip each, above that three on two thirds each.
// CA3D_RENDER_LANES=2..4 / CA3D_STREAM_WGS_PCT (tuning) override both.
static int render_default_lanes(size_t samples)
{
	static const int env = getenv("CA3D_RENDER_LANES") ? atoi(getenv("CA3D_RENDER_LANES")) : 0;
	if (env >= 2 && env <= ca3d_engine::kMaxLanes) return env;
	return samples <= (24u << 20) ? 4 : 3;
}
static int render_walk_share(size_t samples, int lanes) { return lanes < 2 ? 100 : (samples <= (24u << 20) ? 100 / lanes : 67); }

// the engine's stream waits for the frames in flight on the lanes (nothing is waited for on the host)
int join_frames(ca3d_engine *h)
{
	for (auto &L : h->lanes)
		if (L.pending)
		{
			HIP_TRY(hipStreamWaitEvent(h->stream, L.done, 0));
			L.pending = false;
		}
	return CA3D_OK;
}

// forget the temporal history (a fresh canvas): the next literal frame sees zeros, as on the reference's first frame. (rw / rh are only
// non-zero once all five surfaces exist: free_render_targets zeroes them before the allocations.)
int clear_render_history(ca3d_engine *h)
{
	const size_t px = (size_t)h->rw * h->rh;
	for (int i = 0; i < 2 && px && h->r_light[i] && h->r_depth[i]; i++)
	{
		HIP_TRY(hipMemsetAsync(h->r_light[i], 0, px * 8, h->stream));
		HIP_TRY(hipMemsetAsync(h->r_depth[i], 0, px * 4, h->stream));
	}
	return CA3D_OK;
}

// diagnostics: CA3D_RENDER_TRACE=<file> makes every wave of the scheduled kernel record when and where it ran
// (tools/render_trace.py draws the occupancy timeline from the file)
static const char *render_trace_path()
{
	static const char *path = getenv("CA3D_RENDER_TRACE");
	return path;
}
static bool render_aux_off()
{
	static const bool off = getenv("CA3D_RENDER_AUX") && atoi(getenv("CA3D_RENDER_AUX")) == 0; // tuning: everything on one stream
	return off;
}

// One ca3d_render call on its way through the steps below, in the order ca3d_render calls them.
struct Frame
{
	uint32_t width, height, spp;
	bool to_host;                          // the caller takes a target back on the host
	const char *trace_path;
	size_t counter_words = 0;
	ca3d_engine::FrameLane *L = nullptr;   // the lane the frame runs on; null: the engine's stream
	int active_lanes = 0;
	hipStream_t rs = nullptr;              // the stream the frame runs on
	unsigned long long *counters = nullptr;
	uint64_t state_key[3] = {0, 0, 0};     // what the occupancy bits / the bricks were built from
	bool occ_built = false, bricks_built = false;
	RenderLaunch l;
};

// frames in flight (FrameLane): converged frames of a packed volume that stay on the device and go down the stream passes
// The first frame after a step, an upload or any other call on the engine's stream is drawn ON that stream: it has to wait for that call,
// which waited for every earlier frame — nothing can be in flight beside it, and on a lane it would only pay two cross-stream hand-offs
// (a host that steps between frames: 0.628 against 0.564 ms per step + frame, tools/run_render_step_loop.py). The frames behind it go
// down the lanes.
static bool frame_pipelined(const ca3d_engine *h, const Frame &f)
{
	const bool first_after_touch = h->state_touched;
	return !first_after_touch && h->render_pipeline && h->render_mode == 0 && !f.to_host && h->stream == h->own_stream &&
	       h->layout == CA3D_LAYOUT_PACKED32 && h->render_stream && h->render_sched && !h->render_indirect && !h->render_stream_check && !f.trace_path &&
	       !render_aux_off() && !h->render_row0 && !h->render_row1 && f.width == h->rw && f.height == h->rh;
}

// _createResolutionDependentAssests (main_pathtraced.js:729-779)
static int size_render_targets(ca3d_engine *h, const Frame &f)
{
	if (f.width == h->rw && f.height == h->rh) return CA3D_OK;
	const size_t px = (size_t)f.width * f.height;
	HIP_TRY(hipStreamSynchronize(h->stream)); // (a frame of a new size is never pipelined: the lanes were joined above)
	free_render_targets(h);
	HIP_TRY(hipMalloc((void **)&h->r_present, px * 4));
	for (int i = 0; i < 2; i++)
	{
		HIP_TRY(hipMalloc(&h->r_light[i], px * 8));
		HIP_TRY(hipMalloc((void **)&h->r_depth[i], px * 4));
		HIP_TRY(hipMemsetAsync(h->r_light[i], 0, px * 8, h->stream));
		HIP_TRY(hipMemsetAsync(h->r_depth[i], 0, px * 4, h->stream));
	}
	h->rw = f.width;
	h->rh = f.height;
	h->r_swap = 0;
	return CA3D_OK;
}

// the engine's counters: eight words, and behind them the wave records of a traced frame (render_trace_path)
static int size_render_counters(ca3d_engine *h, Frame &f)
{
	const size_t trace_waves = f.trace_path ? ((size_t)(f.width + 31u) / 32u * 2u) * ((f.height + 15u) / 16u * 4u) : 0u; // wave tiles of 16 x 4 pixels
	f.counter_words = 8u + 4u * trace_waves;
	if (h->r_counters && h->r_counter_words < f.counter_words) { HIP_TRY(hipFree(h->r_counters)); h->r_counters = nullptr; }
	if (!h->r_counters)
	{
		HIP_TRY(hipMalloc((void **)&h->r_counters, f.counter_words * sizeof(unsigned long long)));
		h->r_counter_words = f.counter_words;
	}
	return CA3D_OK;
}

// the lanes: streams that the runtime has put on pairwise DIFFERENT hardware queues (probed: ca_diag.hip) — two streams on one queue
// run in order and a frame would only queue up behind the other. Fewer than two such streams: no pipeline.
static int create_lanes(ca3d_engine *h, int want_lanes)
{
	for (auto &fl : h->lanes)
		if (fl.s && fl.pending) HIP_TRY(hipStreamSynchronize(fl.s)); // (the probe needs idle streams)
	if (!h->lanes[0].s) { HIP_TRY(hipStreamCreateWithFlags(&h->lanes[0].s, hipStreamNonBlocking)); h->n_lanes = 1; }
	for (int tries = 0; tries < 10 && h->n_lanes < want_lanes; tries++)
	{
		hipStream_t cand = nullptr;
		HIP_TRY(hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
		bool side_by_side = true;
		for (int i = 0; i < h->n_lanes && side_by_side; i++) HIP_TRY(streams_concurrent(h->lanes[i].s, cand, &side_by_side));
		if (side_by_side) h->lanes[h->n_lanes++].s = cand;
		else h->lane_spares.push_back(cand);
	}
	if (h->n_lanes < want_lanes) h->lanes_exhausted = true; // the runtime has no more queues to give: do not probe again on every frame
	if (h->n_lanes < 2) h->render_pipeline = 0;
	else
		for (int i = 0; i < h->n_lanes; i++)
		{
			ca3d_engine::FrameLane &fl = h->lanes[i];
			if (fl.done) continue;
			HIP_TRY(hipEventCreateWithFlags(&fl.done, hipEventDisableTiming));
			HIP_TRY(hipEventCreate(&fl.start));
			HIP_TRY(hipEventCreate(&fl.stop));
			HIP_TRY(hipMalloc((void **)&fl.counters, 8u * sizeof(unsigned long long)));
		}
	if (!h->ev_state) HIP_TRY(hipEventCreateWithFlags(&h->ev_state, hipEventDisableTiming));
	return CA3D_OK;
}

// where this frame runs: the engine's stream, or the next lane
static int pick_lane(ca3d_engine *h, Frame &f, bool pipelined)
{
	f.l.walk_share_pct = 100;
	f.rs = h->stream;
	f.counters = h->r_counters;
	const size_t frame_samples = (size_t)f.width * f.height * f.spp;
	const int want_lanes = h->render_pipeline >= 2 ? (h->render_pipeline < ca3d_engine::kMaxLanes ? h->render_pipeline : ca3d_engine::kMaxLanes) : render_default_lanes(frame_samples);
	if (pipelined && h->n_lanes < want_lanes && !h->lanes_exhausted)
		if (int rc = create_lanes(h, want_lanes)) return rc;
	f.active_lanes = h->n_lanes < want_lanes ? h->n_lanes : want_lanes;
	if (!(pipelined && h->render_pipeline && f.active_lanes >= 2)) return CA3D_OK;
	if (h->lane_next >= f.active_lanes) h->lane_next = 0;
	ca3d_engine::FrameLane *L = f.L = &h->lanes[h->lane_next];
	h->lanes_in_use = f.active_lanes;
	// is another frame still in flight beside this one? Then this frame's walks take their share of the chip (render_walk_share); a
	// frame that finds the lanes idle — a host that draws one frame per display refresh — takes the whole chip and is done sooner.
	// (A frame that has to wait for the engine's stream — a step or an upload since the last frame — starts after every earlier frame:
	// the engine's stream joined them before that call's work. It runs alone whatever is still in flight now.)
	bool beside = false;
	for (int i = 0; i < f.active_lanes && !beside && !h->main_touched; i++)
		if (&h->lanes[i] != L && h->lanes[i].used)
		{
			const hipError_t q = hipEventQuery(h->lanes[i].done);
			if (q == hipErrorNotReady) { beside = true; (void)hipGetLastError(); }
			else if (q != hipSuccess) HIP_TRY(q);
		}
	f.l.walk_share_pct = beside ? render_walk_share(frame_samples, f.active_lanes) : 100;
	if (h->main_touched)
	{
		// the steps and uploads in front of this frame — recorded only when an entry point has touched the engine's stream since the last
		// record (a marker behind another lane's frames on a shared hardware queue would make this frame wait for them)
		HIP_TRY(hipEventRecord(h->ev_state, h->stream));
		h->main_touched = false;
		for (auto &fl : h->lanes) fl.need_state = true;
	}
	if (L->need_state)
	{
		HIP_TRY(hipStreamWaitEvent(L->s, h->ev_state, 0));
		L->need_state = false;
	}
	f.rs = L->s;
	f.counters = L->counters;
	return CA3D_OK;
}

// clears the frame's counters and fills in what every frame's launch is given
static int begin_launch(ca3d_engine *h, Frame &f, const float *uniforms)
{
	HIP_TRY(hipMemsetAsync(f.counters, 0, (f.trace_path ? f.counter_words : 8u) * sizeof(unsigned long long), f.rs)); // [3]: the tile queue's head
	RenderLaunch &l = f.l;
	l.trace = f.trace_path != nullptr;
	l.cells = h->buf[h->cur];
	l.G = h->G;
	l.W = f.width;
	l.H = f.height;
	l.spp = f.spp;
	l.uniforms = uniforms;
	l.presentation = h->r_present;
	l.light = h->r_light[h->r_swap];
	l.depth = h->r_depth[h->r_swap];
	l.counters = f.counters;
	if (h->buffers_exposed) h->state_serial++; // a caller holds a pointer to the state and may have written it since the last frame
	f.state_key[0] = h->state_serial;
	f.state_key[1] = h->step;
	f.state_key[2] = (uint64_t)(uintptr_t)l.cells;
	return CA3D_OK;
}

// empty-space skipping: room for the block-occupancy bits, and whether an earlier frame built them from this very state
static int prepare_occupancy(ca3d_engine *h, Frame &f)
{
	if (!(h->render_skip && h->layout == CA3D_LAYOUT_PACKED32)) return CA3D_OK;
	const size_t fine = (size_t)(h->G / 32u) * (h->G / 8u) * (h->G / 8u); // fine bits, count word, coarse bits (render.hip)
	const size_t words = (fine + 63u) / 64u + 1u + (fine / 64u + 63u) / 64u + 3u; // (+ the six words of the live box)
	if (words != h->r_occ_words)
	{
		h->r_occ_key[0] = 0;
		for (auto &fl : h->lanes)
			if (fl.s) HIP_TRY(hipStreamSynchronize(fl.s));
		if (h->r_occ) HIP_TRY(hipFree(h->r_occ));
		h->r_occ = nullptr;
		h->r_occ_words = 0;
		HIP_TRY(hipMalloc((void **)&h->r_occ, words * sizeof(unsigned long long)));
		h->r_occ_words = words;
	}
	f.l.occ = h->r_occ;
	f.l.occ_valid = !memcmp(f.state_key, h->r_occ_key, sizeof f.state_key);
	f.l.occ_built = &f.occ_built;
	return CA3D_OK;
}

// the engine's render options into the launch; the combinations that are not implemented
static int apply_render_options(const ca3d_engine *h, Frame &f)
{
	RenderLaunch &l = f.l;
	l.mode = h->render_mode;
	l.sched = h->render_sched;
	l.indirect = h->render_indirect != 0;
	if (l.indirect && (h->render_mode != 0 || h->layout != CA3D_LAYOUT_PACKED32)) return fail(CA3D_ERR_UNSUPPORTED, "render_indirect is implemented for the converged-frame mode over the packed layout");
	l.row0 = h->render_row0;
	l.row1 = h->render_row1 > f.height ? f.height : h->render_row1;
	if (l.row1 && l.row0 >= l.row1) return fail(CA3D_ERR_INVALID_ARGUMENT, "render rows [%u, %u) are empty for a target of %u rows", l.row0, h->render_row1, f.height);
	if ((l.row0 || l.row1) && h->render_mode != 0) return fail(CA3D_ERR_UNSUPPORTED, "row bands are implemented for the converged-frame mode only");
	l.legacy = h->layout == CA3D_LAYOUT_UNPACKED; // legacy volume -> legacy shader (pathtraced_fragment.wgsl)
	l.prev_light = h->r_light[h->r_swap ^ 1]; // group 1 of the render pass: last frame's targets (1519-1555, 1787)
	l.prev_depth = h->r_depth[h->r_swap ^ 1];
	return CA3D_OK;
}

// the second stream of a frame on the engine's stream (RenderLaunch::aux)
static int prepare_aux_stream(ca3d_engine *h, Frame &f)
{
	if (f.L) return CA3D_OK; // (a lane is ONE stream: its side kernels run behind its stream passes, the other lane's frame fills the chip meanwhile)
	if (render_aux_off() || h->render_mode != 0 || !h->render_sched || f.trace_path) return CA3D_OK;
	if (!h->r_aux)
	{
		HIP_TRY(hipStreamCreateWithFlags(&h->r_aux, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&h->r_fork, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&h->r_join, hipEventDisableTiming));
	}
	f.l.aux = h->r_aux;
	f.l.ev_fork = h->r_fork;
	f.l.ev_join = h->r_join;
	return CA3D_OK;
}

// scratch of the ray-stream passes: the lane's, or the engine's
static int prepare_stream_scratch(ca3d_engine *h, Frame &f)
{
	RenderLaunch &l = f.l;
	if (!(h->render_stream && h->render_mode == 0 && h->render_sched && !l.legacy && !l.indirect && !f.trace_path)) return CA3D_OK;
	size_t o0, o1, o2;
	const size_t need = stream_scratch_bytes(f.width, f.height, f.spp, &o0, &o1, &o2);
	void *&scratch = f.L ? f.L->scratch : h->r_stream;
	size_t &scratch_bytes = f.L ? f.L->scratch_bytes : h->r_stream_bytes;
	if (scratch_bytes < need)
	{
		HIP_TRY(hipStreamSynchronize(f.rs));
		if (scratch) HIP_TRY(hipFree(scratch));
		scratch = nullptr;
		scratch_bytes = 0;
		HIP_TRY(hipMalloc(&scratch, need));
		scratch_bytes = need;
	}
	l.stream_scratch = scratch;
	l.stream_check = h->render_stream_check != 0;
	// the check below reads the passes' control words after the frame: zero them here, for a frame whose stream passes do not run
	// (volume off screen or outside the band) would otherwise report an earlier frame's counts — or, on fresh scratch, noise
	if (l.stream_check) HIP_TRY(hipMemsetAsync(scratch, 0, 4096, f.rs));
	return CA3D_OK;
}

// room for the bricked copy of the volume, and whether an earlier frame built it from this very state
static int prepare_bricks(ca3d_engine *h, Frame &f)
{
	if (!(h->render_frame_bricks && frame_bricks_applies(h->G) && (h->render_mode == 1 || f.l.stream_scratch))) return CA3D_OK;
	const size_t need = frame_bricks_bytes(h->G);
	if (h->r_bricks_bytes != need)
	{
		HIP_TRY(hipStreamSynchronize(h->stream));
		for (auto &fl : h->lanes)
			if (fl.s) HIP_TRY(hipStreamSynchronize(fl.s));
		if (h->r_bricks) HIP_TRY(hipFree(h->r_bricks));
		h->r_bricks = nullptr;
		h->r_bricks_bytes = 0;
		HIP_TRY(hipMalloc((void **)&h->r_bricks, need));
		h->r_bricks_bytes = need;
		h->r_bricks_key[0] = 0;
	}
	f.l.bricks = h->r_bricks;
	f.l.bricks_valid = !memcmp(f.state_key, h->r_bricks_key, sizeof f.state_key);
	f.l.bricks_built = &f.bricks_built;
	return CA3D_OK;
}

// what a frame on a lane shares with the frames on the other lanes
static int cross_lane_waits(ca3d_engine *h, Frame &f)
{
	if (!f.L) return CA3D_OK;
	RenderLaunch &l = f.l;
	// the presentation surface is shared: this frame's pixels after those of the frame before it (which waited for the one before that)
	if (h->last_lane >= 0 && h->last_lane != h->lane_next && h->lanes[h->last_lane].used) l.after = h->lanes[h->last_lane].done;
	// the occupancy bits and the bricks are shared too: a frame that rebuilds them waits for the frames that may still be reading them
	const bool occ_rebuild = l.occ && !l.occ_valid, bricks_rebuild = l.bricks && !l.bricks_valid;
	if (occ_rebuild || bricks_rebuild)
		for (auto &fl : h->lanes)
			if (&fl != f.L && fl.used) HIP_TRY(hipStreamWaitEvent(f.rs, fl.done, 0));
	return CA3D_OK;
}

// the frame itself between its two timing events; the keys of the derived buffers it rebuilt, the lane's `done` event
static int launch_frame(ca3d_engine *h, Frame &f)
{
	ca3d_engine::FrameLane *L = f.L;
	HIP_TRY(hipEventRecord(L ? L->start : h->rev_start, f.rs));
	hipError_t e = launch_render(f.l, f.rs);
	if (e != hipSuccess)
	{
		h->r_occ_key[0] = h->r_bricks_key[0] = 0; // whatever was half built is not to be trusted
		return fail(CA3D_ERR_DEVICE, "render launch failed: %s", hipGetErrorString(e));
	}
	// the derived buffers this call rebuilt now describe this state; the ones it did not touch keep the key of the state they were built from
	if (f.occ_built) memcpy(h->r_occ_key, f.state_key, sizeof f.state_key);
	if (f.bricks_built) memcpy(h->r_bricks_key, f.state_key, sizeof f.state_key);
	HIP_TRY(hipEventRecord(L ? L->stop : h->rev_stop, f.rs));
	h->rev_valid = true;
	h->last_lane = L ? h->lane_next : -1;
	if (L)
	{
		HIP_TRY(hipEventRecord(L->done, f.rs));
		L->pending = L->used = true;
		h->lane_next = (h->lane_next + 1) % f.active_lanes;
	}
	return CA3D_OK;
}

// diagnostics read back after the frame: the wave trace, the stream passes' self-check
static int read_back_diagnostics(ca3d_engine *h, const Frame &f)
{
	if (f.trace_path)
	{
		std::vector<unsigned long long> t(f.counter_words);
		HIP_TRY(hipStreamSynchronize(h->stream));
		HIP_TRY(hipMemcpy(t.data(), h->r_counters, f.counter_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		if (FILE *file = fopen(f.trace_path, "wb")) // the last frame wins
		{
			fwrite(t.data(), sizeof(unsigned long long), f.counter_words, file);
			fclose(file);
		}
	}
	if (f.l.stream_scratch && f.l.stream_check)
	{
		// diagnostics: the stream passes counted where their interval filter and the reference's slab test disagreed (must be nowhere)
		uint32_t bad[4] = {0, 0, 0, 0};
		HIP_TRY(hipStreamSynchronize(h->stream));
		HIP_TRY(hipMemcpy(bad, static_cast<const uint32_t *>(f.l.stream_scratch) + 2, sizeof bad, hipMemcpyDeviceToHost));
		if (bad[0]) return fail(CA3D_ERR_DEVICE, "render_stream_check: the interval filter contradicted the slab test at %u live cells", bad[0]);
		if (bad[1]) return fail(CA3D_ERR_DEVICE, "render_stream_check: %u looked-up answers had not been given in this frame (jobs lost by the queues; jobs %u .. %u)", bad[1], ~bad[2], bad[3]);
	}
	return CA3D_OK;
}
} // namespace ca3d

using namespace ca3d;

extern "C"
{

int ca3d_render_target(ca3d_t *h, int which, void **device_ptr, size_t *n_bytes) CA3D_API_TRY
{
	if (!h || !device_ptr || !n_bytes) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!h->r_present) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_render has not been called yet");
	if (int rcb = bind_device(h)) return rcb; // (whoever reads the target after the engine's stream also reads it after the frames in flight)
	const size_t px = (size_t)h->rw * h->rh;
	switch (which)
	{
	case 0: *device_ptr = h->r_present; *n_bytes = px * 4; break;
	case 1: *device_ptr = h->r_light[h->r_swap ^ 1]; *n_bytes = px * 8; break; // the surfaces the LAST frame was written to
	case 2: *device_ptr = h->r_depth[h->r_swap ^ 1]; *n_bytes = px * 4; break;
	default: return fail(CA3D_ERR_INVALID_ARGUMENT, "target must be 0 (presentation), 1 (light) or 2 (depth)");
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_render(ca3d_t *h, const float uniforms[128], uint32_t width, uint32_t height, uint32_t spp,
                uint8_t *presentation_rgba8, uint16_t *light_rgba16f, uint16_t *depth_rg16f) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!h->configured || !h->has_state) return fail(CA3D_ERR_NOT_CONFIGURED, "no state to render: configure and upload first");
	FLUSH_QUEUED(h);
	if (h->slab) return fail(CA3D_ERR_UNSUPPORTED, "the renderer reads a full grid, not a slab");
	if (h->layout == CA3D_LAYOUT_UNPACKED && h->render_mode != 0) return fail(CA3D_ERR_UNSUPPORTED, "the literal frame mode is implemented for the packed layout only");
	if (!uniforms) return fail(CA3D_ERR_INVALID_ARGUMENT, "uniforms is NULL");
	if (width == 0 || height == 0 || width > 16384u || height > 16384u) return fail(CA3D_ERR_INVALID_ARGUMENT, "bad target size %ux%u", width, height);
	if (spp != 1 && spp != 4) return fail(CA3D_ERR_INVALID_ARGUMENT, "spp must be 1 or 4");
	if (h->render_mode == 1 && spp != 1) return fail(CA3D_ERR_INVALID_ARGUMENT, "the literal frame mode takes one jittered sample per pixel (spp = 1)");
	Frame f;
	f.width = width;
	f.height = height;
	f.spp = spp;
	f.to_host = presentation_rgba8 || light_rgba16f || depth_rg16f;
	f.trace_path = render_trace_path();
	const bool pipelined = frame_pipelined(h, f);
	int rc = bind_device(h, !pipelined);
	if (rc) return rc;
	// The frame shows a state the engine has verified — when the caller gets the frame back on the host. A frame that stays on the
	// device (no host pointers: the reference's render pass, which only enqueues) does not block on the step batch in front of it: a
	// resident launch that has ALREADY given up (pinned flag set) is recovered first, one still running is left pending — the next
	// call that waits for the stream verifies it, and a frame drawn from a launch that later turns out to have timed out (a foreign
	// kernel holding CUs for 200 ms) is simply the wrong frame once.
	if (f.to_host || (h->res_status_host && *h->res_status_host)) rc = settle_resident(h);
	if (rc) return rc;
	if ((rc = size_render_targets(h, f))) return rc;
	if ((rc = size_render_counters(h, f))) return rc;
	if ((rc = pick_lane(h, f, pipelined))) return rc;
	if ((rc = begin_launch(h, f, uniforms))) return rc;
	if ((rc = prepare_occupancy(h, f))) return rc;
	if ((rc = apply_render_options(h, f))) return rc;
	if ((rc = prepare_aux_stream(h, f))) return rc;
	if ((rc = prepare_stream_scratch(h, f))) return rc;
	if ((rc = prepare_bricks(h, f))) return rc;
	if ((rc = cross_lane_waits(h, f))) return rc;
	if ((rc = launch_frame(h, f))) return rc;
	if ((rc = read_back_diagnostics(h, f))) return rc;
	const size_t px = (size_t)width * height;
	h->rstats.primary_rays = (uint64_t)width * ((f.l.row1 ? f.l.row1 : height) - f.l.row0) * spp;
	if (presentation_rgba8) HIP_TRY(hipMemcpyAsync(presentation_rgba8, h->r_present, px * 4, hipMemcpyDeviceToHost, h->stream));
	if (light_rgba16f) HIP_TRY(hipMemcpyAsync(light_rgba16f, h->r_light[h->r_swap], px * 8, hipMemcpyDeviceToHost, h->stream));
	if (depth_rg16f) HIP_TRY(hipMemcpyAsync(depth_rg16f, h->r_depth[h->r_swap], px * 4, hipMemcpyDeviceToHost, h->stream));
	if (f.to_host) HIP_TRY(hipStreamSynchronize(h->stream));
	h->r_swap ^= 1;
	h->state_touched = false; // (set again by the next entry point that is not a frame: bind_device)
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_render_stats(ca3d_t *h, ca3d_render_stats *out) CA3D_API_TRY
{
	if (!h || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!h->rev_valid) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_render has not been called yet");
	int rc = bind_device(h);
	if (rc) return rc;
	// the last frame's events and counters: the engine's, or those of the lane it ran on (frames in flight)
	const ca3d_engine::FrameLane *L = h->last_lane >= 0 ? &h->lanes[h->last_lane] : nullptr;
	HIP_TRY(hipEventSynchronize(L ? L->stop : h->rev_stop));
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, L ? L->start : h->rev_start, L ? L->stop : h->rev_stop));
	unsigned long long c[3] = {0, 0, 0};
	HIP_TRY(hipMemcpy(c, L ? L->counters : h->r_counters, sizeof c, hipMemcpyDeviceToHost));
	h->rstats.gpu_ms = ms;
	h->rstats.shadow_rays = c[0];
	h->rstats.primary_cell_visits = c[1];
	h->rstats.shadow_cell_visits = c[2];
	*out = h->rstats;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_render_pipeline(ca3d_t *h, int32_t *frames_in_flight) CA3D_API_TRY
{
	if (!h || !frames_in_flight) return fail(CA3D_ERR_INVALID_ARGUMENT, "ca3d_get_render_pipeline: NULL argument");
	*frames_in_flight = h->render_pipeline && h->n_lanes >= 2 ? h->lanes_in_use : 0; // of the last pipelined frame (the default depth follows the frame's size)
	return CA3D_OK;
}
CA3D_API_CATCH

} // extern "C"
