// The step path of the C-ABI layer: which kernels serve the current rules and grid (select_kernels, check_residency, the name
// ca3d_get_info reports), and how a batch of steps reaches the stream — kernel by kernel, as a captured graph, or as one launch of
// the resident kernel with its recovery. Everything a single step launch passes through (submit_steps -> step_graph / enqueue_batch
// -> enqueue_step) stays in this one translation unit: launching step by step costs about 6 us per step on the host.
#include <cstdio>
#include <cstring>

#include "ca3d_engine.h"

namespace ca3d
{

static int submit_steps(ca3d_engine *h, uint32_t n_steps); // (the recovery in check_resident re-runs steps)

// One launch reading buffer `src` over output planes [lo, hi) (plus [lo2, hi2) when given: the packed class kernels
// take both ranges in one launch): a single step, or a fused multi-step pass.
int enqueue_step(ca3d_engine *h, int src, uint32_t lo, uint32_t hi, hipStream_t s, bool fused, uint32_t lo2, uint32_t hi2)
{
	PlaneRange pr;
	pr.G = h->G;
	pr.nplanes = h->nplanes;
	pr.zbase = h->slab ? (int32_t)h->z0 - (int32_t)h->ghost : 0;
	pr.lo = lo;
	pr.hi = hi;
	pr.wrap_full = h->slab ? 0u : 1u;
	hipError_t e;
	if (h->layout == CA3D_LAYOUT_PACKED32)
	{
		pr.lo2 = lo2;
		pr.hi2 = hi2;
		PackedLaunch l{h->buf[src], h->buf[src ^ 1], pr, &h->rules, h->variant, h->vn_jit.cvl >= 0 ? &h->vn_jit : nullptr, h->class_jit.main >= 0 ? &h->class_jit : nullptr, (h->roll_jit.cvl >= 0 || h->roll_jit.cv_np2 > 0) ? &h->roll_jit : nullptr, h->roll_z, h->roll_tile, h->rows_jit.main >= 0 ? &h->rows_jit : nullptr};
		e = fused ? launch_packed_fused(l, s) : launch_packed_step(l, s);
	}
	else
	{
		UnpackedLaunch l{h->buf[src], h->buf[src ^ 1], pr, &h->rules, h->binary_state && h->variant == 0};
		e = launch_unpacked_step(l, s, &h->unpacked_kernel);
		if (e == hipSuccess && hi2 > lo2)
		{
			l.pr.lo = lo2;
			l.pr.hi = hi2;
			e = launch_unpacked_step(l, s, &h->unpacked_kernel);
		}
		h->binary_state = true; // the kernel writes only 0 / 1 (compute.wgsl:160-174)
	}
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(e));
	return CA3D_OK;
}

// (Re)select the kernels for the current rules and grid; compiles the rule's specialisation when one applies. Called
// whenever rules, grid or the relevant options change — never from the step path (the WebGPU analogue is pipeline
// creation). A failed compile leaves the ahead-of-time kernels in charge.
// the 512^3 von Neumann form runs as the row-pair kernel (32-row tiles, one z group: its own geometry)
static int vn_pair(const ca3d_engine *h) { return h->res_pair && h->G == 512u && h->res_rows == 32u && h->res_zsplit == 1u ? 1 : 0; } // another geometry asked for: the general form

// the shape of a resident launch for the kernels selected: rows per tile, thread groups along z, row-pair form
ResidentShape resident_shape(const ca3d_engine *h)
{
	return {(h->res_class || vn_pair(h)) ? 32u : h->res_rows, h->res_class ? resident_class_zsplit(h->G) : h->res_zsplit, h->res_class ? 0 : vn_pair(h)};
}

// the resident kernel exists for the rules / grid and is switched on: full-grid engines, and the slab form
static bool resident_enabled(const ca3d_engine *h) { return h->res_ready && h->use_resident && !h->res_failed; }
static bool resident_slab_enabled(const ca3d_engine *h) { return h->res_slab_fn && h->use_resident && !h->res_failed; }
bool resident_wanted(const ca3d_engine *h, uint32_t n)
{
	return (h->slab ? resident_slab_enabled(h) : resident_enabled(h)) && n >= h->res_min && h->stream != nullptr;
}

static void select_kernels(ca3d_engine *h)
{
	h->vn_jit = VnJit{};
	h->class_jit = ClassJit{};
	h->rows_jit = RowsJit{};
	h->roll_jit = RollJit{};
	h->res_ready = false;
	h->res_class = false;
	h->res_jit_fn = nullptr;
	h->res_slab_fn = nullptr;
	h->jit_log.clear();
	if (!h->configured || !h->rules.valid) return;
	if (h->layout != CA3D_LAYOUT_PACKED32) { h->unpacked_kernel = "ca_unpacked_literal"; return; }
	if (h->slab && h->use_resident && h->use_jit)
	{
		// a rank's share of a 1024^3 grid: K sub-steps per launch with the slab on chip (ca_resident_kernel.inc, slab form)
		const int pz = resident_slab_planes(h->rules, h->G, h->nplanes, h->variant);
		if (pz && hipSetDevice(h->device) == hipSuccess)
		{
			uint32_t ls1 = 0, lb1 = 0;
			vn_tables(h->rules, &ls1, &lb1);
			if (jit_resident_slab_kernel(h->device, ls1, lb1, pz, &h->res_slab_fn, &h->jit_log) != CA3D_OK) h->res_slab_fn = nullptr;
		}
	}
	{
		// the resident kernel of the start-up rule is pre-built: available with or without the run-time compiler
		uint32_t ls0 = 0, lb0 = 0;
		if (h->use_resident && !h->slab && resident_kernel_applies(h->rules, h->G, h->variant))
		{
			vn_tables(h->rules, &ls0, &lb0);
			if (vn_tables_prebuilt(ls0, lb0)) h->res_ready = true;
		}
	}
	if (!h->use_jit) return;
	if (h->use_roll && roll_np2_applies(h->rules, h->G, h->variant))
	{
		// rows of 3, 5, 6 or 7 uint4 and a rule with diagonal neighbour classes: the rolling-window kernel's whole-rows-per-wave form
		if (hipSetDevice(h->device) != hipSuccess) return;
		RollJit rj;
		if (jit_roll_np2_kernels(h->device, h->rules, (int)(h->G / 128u), &rj, &h->jit_log) == CA3D_OK) { h->roll_jit = rj; return; }
	}
	if (h->use_rows && rows_kernel_applies(h->rules, h->G, h->variant))
	{
		// grids without a uint4 kernel that has the rule compiled in (not a power of two, or rows that are not whole uint4)
		if (hipSetDevice(h->device) != hipSuccess) return;
		RowsJit rj;
		if (jit_rows_kernels(h->device, h->rules, h->G, &rj, &h->jit_log) == CA3D_OK) h->rows_jit = rj;
		if (h->G == 64u && !h->res_ready && h->use_resident && !h->slab && resident_kernel_applies(h->rules, h->G, h->variant))
		{
			// 64^3, a von Neumann table pair other than the start-up rule's: the one-workgroup resident kernel compiled for the tables
			uint32_t ls64 = 0, lb64 = 0;
			vn_tables(h->rules, &ls64, &lb64);
			if (jit_resident_kernel(h->device, ls64, lb64, 64u, 1u, 0, &h->res_jit_fn, &h->jit_log) == CA3D_OK) h->res_ready = true;
		}
		return;
	}
	if (!vn_kernel_applies(h->rules, h->G, h->variant))
	{
		// class kernels on power-of-two grids: the rule's truth tables become compile-time constants
		const uint32_t cv = h->G / 128u;
		if (!use_class_kernel(h->rules, h->G, h->variant) || h->G % 128u || cv > 64u) return;
		if (hipSetDevice(h->device) != hipSuccess) return;
		ClassJit cj;
		if (jit_class_kernels(h->device, h->rules, &cj, &h->jit_log) == CA3D_OK) h->class_jit = cj;
		else return;
		if (cv & (cv - 1u)) return; // not a power of two: the class kernel's np2 entry points, nothing else
		if (h->use_roll && roll_kernel_applies(h->rules, h->G, h->variant))
		{
			RollJit rj;
			if (jit_roll_kernels(h->device, h->rules, vn_grid_log2(h->G), &rj, &h->jit_log) == CA3D_OK) h->roll_jit = rj;
		}
		if (h->use_resident && !h->slab && resident_class_applies(h->rules, h->G, h->variant) &&
		    jit_resident_class_kernel(h->device, h->rules, h->G, resident_class_zsplit(h->G), &h->res_jit_fn, &h->jit_log) == CA3D_OK)
		{
			h->res_ready = true;
			h->res_class = true;
		}
		return;
	}
	uint32_t ls = 0, lb = 0;
	vn_tables(h->rules, &ls, &lb);
	const bool resident = h->use_resident && !h->slab && resident_kernel_applies(h->rules, h->G, h->variant);
	if (vn_tables_prebuilt(ls, lb)) return;
	if (hipSetDevice(h->device) != hipSuccess) return;
	VnJit j;
	if (jit_vn_kernels(h->device, vn_grid_log2(h->G), ls, lb, &j, &h->jit_log) == CA3D_OK) h->vn_jit = j;
	const ResidentShape shape = resident_shape(h); // (the von Neumann form's: res_class is off here)
	if (resident && jit_resident_kernel(h->device, ls, lb, h->G == 256u ? 256u : shape.rows, shape.zsplit, shape.pair, &h->res_jit_fn, &h->jit_log) == CA3D_OK) h->res_ready = true;
}

// The name ca3d_get_info reports for the kernels selected above.
void reported_kernel_name(const ca3d_engine *h, char *out, size_t n_bytes)
{
	const char *name = "";
	const bool fused = h->configured && h->rules.valid && h->layout == CA3D_LAYOUT_PACKED32 && h->use_fused && !h->slab && packed_fused_steps(h->rules, h->G, h->variant) == 2;
	if (h->configured && h->rules.valid)
	{
		if (h->layout != CA3D_LAYOUT_PACKED32) name = h->step > 0 && h->unpacked_kernel[0] ? h->unpacked_kernel : "ca_unpacked";
		else if (fused) name = "ca_packed_fused+ca_packed_class";
		else if (resident_enabled(h)) name = h->res_class ? "ca_resident_class(jit)" : (h->res_jit_fn ? "ca_resident_vn(jit)" : "ca_resident_vn");
		else if (h->slab && resident_slab_enabled(h)) name = "ca_resident_slab_vn(jit)";
		else if (h->roll_jit.cv_np2 > 0) name = "ca_packed_roll_np2(jit)";
		else if (h->rows_jit.main >= 0) name = "ca_packed_rows(jit)";
		else name = h->vn_jit.cvl >= 0 ? "ca_packed_vn(jit)" : packed_kernel_name(h->rules, h->G, h->variant);
	}
	const bool class_jit = h->configured && h->rules.valid && h->layout == CA3D_LAYOUT_PACKED32 && h->class_jit.main >= 0 && strncmp(name, "ca_resident", 11) != 0 && !fused;
	if (class_jit && h->roll_jit.cvl >= 0 && !strncmp(name, "ca_packed_class", 15))
		snprintf(out, n_bytes, "ca_packed_class_roll%s(jit)", name + 15); // rolling-window form
	else
		snprintf(out, n_bytes, "%s%s", name, class_jit ? "(jit)" : "");
}

// A resident launch only completes when ALL its workgroups are on the chip at once (they wait for each other's faces). Ask the
// runtime before selecting one: occupancy of the chosen kernel per CU x the CUs the engine's stream may use (a CU mask, a
// partitioned device) against the tile count. Too few: the per-step kernels run, and ca3d_last_error says why. What the
// query cannot see (another process or stream holding CUs) is left to the kernels' bounded waits and the recovery below.
static void check_residency(ca3d_engine *h)
{
	h->res_note.clear();
	if (!h->res_ready && !h->res_slab_fn) return;
	if (hipSetDevice(h->device) != hipSuccess) return;
	uint32_t tiles = 0, cap = 0;
	char buf[256];
	if (h->res_ready)
	{
		const ResidentShape shape = resident_shape(h);
		if (resident_capacity(h->G, shape.rows, shape.zsplit, shape.pair, h->res_jit_fn, h->stream, &tiles, &cap) && cap < tiles)
		{
			h->res_ready = false;
			h->res_class = false;
			snprintf(buf, sizeof buf, "resident multi-step kernel not selected: it needs %u co-resident workgroups, this device / stream holds %u; per-step kernels in use", tiles, cap);
			h->res_note = buf;
		}
	}
	if (h->res_slab_fn && resident_slab_capacity(h->res_slab_fn, h->stream, &tiles, &cap) && cap < tiles)
	{
		h->res_slab_fn = nullptr;
		snprintf(buf, sizeof buf, "resident slab kernel not selected: it needs %u co-resident workgroups, this device / stream holds %u; per-step kernels in use", tiles, cap);
		h->res_note = buf;
	}
}

// A failed specialisation is not an error of the call that triggered it (the ahead-of-time kernels take over), but it
// must not be silent: the message goes where the caller looks (ca3d_last_error, ca3d_get_jit_log). Likewise a resident
// kernel that exists for the rules but cannot be co-resident on this device / stream.
static void note_jit_failure(const ca3d_engine *h)
{
	if (!h->jit_log.empty()) fail(0, "run-time kernel specialisation failed, pre-built kernels in use: %s", h->jit_log.c_str());
	else if (!h->res_note.empty()) set_last_error(h->res_note.c_str());
}

void refresh_kernels(ca3d_engine *h)
{
	select_kernels(h);
	check_residency(h);
	note_jit_failure(h);
}

constexpr size_t kMaxStepGraphs = 24; // cached graphs per engine (see kMaxGraphSteps, ca3d_engine.h)

// Launch plan for n steps that keeps the reference's ping-pong invariant (main_pathtraced.js:1580-1609): the
// state after n steps sits in buffer (start + n) % 2 and the other buffer holds the state one step earlier. A
// fused pass advances T = 2 steps but flips the buffer once, so fused passes come in even numbers and the batch
// always ends with single steps.
static void plan_steps(const ca3d_engine *h, uint32_t n, uint32_t *n_fused, uint32_t *n_single)
{
	uint32_t f = 0;
	if (h->use_fused && h->layout == CA3D_LAYOUT_PACKED32 && !h->slab && packed_fused_steps(h->rules, h->G, h->variant) == 2 && n >= 3)
	{
		f = (n - 1u) / 2u;
		f &= ~1u;
	}
	*n_fused = f;
	*n_single = n - 2u * f;
}

static int enqueue_batch(ca3d_engine *h, uint32_t n, uint32_t start_buf, hipStream_t s, uint64_t *launches)
{
	uint32_t f, single;
	plan_steps(h, n, &f, &single);
	uint32_t cur = start_buf;
	for (uint32_t i = 0; i < f; i++, cur ^= 1u)
	{
		int rc = enqueue_step(h, (int)cur, 0, h->G, s, true);
		if (rc) return rc;
	}
	for (uint32_t i = 0; i < single; i++, cur ^= 1u)
	{
		int rc = enqueue_step(h, (int)cur, 0, h->G, s, false);
		if (rc) return rc;
	}
	if (launches) *launches += f + single;
	return CA3D_OK;
}

// Captured batch of n steps starting from buffer `start` (built on first use).
int step_graph(ca3d_engine *h, uint32_t n, uint32_t start, ca3d_engine::StepGraph **out)
{
	const uint64_t key = ((uint64_t)start << 32) | n;
	auto it = h->step_graphs.find(key);
	if (it != h->step_graphs.end()) { *out = &it->second; return CA3D_OK; }
	if (h->step_graphs.size() >= kMaxStepGraphs)
	{
		// a caller cycling through many batch lengths: start over rather than grow without bound
		HIP_TRY(hipStreamSynchronize(h->stream));
		for (auto &kv : h->step_graphs) hipGraphExecDestroy(kv.second.exec);
		h->step_graphs.clear();
	}
	// Launch boundaries stay; the host cost per launch drops from ~4 us to the graph's amortised cost.
	uint64_t launches = 0;
	ca3d_engine::StepGraph g;
	int rc = capture_graph(h, [&]() { return enqueue_batch(h, n, start, h->stream, &launches); }, &g.exec);
	if (rc) return rc;
	g.launches = (uint32_t)launches;
	*out = &h->step_graphs.emplace(key, g).first->second;
	return CA3D_OK;
}

// Looks at the resident launches issued since the last look; the stream must have been waited for. Slab engines: a launch
// that timed out leaves an invalid state behind (the neighbours' ghosts were refreshed from it) — an error, the path goes
// off. Full-grid engines recover (see ca3d_engine::res_pending): the failed launch and the ones behind it wrote nothing, so
// the engine returns to the failed launch's input and runs all their steps through the per-step kernels, then waits for
// them. Success with the resident path switched off; ca3d_last_error carries the note.
int check_resident(ca3d_engine *h)
{
	if (!h->res_status_host) return CA3D_OK;
	if (!h->res_check && h->res_pending.empty()) return CA3D_OK;
	h->res_check = false;
	if (*h->res_status_host == 0) { h->res_pending.clear(); return CA3D_OK; }
	const uint32_t who = h->res_status_host[0], ep = h->res_status_host[1];
	h->res_failed = true; // per-step kernels from here on
	size_t idx = h->res_pending.size();
	for (size_t i = 0; i < h->res_pending.size(); i++)
		if (h->res_pending[i].epoch0 == ep) { idx = i; break; }
	if (h->slab || idx == h->res_pending.size())
	{
		h->res_pending.clear();
		h->has_state = false;
		return fail(CA3D_ERR_DEVICE, "resident multi-step kernel: a wait for neighbour tile faces timed out (tile %u gave up first) — were all its "
		            "workgroups resident? The state is invalid: upload it again; the engine now uses the per-step kernels", who - 1u);
	}
	const ca3d_engine::ResPending p = h->res_pending[idx];
	uint64_t total = 0;
	for (size_t i = idx; i < h->res_pending.size(); i++) total += h->res_pending[i].n;
	h->res_pending.clear();
	drop_graph(h);
	// The three buffers only rotate: whichever of them is neither the failed launch's input nor its other buffer is the spare — not
	// `p.spare`, which is null when that launch was a one-step one issued before a later queued launch allocated the third buffer
	// (restoring null would leak it).
	uint32_t *third = p.spare;
	for (uint32_t *q : {h->buf[0], h->buf[1], h->spare})
		if (q && q != p.in && q != p.other) third = q;
	h->buf[p.cur_before] = p.in;
	h->buf[p.cur_before ^ 1u] = p.other;
	h->spare = third;
	h->cur = p.cur_before;
	h->step = p.step_before;
	h->state_serial++; // whatever the renderer derived from the buffers of the failed launches is void
	// ... and so is what frames drawn in the meantime left behind: ca3d_render without host pointers does not wait for a pending
	// resident launch (the frame loop must not stall on it), so a frame may have been drawn from the unwritten output of the launch
	// that has now turned out to have failed — wrong once on screen, but in the literal mode it was also blended into the history
	// surfaces and would linger for several frames (EMA, alpha 0.1). A fresh canvas instead.
	if (int rch = clear_render_history(h)) return rch;
	HIP_TRY(hipMemsetAsync(h->res_mail, 0, h->res_mail_bytes, h->stream));
	HIP_TRY(hipMemsetAsync(h->res_status, 0, kResStatusBytes, h->stream));
	h->res_status_host[0] = h->res_status_host[1] = 0;
	h->res_epoch = 0;
	h->res_recovered++;
	char note[256];
	snprintf(note, sizeof note, "resident multi-step kernel: a wait for neighbour tile faces timed out (tile %u gave up first); the %llu steps "
	         "it and the launches behind it covered were re-run through the per-step kernels, which stay in use", who - 1u, (unsigned long long)total);
	h->res_note = note;
	while (total)
	{
		const uint32_t n = total > 0x40000000ull ? 0x40000000u : (uint32_t)total;
		int rc = submit_steps(h, n);
		if (rc) return rc;
		total -= n;
	}
	HIP_TRY(hipStreamSynchronize(h->stream));
	set_last_error(h->res_note.c_str());
	return CA3D_OK;
}

// Before anything that reads the state, hands out its buffers or changes how steps run: make sure no unverified resident
// launch is outstanding (wait for the stream, recover if one gave up). Costs nothing when none is.
int settle_resident(ca3d_engine *h)
{
	if (h->res_pending.empty() && !h->res_check) return CA3D_OK;
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(h->stream));
	return check_resident(h);
}

// n steps as ONE launch of the resident kernel (state in registers between steps).
static int resident_buffers(ca3d_engine *h, uint32_t n)
{
	if (!h->res_mail)
	{
		const size_t bytes = h->slab ? resident_slab_mail_bytes() : resident_mail_bytes(h->G, 16u); // sized for the finer tiling
		h->res_mail_bytes = bytes;
		HIP_TRY(hipMalloc((void **)&h->res_mail, bytes));
		HIP_TRY(hipMalloc((void **)&h->res_status, kResStatusBytes));
		HIP_TRY(hipHostMalloc((void **)&h->res_status_host, 16, hipHostMallocDefault));
		*h->res_status_host = 0;
		HIP_TRY(hipMemsetAsync(h->res_mail, 0, bytes, h->stream));
		HIP_TRY(hipMemsetAsync(h->res_status, 0, kResStatusBytes, h->stream));
		h->res_epoch = 0;
	}
	if (h->res_epoch > 0xFFFFFFFFu - n - 4u)
	{
		// the 32-bit state tags would wrap: start the numbering again from clean mailboxes
		HIP_TRY(hipMemsetAsync(h->res_mail, 0, h->res_mail_bytes, h->stream));
		h->res_epoch = 0;
	}
	return CA3D_OK;
}

// n sub-steps of a slab as ONE launch (state tiles in registers, faces through the mailboxes); the whole array is updated,
// the planes outside [n, L - n) are stale afterwards like after a per-step batch.
int resident_slab_steps(ca3d_engine *h, uint32_t n)
{
	int rc = resident_buffers(h, n);
	if (rc) return rc;
	ResidentSlabLaunch l;
	l.in = h->buf[h->cur];
	l.out = h->buf[(h->cur + n) & 1u];
	l.mail = h->res_mail;
	l.status = h->res_status;
	l.host_flag = h->res_status_host;
	l.steps = n;
	l.epoch0 = h->res_epoch;
	l.timeout_ticks = h->res_timeout_ticks;
	const int64_t zbase = (int64_t)h->z0 - (int64_t)h->ghost;
	const int64_t dead = ((-zbase) % (int64_t)h->G + (int64_t)h->G) % (int64_t)h->G; // array plane with global z == 0
	l.dead_plane = dead < (int64_t)h->nplanes ? (int)dead : -1;
	l.fn = h->res_slab_fn;
	hipError_t e = launch_resident_slab(l, h->stream);
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "resident slab kernel launch failed: %s", hipGetErrorString(e));
	h->res_epoch += n;
	h->res_check = true;
	return CA3D_OK;
}

static int resident_steps(ca3d_engine *h, uint32_t n)
{
	int rc0 = resident_buffers(h, n);
	if (rc0) return rc0;
	if (n >= 2u && !h->spare)
	{
		HIP_TRY(hipMalloc((void **)&h->spare, h->buffer_words() * sizeof(uint32_t)));
	}
	uint32_t *in = h->buf[h->cur], *other = h->buf[h->cur ^ 1u];
	ResidentLaunch l;
	l.in = in;
	// n >= 2: nothing is written to the input (see ca3d_engine::spare); n == 1: the other buffer receives the new state and
	// the input IS the state one step earlier
	l.out_last = n >= 2u ? h->spare : other;
	l.out_prev = n >= 2u ? other : in;
	l.G = h->G;
	l.mail = h->res_mail;
	l.status = h->res_status;
	l.host_flag = h->res_status_host;
	l.steps = n;
	l.epoch0 = h->res_epoch;
	l.timeout_ticks = h->res_timeout_ticks;
	l.fault_tile = h->res_fault_tile;
	h->res_fault_tile = 0;
	l.lut_s = l.lut_b = 0;
	if (!h->res_class) vn_tables(h->rules, &l.lut_s, &l.lut_b);
	l.jit_fn = h->res_jit_fn;
	const ResidentShape shape = resident_shape(h);
	l.rows = shape.rows;
	l.zsplit = shape.zsplit;
	l.pair = shape.pair;
	hipError_t e = launch_resident(l, h->stream);
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "resident kernel launch failed: %s", hipGetErrorString(e));
	h->res_pending.push_back({h->res_epoch, n, h->cur, h->step, in, other, h->spare});
	if (n >= 2u)
	{
		// rotate: buf[(cur + n) % 2] = the final state, the other one = the state one step earlier, the input becomes the spare
		if (!h->step_graphs.empty() || !h->slab_graphs.empty()) drop_graph(h); // they hold the old pointers
		const uint32_t f = (h->cur + n) & 1u;
		h->buf[f] = h->spare;
		h->buf[f ^ 1u] = other;
		h->spare = in;
	}
	h->res_epoch += n;
	return CA3D_OK;
}

// The unpacked layout's first step after an upload with cell values > 1 must be the literal kernel (raw u32 sums,
// compute.wgsl:160-174); every later state is 0 / 1. Graphs are only ever captured in the 0 / 1 regime, so a
// cached graph can never replay the wrong kernel after a new upload.
bool graphs_allowed(const ca3d_engine *h)
{
	return h->use_graph && h->stream != nullptr && !(h->layout == CA3D_LAYOUT_UNPACKED && !h->binary_state);
}

// The event pair and the figures ca3d_get_stats reports for the batch just enqueued; `planes`: G for a full grid, nz for a slab (owned
// cells only: ghost recompute is overhead).
int record_batch_stats(ca3d_engine *h, uint32_t steps, uint64_t launches, uint32_t planes)
{
	if (h->want_stats) HIP_TRY(hipEventRecord(h->ev_stop, h->stream));
	h->ev_valid = h->want_stats != 0;
	h->stats.steps = steps;
	h->stats.kernel_launches = launches;
	h->stats.cell_steps = (double)steps * h->cells_per_plane() * planes;
	h->stats.algorithmic_bytes = h->stats.cell_steps * h->bytes_per_cell_step();
	return CA3D_OK;
}

// n steps onto the stream now.
static int submit_steps(ca3d_engine *h, uint32_t n_steps)
{
	int rc = bind_device(h);
	if (rc) return rc;
	if (n_steps == 0) return CA3D_OK;
	h->buffers_exposed = false; // (ca3d_device_buffer: the pointer it handed out was valid until this call)
	if (h->want_stats) HIP_TRY(hipEventRecord(h->ev_start, h->stream));
	uint32_t left = n_steps;
	uint64_t launches = 0;
	const bool want_resident = resident_wanted(h, n_steps);
	if (!h->res_pending.empty() && (!want_resident || h->res_pending.size() >= 64u))
	{
		// Per-step kernels write the ping-pong buffers whatever happened before them — one of which is the input a recovery
		// would start from (a launch queued behind a failed one does nothing, a per-step kernel cannot know): verify the
		// resident launches still outstanding first. Also for a host that never looks at the state, so that the list stays short.
		rc = settle_resident(h);
		if (rc) return rc;
	}
	if (want_resident)
	{
		rc = resident_steps(h, n_steps);
		if (rc) return rc;
		h->step += n_steps;
		h->cur = (h->cur + n_steps) & 1u;
		launches = 1;
		left = 0;
	}
	while (left)
	{
		uint32_t n = left > kMaxGraphSteps ? kMaxGraphSteps : left;
		if (!graphs_allowed(h) && h->use_graph && h->stream != nullptr) n = 1; // non-binary unpacked state: one literal step, then graphs
		if (graphs_allowed(h) && n >= h->graph_min)
		{
			ca3d_engine::StepGraph *g = nullptr;
			rc = step_graph(h, n, h->cur, &g);
			if (rc) return rc;
			HIP_TRY(hipGraphLaunch(g->exec, h->stream));
			launches += g->launches;
		}
		else
		{
			rc = enqueue_batch(h, n, h->cur, h->stream, &launches);
			if (rc) return rc;
		}
		h->step += n;
		h->cur = (h->cur + n) & 1u;
		left -= n;
	}
	h->prev_ok = true; // every full-grid path leaves the state one step earlier in the other buffer (include/ca3d.h, ca3d_step)
	h->launches_total += launches;
	return record_batch_stats(h, n_steps, launches, h->G);
}

// queue.submit of the steps encoded so far (option "queue"). Every entry point that looks at the state, the stream or the
// options goes through here first, so a caller only ever sees the order it asked for.
int flush_queued(ca3d_engine *h)
{
	if (!h || !h->queued) return CA3D_OK;
	const uint32_t n = h->queued;
	h->queued = 0;
	return submit_steps(h, n);
}
} // namespace ca3d

using namespace ca3d;

extern "C"
{

int ca3d_step(ca3d_t *h, uint32_t n_steps) CA3D_API_TRY
{
	int rc = check_ready(h);
	if (rc) return rc;
	if (h->slab) return fail(CA3D_ERR_INVALID_ARGUMENT, "engine is a slab: use ca3d_slab_step and refresh the ghosts between batches");
	if (h->queue_max)
	{
		// encode only (the reference's commandEncoder, main_pathtraced.js:1833-1850): the steps of consecutive calls go to
		// the GPU as one submission, which lets the resident kernel run them as one launch
		if (n_steps > 0xFFFFFFFFu - h->queued) FLUSH_QUEUED(h);
		h->queued += n_steps;
		if (h->queued >= h->queue_max) return flush_queued(h);
		return CA3D_OK;
	}
	return submit_steps(h, n_steps);
}
CA3D_API_CATCH

int ca3d_flush(ca3d_t *h) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	return flush_queued(h);
}
CA3D_API_CATCH

} // extern "C"
