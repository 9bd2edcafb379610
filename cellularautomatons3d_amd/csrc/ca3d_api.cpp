// C-ABI layer (include/ca3d.h): the engine object's lifecycle, the error slot, state in and out, streams, summaries, the info / stats
// getters and the options. Stepping is ca3d_step.cpp, slabs and their transport ca3d_slab.cpp, the renderer ca3d_render.cpp.
// Replaces the WebGPU calls of main_pathtraced.js listed per entry point in the header. No CPU fallback.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <stdexcept>

#include "ca3d_engine.h"

namespace
{
// the message slot of ca3d_last_error(): a fixed buffer per thread — setting it never allocates, so it can be set while reporting
// std::bad_alloc (a std::string here could throw from inside the handler that reports the failure)
thread_local char g_last_error[1024] = "";
} // namespace

namespace ca3d
{
void set_last_error(const char *msg) noexcept
{
	if (!msg) msg = "";
	size_t n = strlen(msg);
	if (n >= sizeof g_last_error) n = sizeof g_last_error - 1;
	memmove(g_last_error, msg, n); // (msg may point into the slot itself)
	g_last_error[n] = 0;
}

int fail(int code, const char *fmt, ...)
{
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	set_last_error(buf);
	return code;
}

// Every entry point of include/ca3d.h is a function-try-block (CA3D_API_TRY ... CA3D_API_CATCH, ca3d_internal.h) whose handler lands
// here: the header promises status codes, and an exception leaving an extern "C" function called from Node.js / ctypes ends the
// process. What can throw inside the library is host allocation (std::string / std::vector / std::map in the rule canonicaliser,
// the run-time compiler, the group) and whatever the standard library reports as std::exception.
int exception_to_status() noexcept
{
	try
	{
		throw;
	}
	catch (const std::bad_alloc &)
	{
		set_last_error("out of host memory (std::bad_alloc inside the library)");
		return CA3D_ERR_OUT_OF_MEMORY;
	}
	catch (const std::exception &e)
	{
		char buf[1024];
		snprintf(buf, sizeof buf, "internal error: %s", e.what());
		set_last_error(buf);
		return CA3D_ERR_DEVICE;
	}
	catch (...)
	{
		set_last_error("internal error: unknown C++ exception inside the library");
		return CA3D_ERR_DEVICE;
	}
}

void drop_graph(ca3d_engine *h)
{
	for (auto &kv : h->step_graphs) hipGraphExecDestroy(kv.second.exec);
	h->step_graphs.clear();
	for (auto &kv : h->slab_graphs) hipGraphExecDestroy(kv.second);
	h->slab_graphs.clear();
}

static void free_resident(ca3d_engine *h)
{
	if (h->res_mail) hipFree(h->res_mail);
	if (h->res_status) hipFree(h->res_status);
	if (h->res_status_host) hipHostFree(h->res_status_host);
	h->res_mail = nullptr;
	h->res_status = h->res_status_host = nullptr;
	h->res_epoch = 0;
	h->res_check = false;
	h->res_failed = false;
	h->res_pending.clear();
	h->res_note.clear();
}

static void free_buffers(ca3d_engine *h)
{
	drop_graph(h);
	free_resident(h);
	if (h->spare) hipFree(h->spare);
	h->spare = nullptr;
	for (int i = 0; i < 2; i++)
	{
		if (h->buf[i]) hipFree(h->buf[i]);
		h->buf[i] = nullptr;
	}
	h->configured = false;
	h->has_state = false;
	h->step = 0;
	h->cur = 0;
	h->pending_edges = 0; // an edge phase belongs to the state that has just gone
	h->ghosts_valid = false;
	h->prev_ok = false;
	if (h->sum_dev) hipFree(h->sum_dev);
	if (h->sum_host) hipHostFree(h->sum_host);
	h->sum_dev = h->sum_host = nullptr;
	h->sum_words = 0;
	h->sum_ev_valid = false;
	if (h->cycle_anchor) hipFree(h->cycle_anchor);
	h->cycle_anchor = nullptr;
}

int bind_device(ca3d_engine *h, bool join)
{
	HIP_TRY(hipSetDevice(h->device));
	if (join) h->main_touched = h->state_touched = true; // (whatever the caller is about to put on the engine's stream: the next pipelined frame waits for it)
	if (join)
		for (auto &L : h->lanes)
			if (L.pending) return join_frames(h);
	return CA3D_OK;
}

static int allocate(ca3d_engine *h)
{
	const size_t bytes = h->buffer_words() * sizeof(uint32_t);
	for (int i = 0; i < 2; i++)
	{
		hipError_t e = hipMalloc((void **)&h->buf[i], bytes);
		if (e != hipSuccess)
		{
			free_buffers(h);
			return fail(CA3D_ERR_OUT_OF_MEMORY, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
		}
	}
	HIP_TRY(hipMemsetAsync(h->buf[0], 0, bytes, h->stream));
	HIP_TRY(hipMemsetAsync(h->buf[1], 0, bytes, h->stream));
	h->configured = true;
	return CA3D_OK;
}

int check_ready(ca3d_engine *h)
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!h->configured) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_configure has not been called");
	if (!h->rules.valid) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_set_rules has not been called");
	if (!h->has_state) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_upload_state has not been called");
	return CA3D_OK;
}

// "State edited": what holds of an engine whose CURRENT buffer has just been written by something other than a step, on the engine's
// stream (ca3d_stamp_windows edits it in place; the caller has bound the device, joined the frames in flight, submitted the queued steps
// and settled a resident launch). The step counter and the buffers stay; the other buffer no longer holds the state one step earlier, and
// what the renderer derived from the state is stale.
void engine_state_edited(ca3d_engine *h)
{
	h->prev_ok = false;
	h->state_serial++;
}

// The "state replaced" tail of ca3d_upload_state and ca3d_seed_state: what holds of an engine whose two ping-pong buffers have just been
// given the same new words (on the engine's stream; the caller has bound the device, joined the frames in flight and dropped the queued
// steps). A resident launch whose completion has not been looked at must have left the stream before this is called.
static int state_replaced(ca3d_engine *h)
{
	h->step = 0;
	h->cur = 0;
	engine_state_edited(h);
	h->buffers_exposed = false;
	h->pending_edges = 0; // a restart between the two phases of a batch abandons the batch
	h->ghosts_valid = false;
	h->res_pending.clear(); // their results have just been overwritten
	if (h->res_status_host && *h->res_status_host)
	{
		// a resident launch gave up earlier: clean mailboxes and status for whoever turns the path on again
		HIP_TRY(hipMemsetAsync(h->res_mail, 0, h->res_mail_bytes, h->stream));
		HIP_TRY(hipMemsetAsync(h->res_status, 0, kResStatusBytes, h->stream));
		h->res_status_host[0] = h->res_status_host[1] = 0;
		h->res_epoch = 0;
		h->res_check = false;
		h->res_failed = true;
	}
	h->has_state = true;
	return CA3D_OK;
}

// ca3d_seed's refusals, decided once for engines, groups and ensembles
const char *seed_spec_error(const ca3d_seed &s, uint32_t G)
{
	if (s.and_rounds > 31u) return "and_rounds must be in [0, 31]";
	for (int i = 0; i < 3; i++)
	{
		if (s.box_min[i] > s.box_max[i]) return "box_min exceeds box_max";
		if (s.box_max[i] >= G) return "box_max lies outside the grid";
	}
	return nullptr;
}

// ca3d_set_stream / ca3d_use_own_stream: everything of the old stream is waited for and verified, what was built for it is dropped
static int switch_stream(ca3d_engine *h, hipStream_t s)
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	FLUSH_QUEUED(h);
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(h->stream));
	rc = check_resident(h);
	if (rc) return rc;
	resident_stream_retired(h->stream);
	drop_graph(h);
	h->stream = s;
	h->ev_valid = false;
	refresh_kernels(h); // the new stream may be confined to fewer CUs (CU mask): residency is checked per stream
	return CA3D_OK;
}
} // namespace ca3d

using namespace ca3d;

extern "C"
{

int ca3d_abi_version(void) { return CA3D_ABI_VERSION; }

const char *ca3d_last_error(void) { return g_last_error; }

// Test hook: throws inside a guarded body so that the exception boundary itself can be exercised without a GPU.
// kind 0: std::bad_alloc, 1: std::runtime_error, 2: a non-std exception, 3: a real allocation failure (a vector of SIZE_MAX / 2 bytes)
int ca3d_selftest_exception(int kind) CA3D_API_TRY
{
	if (kind == 0) throw std::bad_alloc();
	if (kind == 1) throw std::runtime_error("selftest");
	if (kind == 2) throw 42;
	if (kind == 3)
	{
		std::vector<char> v;
		v.resize(v.max_size() / 2u); // std::length_error or std::bad_alloc, whichever the allocator reports
		return fail(CA3D_ERR_DEVICE, "selftest: the allocation of %zu bytes succeeded", v.size());
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_device_count(int *out_count) CA3D_API_TRY
{
	if (!out_count) return fail(CA3D_ERR_INVALID_ARGUMENT, "out_count is NULL");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) { *out_count = 0; return fail(CA3D_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
	*out_count = n;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_create(int device, ca3d_t **out) CA3D_API_TRY
{
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0)
		return fail(CA3D_ERR_DEVICE, "no HIP device available (%s); this engine has no CPU fallback",
		            e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
	if (device < 0 || device >= n) return fail(CA3D_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, n);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(CA3D_ERR_UNSUPPORTED, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
	ca3d_engine *h = new (std::nothrow) ca3d_engine();
	if (!h) return fail(CA3D_ERR_OUT_OF_MEMORY, "out of host memory");
	h->device = device;
	hipError_t err = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
	if (err == hipSuccess) err = hipEventCreate(&h->ev_start);
	if (err == hipSuccess) err = hipEventCreate(&h->ev_stop);
	if (err == hipSuccess) err = hipEventCreate(&h->rev_start);
	if (err == hipSuccess) err = hipEventCreate(&h->rev_stop);
	if (err != hipSuccess)
	{
		ca3d_destroy(h); // releases whatever was created
		return fail(CA3D_ERR_DEVICE, "engine set-up failed: %s", hipGetErrorString(err));
	}
	h->stream = h->own_stream;
	*out = h;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_destroy(ca3d_t *h) CA3D_API_TRY
{
	if (!h) return CA3D_OK;
	hipSetDevice(h->device);
	h->queued = 0; // never submitted: the state goes away with the engine
	if (h->stream || h->own_stream) hipStreamSynchronize(h->stream);
	for (auto &L : h->lanes)
		if (L.s) hipStreamSynchronize(L.s); // frames in flight read the state
	resident_stream_retired(h->stream);
	free_buffers(h);
	free_render_targets(h);
	free_slab_comm(h);
	if (h->r_counters) hipFree(h->r_counters);
	if (h->r_occ) hipFree(h->r_occ);
	if (h->r_stream) hipFree(h->r_stream);
	if (h->r_bricks) hipFree(h->r_bricks);
	for (auto &L : h->lanes)
	{
		if (L.s) { hipStreamSynchronize(L.s); hipStreamDestroy(L.s); }
		for (hipEvent_t e : {L.start, L.stop, L.done})
			if (e) hipEventDestroy(e);
		if (L.scratch) hipFree(L.scratch);
		if (L.counters) hipFree(L.counters);
	}
	for (hipStream_t sp : h->lane_spares) hipStreamDestroy(sp);
	if (h->ev_state) hipEventDestroy(h->ev_state);
	if (h->r_aux) hipStreamDestroy(h->r_aux);
	if (h->r_fork) hipEventDestroy(h->r_fork);
	if (h->r_join) hipEventDestroy(h->r_join);
	if (h->rev_start) hipEventDestroy(h->rev_start);
	if (h->rev_stop) hipEventDestroy(h->rev_stop);
	if (h->ev_start) hipEventDestroy(h->ev_start);
	if (h->ev_stop) hipEventDestroy(h->ev_stop);
	if (h->sum_ev0) hipEventDestroy(h->sum_ev0);
	if (h->sum_ev1) hipEventDestroy(h->sum_ev1);
	if (h->own_stream) hipStreamDestroy(h->own_stream);
	delete h;
	return CA3D_OK;
}
CA3D_API_CATCH

static int configure_common(ca3d_t *h, uint32_t g, int layout)
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (layout != CA3D_LAYOUT_PACKED32 && layout != CA3D_LAYOUT_UNPACKED) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown layout %d", layout);
	if (g == 0) return fail(CA3D_ERR_INVALID_ARGUMENT, "grid size must be positive");
	if (layout == CA3D_LAYOUT_PACKED32 && (g % 32u)) return fail(CA3D_ERR_INVALID_ARGUMENT, "packed layout needs a grid size that is a multiple of 32 (got %u)", g);
	if (layout == CA3D_LAYOUT_UNPACKED && (g % 4u)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unpacked layout needs a grid size that is a multiple of 4 (got %u)", g);
	if (g > 8192u) return fail(CA3D_ERR_UNSUPPORTED, "grid size %u exceeds the supported maximum 8192", g);
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(h->stream));
	free_buffers(h);
	h->buffers_exposed = false;
	h->G = g;
	h->layout = layout;
	h->plane_words = layout == CA3D_LAYOUT_PACKED32 ? (size_t)(g / 32u) * g : (size_t)g * g;
	return CA3D_OK;
}

int ca3d_configure(ca3d_t *h, uint32_t gx, uint32_t gy, uint32_t gz, int layout) CA3D_API_TRY
{
	if (gx != gy || gy != gz) return fail(CA3D_ERR_UNSUPPORTED, "only cubic grids exist in the reference (got %ux%ux%u)", gx, gy, gz);
	if (h) h->queued = 0; // steps of a state that is being thrown away
	int rc = configure_common(h, gx, layout);
	if (rc) return rc;
	h->slab = false;
	h->z0 = 0;
	h->nz = gx;
	h->ghost = 0;
	h->nplanes = gx;
	rc = allocate(h);
	if (rc == CA3D_OK) refresh_kernels(h);
	return rc;
}
CA3D_API_CATCH

int ca3d_configure_slab(ca3d_t *h, uint32_t g, int layout, uint32_t z0, uint32_t nz, uint32_t ghost) CA3D_API_TRY
{
	if (h) h->queued = 0;
	int rc = configure_common(h, g, layout);
	if (rc) return rc;
	if (nz == 0 || z0 + nz > g) return fail(CA3D_ERR_INVALID_ARGUMENT, "slab [%u, %u) is outside the grid of %u planes", z0, z0 + nz, g);
	if (ghost == 0 || ghost > nz) return fail(CA3D_ERR_INVALID_ARGUMENT, "ghost depth must be in [1, nz] (got %u, nz %u)", ghost, nz);
	if (layout == CA3D_LAYOUT_UNPACKED && (g & (g - 1u))) return fail(CA3D_ERR_UNSUPPORTED, "unpacked slabs need a power-of-two grid size: the legacy kernel's -1 wrap is a torus only then");
	h->slab = true;
	h->z0 = z0;
	h->nz = nz;
	h->ghost = ghost;
	h->nplanes = nz + 2u * ghost;
	rc = allocate(h);
	if (rc == CA3D_OK) refresh_kernels(h);
	return rc;
}
CA3D_API_CATCH

int ca3d_set_rules(ca3d_t *h, const int32_t *main_offsets, uint32_t n_main, const int32_t *edges_offsets, uint32_t n_edges,
                   const int32_t *corners_offsets, uint32_t n_corners, const uint32_t survive[CA3D_LUT_LEN],
                   const uint32_t born[CA3D_LUT_LEN]) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	FLUSH_QUEUED(h); // the steps encoded so far run under the rules they were encoded with
	if (int rcs = settle_resident(h)) return rcs; // ... and a recovery re-runs them under those rules too
	CanonRules r;
	std::string err;
	int rc = canonicalize_rules(main_offsets, n_main, edges_offsets, n_edges, corners_offsets, n_corners, survive, born, &r, &err);
	if (rc) return fail(rc, "%s", err.c_str());
	rc = bind_device(h);
	if (rc) return rc;
	drop_graph(h);
	h->rules = r;
	refresh_kernels(h);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_upload_state(ca3d_t *h, const uint32_t *words, size_t n_words) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!h->configured) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_configure has not been called");
	if (!words) return fail(CA3D_ERR_INVALID_ARGUMENT, "words is NULL");
	h->queued = 0; // the state they would have produced is overwritten
	if (n_words != h->state_words()) return fail(CA3D_ERR_INVALID_ARGUMENT, "state has %zu words, expected %zu", n_words, h->state_words());
	int rc = bind_device(h);
	if (rc) return rc;
	const size_t off = h->slab ? (size_t)h->ghost * h->plane_words : 0;
	const size_t bytes = n_words * sizeof(uint32_t);
	// Same data into both ping-pong buffers (main_pathtraced.js:1361-1362); ghosts are cleared.
	if (h->slab)
	{
		HIP_TRY(hipMemsetAsync(h->buf[0], 0, h->buffer_words() * sizeof(uint32_t), h->stream));
		HIP_TRY(hipMemsetAsync(h->buf[1], 0, h->buffer_words() * sizeof(uint32_t), h->stream));
	}
	HIP_TRY(hipMemcpyAsync(h->buf[0] + off, words, bytes, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipMemcpyAsync(h->buf[1] + off, h->buf[0] + off, bytes, hipMemcpyDeviceToDevice, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	rc = state_replaced(h);
	if (rc) return rc;
	h->binary_state = false;
	if (h->layout == CA3D_LAYOUT_UNPACKED)
	{
		bool bin = true;
		for (size_t i = 0; i < n_words && bin; i++) bin = words[i] <= 1u;
		h->binary_state = bin;
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_seed_state(ca3d_t *h, const ca3d_seed *spec) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!spec) return fail(CA3D_ERR_INVALID_ARGUMENT, "spec is NULL");
	if (!h->configured) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_configure has not been called");
	if (const char *why = seed_spec_error(*spec, h->G))
		return fail(CA3D_ERR_INVALID_ARGUMENT, "seed spec for a grid of %u: %s (box (%u, %u, %u) .. (%u, %u, %u), and_rounds %u)", h->G, why, spec->box_min[0],
		            spec->box_min[1], spec->box_min[2], spec->box_max[0], spec->box_max[1], spec->box_max[2], spec->and_rounds);
	h->queued = 0; // the state they would have produced is overwritten
	int rc = bind_device(h);
	if (rc) return rc;
	// a resident launch nobody has looked at yet: its verdict must not arrive after the state it belonged to has gone (the upload's wait)
	if (!h->res_pending.empty() || h->res_check) HIP_TRY(hipStreamSynchronize(h->stream));
	SeedLaunch l;
	l.buf0 = h->buf[0]; l.buf1 = h->buf[1];
	l.G = h->G;
	l.layout = h->layout;
	l.z0 = h->z0; l.nz = h->nz; l.ghost = h->slab ? h->ghost : 0u;
	l.spec = *spec;
	hipError_t e = launch_seed(l, h->stream); // both buffers, ghost planes zeroed, in one pass
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "seed kernel launch failed: %s", hipGetErrorString(e));
	rc = state_replaced(h);
	if (rc) return rc;
	h->binary_state = true; // unpacked: every cell is 0 or 1
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_read_state(ca3d_t *h, uint32_t *words, size_t n_words) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!h->configured || !h->has_state) return fail(CA3D_ERR_NOT_CONFIGURED, "no state to read: configure and upload first");
	if (!words) return fail(CA3D_ERR_INVALID_ARGUMENT, "words is NULL");
	FLUSH_QUEUED(h);
	if (n_words != h->state_words()) return fail(CA3D_ERR_INVALID_ARGUMENT, "state has %zu words, expected %zu", n_words, h->state_words());
	int rc = bind_device(h);
	if (rc) return rc;
	rc = settle_resident(h); // a resident launch that gave up is recovered from before the state is looked at
	if (rc) return rc;
	const size_t off = h->slab ? (size_t)h->ghost * h->plane_words : 0;
	HIP_TRY(hipMemcpyAsync(words, h->buf[h->cur] + off, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_synchronize(ca3d_t *h) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	FLUSH_QUEUED(h);
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(h->stream));
	return check_resident(h);
}
CA3D_API_CATCH

int ca3d_measure_copy(ca3d_t *h, size_t n_bytes, uint32_t reps, double *gb_per_s) CA3D_API_TRY
{
	if (!h || !gb_per_s) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (n_bytes < (1u << 20) || n_bytes % 16u || reps == 0 || reps > 4096u) return fail(CA3D_ERR_INVALID_ARGUMENT, "n_bytes must be a multiple of 16 of at least 1 MiB, reps in [1, 4096]");
	FLUSH_QUEUED(h);
	int rc = bind_device(h);
	if (rc) return rc;
	void *a = nullptr, *b = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	auto cleanup = [&]() { if (a) hipFree(a); if (b) hipFree(b); if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); };
#define COPY_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail(e_ == hipErrorOutOfMemory ? CA3D_ERR_OUT_OF_MEMORY : CA3D_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } } while (0)
	COPY_TRY(hipMalloc(&a, n_bytes));
	COPY_TRY(hipMalloc(&b, n_bytes));
	COPY_TRY(hipEventCreate(&e0));
	COPY_TRY(hipEventCreate(&e1));
	COPY_TRY(hipMemsetAsync(a, 0x5A, n_bytes, h->stream));
	COPY_TRY(launch_copy_f4(a, b, n_bytes, h->stream)); // warm: page tables, clocks
	COPY_TRY(hipEventRecord(e0, h->stream));
	for (uint32_t i = 0; i < reps; i++) COPY_TRY(launch_copy_f4((i & 1u) ? b : a, (i & 1u) ? a : b, n_bytes, h->stream));
	COPY_TRY(hipEventRecord(e1, h->stream));
	COPY_TRY(hipEventSynchronize(e1));
	float ms = 0.f;
	COPY_TRY(hipEventElapsedTime(&ms, e0, e1));
#undef COPY_TRY
	cleanup();
	*gb_per_s = ms > 0.f ? 2.0 * (double)n_bytes * reps / (ms * 1e-3) / 1e9 : 0.0; // bytes read + bytes written
	return CA3D_OK;
}
CA3D_API_CATCH

} // extern "C"

// The summary of the current state onto the engine's stream and back: clear of the result block, ONE kernel (ca_summary.hip), one
// small copy into pinned memory, one wait. The entry guard is ca3d_read_state's.
static int summarize_state(ca3d_engine *h, ca3d_summary *out, uint32_t *plane_population)
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	if (!h->configured || !h->has_state) return fail(CA3D_ERR_NOT_CONFIGURED, "no state to summarise: configure and upload first");
	// the edge phase of a slab batch ping-pongs its zones through BOTH buffers: until the interior phase commits the batch neither holds a state
	if (h->pending_edges) return fail(CA3D_ERR_INVALID_ARGUMENT, "an edge phase is pending: finish it with the interior phase");
	FLUSH_QUEUED(h);
	int rc = bind_device(h);
	if (rc) return rc;
	rc = settle_resident(h); // a resident launch that gave up is recovered from before the state is looked at
	if (rc) return rc;
	const size_t words = kSummaryHeaderWords + (size_t)h->nz;
	if (h->sum_words < words)
	{
		HIP_TRY(hipStreamSynchronize(h->stream));
		if (h->sum_dev) hipFree(h->sum_dev);
		if (h->sum_host) hipHostFree(h->sum_host);
		h->sum_dev = h->sum_host = nullptr;
		h->sum_words = 0;
		HIP_TRY(hipMalloc((void **)&h->sum_dev, words * sizeof(uint32_t)));
		HIP_TRY(hipHostMalloc((void **)&h->sum_host, words * sizeof(uint32_t), hipHostMallocDefault));
		h->sum_words = words;
	}
	if (h->want_stats && !h->sum_ev0)
	{
		HIP_TRY(hipEventCreate(&h->sum_ev0));
		HIP_TRY(hipEventCreate(&h->sum_ev1));
	}
	const bool has_prev = h->step >= 1 && h->prev_ok;
	const size_t off = h->slab ? (size_t)h->ghost * h->plane_words : 0;
	SummaryLaunch l;
	l.cur = h->buf[h->cur] + off;
	l.prev = has_prev ? h->buf[h->cur ^ 1u] + off : nullptr;
	l.result = h->sum_dev;
	l.G = h->G;
	l.layout = h->layout;
	l.z0 = h->z0;
	l.nz = h->nz;
	h->sum_ev_valid = false;
	if (h->want_stats) HIP_TRY(hipEventRecord(h->sum_ev0, h->stream));
	HIP_TRY(hipMemsetAsync(h->sum_dev, 0, words * sizeof(uint32_t), h->stream));
	hipError_t e = launch_summary(l, h->stream);
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "summary kernel launch failed: %s", hipGetErrorString(e));
	if (h->want_stats) HIP_TRY(hipEventRecord(h->sum_ev1, h->stream));
	HIP_TRY(hipMemcpyAsync(h->sum_host, h->sum_dev, (plane_population ? words : (size_t)kSummaryHeaderWords) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	h->sum_ev_valid = h->want_stats != 0;
	const uint32_t *r = h->sum_host;
	uint64_t r64[4];
	memcpy(r64, r, sizeof r64);
	memset(out, 0, sizeof *out);
	out->step = h->step;
	out->population = r64[0];
	out->births = has_prev ? r64[1] : 0;
	out->deaths = has_prev ? r64[2] : 0;
	out->digest = r64[3];
	out->has_previous = has_prev ? 1u : 0u;
	for (int i = 0; i < 3; i++)
	{
		out->box_min[i] = r64[0] ? ~r[8 + i] : h->G;
		out->box_max[i] = r64[0] ? r[11 + i] : 0u;
	}
	if (plane_population) memcpy(plane_population, r + kSummaryHeaderWords, (size_t)h->nz * sizeof(uint32_t));
	return CA3D_OK;
}

extern "C"
{

int ca3d_summarize(ca3d_t *h, ca3d_summary *out, uint32_t *plane_population) CA3D_API_TRY
{
	return summarize_state(h, out, plane_population);
}
CA3D_API_CATCH

int ca3d_get_summary_time(ca3d_t *h, double *gpu_ms) CA3D_API_TRY
{
	if (!h || !gpu_ms) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	*gpu_ms = 0.0;
	if (!h->sum_ev_valid) return CA3D_OK;
	int rc = bind_device(h);
	if (rc) return rc;
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, h->sum_ev0, h->sum_ev1));
	*gpu_ms = ms;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_step_until(ca3d_t *h, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, ca3d_summary *out, uint32_t *steps_done,
                    uint32_t *reason) CA3D_API_TRY
{
	if (steps_done) *steps_done = 0;
	if (reason) *reason = 0;
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	if (check_every == 0) return fail(CA3D_ERR_INVALID_ARGUMENT, "check_every must be at least 1");
	if (stop_mask & ~(uint32_t)(CA3D_STOP_EXTINCT | CA3D_STOP_STILL)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in stop_mask %#x", stop_mask);
	if (h->configured && h->slab) return fail(CA3D_ERR_UNSUPPORTED, "ca3d_step_until takes a full-grid engine: a slab's neighbours must step with it");
	int rc = check_ready(h);
	if (rc) return rc;
	uint32_t done = 0;
	for (;;)
	{
		rc = summarize_state(h, out, nullptr);
		if (rc) return rc;
		uint32_t fired = 0;
		if (out->population == 0) fired |= CA3D_STOP_EXTINCT;
		if (out->has_previous && out->births + out->deaths == 0) fired |= CA3D_STOP_STILL;
		fired &= stop_mask;
		if (fired || done == max_steps)
		{
			if (steps_done) *steps_done = done;
			if (reason) *reason = fired;
			return CA3D_OK;
		}
		const uint32_t n = max_steps - done < check_every ? max_steps - done : check_every;
		rc = ca3d_step(h, n); // the very path of a caller's ca3d_step(n): queue, resident kernels, captured graphs
		if (rc) return rc;
		done += n;
	}
}
CA3D_API_CATCH

} // extern "C"

// Is the current state (just summarised: the stream is idle, resident launches are settled) word for word the anchor? One compare kernel
// (ca_summary.hip); its flag word is the summary block's unused header word 14 and comes back through the pinned copy.
static int state_is_anchor(ca3d_engine *h, bool *same)
{
	uint32_t *flag = h->sum_dev + 14;
	HIP_TRY(hipMemsetAsync(flag, 0, sizeof(uint32_t), h->stream));
	hipError_t e = launch_state_equal(h->buf[h->cur], h->cycle_anchor, h->state_words(), flag, h->stream);
	if (e != hipSuccess) return fail(CA3D_ERR_DEVICE, "compare kernel launch failed: %s", hipGetErrorString(e));
	HIP_TRY(hipMemcpyAsync(h->sum_host + 14, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	*same = h->sum_host[14] == 0u;
	return CA3D_OK;
}

extern "C"
{

int ca3d_step_until_cycle(ca3d_t *h, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, ca3d_summary *out, uint32_t *steps_done,
                          uint32_t *reason, uint32_t *period) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (steps_done) *steps_done = 0;
	if (reason) *reason = 0;
	if (period) *period = 0;
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	if (check_every == 0) return fail(CA3D_ERR_INVALID_ARGUMENT, "check_every must be at least 1");
	if (stop_mask & ~(uint32_t)(CA3D_STOP_EXTINCT | CA3D_STOP_STILL | CA3D_STOP_PERIODIC)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in stop_mask %#x", stop_mask);
	if (h->configured && h->slab) return fail(CA3D_ERR_UNSUPPORTED, "ca3d_step_until_cycle takes a full-grid engine: a slab's neighbours must step with it");
	int rc = check_ready(h);
	if (rc) return rc;
	// ca3d_step_until's loop with an anchor on Brent's schedule (include/ca3d.h). The summary's digest is the filter: equal states have
	// equal digests and populations, so anything else proves a difference; a stop is only declared by the compare kernel.
	uint32_t done = 0, j = 0, anchor_step = 0;
	uint64_t anchor_digest = 0, anchor_population = 0;
	for (;;)
	{
		rc = summarize_state(h, out, nullptr);
		if (rc) return rc;
		uint32_t fired = 0;
		if (out->population == 0) fired |= CA3D_STOP_EXTINCT;
		if (out->has_previous && out->births + out->deaths == 0) fired |= CA3D_STOP_STILL;
		if (j > 0 && (stop_mask & CA3D_STOP_PERIODIC) && out->digest == anchor_digest && out->population == anchor_population)
		{
			bool same = false;
			rc = state_is_anchor(h, &same);
			if (rc) return rc;
			if (same) fired |= CA3D_STOP_PERIODIC;
		}
		fired &= stop_mask;
		if (fired || done == max_steps)
		{
			if (steps_done) *steps_done = done;
			if (reason) *reason = fired;
			if (period && (fired & CA3D_STOP_PERIODIC)) *period = done - anchor_step;
			return CA3D_OK;
		}
		if ((stop_mask & CA3D_STOP_PERIODIC) && (j & (j - 1u)) == 0u) // check points 0, 1, 2, 4, 8 ...: the anchor moves, AFTER the comparison
		{
			const size_t bytes = h->state_words() * sizeof(uint32_t);
			if (!h->cycle_anchor) HIP_TRY(hipMalloc((void **)&h->cycle_anchor, bytes));
			// the CURRENT buffer (resident launches rotate three): summarize_state settled them and left the stream idle
			HIP_TRY(hipMemcpyAsync(h->cycle_anchor, h->buf[h->cur], bytes, hipMemcpyDeviceToDevice, h->stream));
			anchor_step = done;
			anchor_digest = out->digest;
			anchor_population = out->population;
		}
		const uint32_t n = max_steps - done < check_every ? max_steps - done : check_every;
		rc = ca3d_step(h, n); // the very path of a caller's ca3d_step(n): queue, resident kernels, captured graphs
		if (rc) return rc;
		done += n;
		j++;
	}
}
CA3D_API_CATCH

int ca3d_recovered_launches(ca3d_t *h, uint32_t *out_count) CA3D_API_TRY
{
	if (!h || !out_count) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	*out_count = h->res_recovered;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_set_stream(ca3d_t *h, void *hip_stream) CA3D_API_TRY
{
	return switch_stream(h, (hipStream_t)hip_stream);
}
CA3D_API_CATCH

int ca3d_use_own_stream(ca3d_t *h) CA3D_API_TRY
{
	return switch_stream(h, h ? h->own_stream : nullptr);
}
CA3D_API_CATCH

int ca3d_device_buffer(ca3d_t *h, int which, void **device_ptr, size_t *n_bytes) CA3D_API_TRY
{
	if (!h || !device_ptr || !n_bytes) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!h->configured) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_configure has not been called");
	if (which != 0 && which != 1) return fail(CA3D_ERR_INVALID_ARGUMENT, "buffer index must be 0 or 1");
	FLUSH_QUEUED(h);
	if (int rcs = settle_resident(h)) return rcs;
	*device_ptr = h->buf[which];
	*n_bytes = h->buffer_words() * sizeof(uint32_t);
	h->prev_ok = false; // (... nor does ca3d_summarize compare buffers the caller may have written: has_previous stays 0 until the next step)
	h->state_serial++; // the caller may write through the pointer: what the renderer derived from the state is stale from here on,
	h->buffers_exposed = true; // and again before every frame while the pointer is valid (ca3d_render)
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_info(ca3d_t *h, ca3d_info *out) CA3D_API_TRY
{
	if (!h || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	FLUSH_QUEUED(h);
	memset(out, 0, sizeof *out);
	out->grid_size = h->G;
	out->layout = h->layout;
	out->z0 = h->z0;
	out->nz = h->nz;
	out->ghost = h->ghost;
	out->step = h->step;
	out->state_words = h->configured ? h->state_words() : 0;
	out->current_buffer = (int32_t)h->cur;
	out->device = h->device;
	out->launches_total = h->launches_total;
	reported_kernel_name(h, out->kernel_name, sizeof out->kernel_name);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_jit_log(ca3d_t *h, char *buf, size_t n_bytes, size_t *needed) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (needed) *needed = h->jit_log.size() + 1;
	if (buf && n_bytes)
	{
		const size_t n = h->jit_log.size() < n_bytes - 1 ? h->jit_log.size() : n_bytes - 1;
		memcpy(buf, h->jit_log.data(), n);
		buf[n] = '\0';
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_jit_stats(ca3d_jit_stats *out) CA3D_API_TRY
{
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	jit_stats(out);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_kernel_variant(ca3d_t *h, char *buf, size_t n_bytes, size_t *needed) CA3D_API_TRY
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	ca3d_info info;
	int rc = ca3d_get_info(h, &info);
	if (rc) return rc;
	uint64_t rh = 1469598103934665603ull;
	auto mix = [&](const void *p, size_t n) { for (size_t i = 0; i < n; i++) { rh ^= static_cast<const unsigned char *>(p)[i]; rh *= 1099511628211ull; } };
	if (h->rules.valid)
	{
		mix(&h->rules.lists, sizeof h->rules.lists);
		mix(h->rules.survive_raw, sizeof h->rules.survive_raw);
		mix(h->rules.born_raw, sizeof h->rules.born_raw);
	}
	const char *zs = getenv("CA3D_RC256_ZS");
	char text[320];
	const bool res = !strncmp(info.kernel_name, "ca_resident", 11);
	const ResidentShape shape = resident_shape(h);
	if (res)
		snprintf(text, sizeof text, "%s;G=%u;rule=%016llx;rows=%u;zsplit=%u;pair=%d;rc256zs=%s;src=%016llx", info.kernel_name, h->G, (unsigned long long)rh,
		         shape.rows, shape.zsplit, shape.pair, zs ? zs : "-", (unsigned long long)jit_sources_hash());
	else
		snprintf(text, sizeof text, "%s;G=%u;rule=%016llx;variant=%d;src=%016llx", info.kernel_name, h->G, (unsigned long long)rh, h->variant, (unsigned long long)jit_sources_hash());
	const size_t len = strlen(text);
	if (needed) *needed = len + 1;
	if (buf && n_bytes)
	{
		const size_t n = len < n_bytes - 1 ? len : n_bytes - 1;
		memcpy(buf, text, n);
		buf[n] = '\0';
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_get_stats(ca3d_t *h, ca3d_stats *out) CA3D_API_TRY
{
	if (!h || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	FLUSH_QUEUED(h);
	if (!h->ev_valid) return fail(CA3D_ERR_NOT_CONFIGURED, "no step batch has been timed yet (or option \"stats\" is 0)");
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipEventSynchronize(h->ev_stop));
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, h->ev_start, h->ev_stop));
	h->stats.gpu_ms = ms;
	*out = h->stats;
	HIP_TRY(hipStreamSynchronize(h->stream));
	return check_resident(h);
}
CA3D_API_CATCH

int ca3d_set_option(ca3d_t *h, const char *name, int64_t value) CA3D_API_TRY
{
	if (!h || !name) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	FLUSH_QUEUED(h); // options apply to the steps encoded after them
	if (strcmp(name, "queue") && strcmp(name, "stats"))
		if (int rcs = settle_resident(h)) return rcs; // ... and a recovery re-runs steps under the options they were issued with
	if (!strcmp(name, "resident_fault_tile"))
	{
		// diagnostics: tile `value - 1` of the NEXT resident launch leaves at once, as a workgroup that never became resident
		// would; its neighbours time out and the engine recovers (tests/test_gpu_ca_parity.py)
		if (value < 0 || value > 1024) return fail(CA3D_ERR_INVALID_ARGUMENT, "resident_fault_tile must be in [0, 1024]");
		h->res_fault_tile = (uint32_t)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "queue"))
	{
		if (value < 0 || value > 1000000) return fail(CA3D_ERR_INVALID_ARGUMENT, "queue must be in [0, 1000000] steps");
		h->queue_max = (uint32_t)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "graph")) { h->use_graph = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "graph_prepare"))
	{
		// capture and instantiate, now, the graphs a later ca3d_step(value) replays (otherwise built on first use)
		int rc = check_ready(h);
		if (rc) return rc;
		rc = bind_device(h);
		if (rc) return rc;
		if (!graphs_allowed(h) || h->slab || value <= 0) return CA3D_OK;
		// the batches ca3d_step(value) will replay, from either buffer (an odd batch length alternates)
		uint64_t left = (uint64_t)value;
		uint32_t cur = h->cur;
		for (int pass = 0; pass < 2; pass++)
		{
			for (uint64_t l = left; l;)
			{
				const uint32_t n = l > kMaxGraphSteps ? kMaxGraphSteps : (uint32_t)l;
				if (n >= h->graph_min)
				{
					ca3d_engine::StepGraph *g = nullptr;
					rc = step_graph(h, n, cur, &g);
					if (rc) return rc;
				}
				cur = (cur + n) & 1u;
				l -= n;
			}
			if (cur == h->cur) break; // even total: the next call starts from the same buffer
		}
		return CA3D_OK;
	}
	if (!strcmp(name, "stats")) { h->want_stats = value ? 1 : 0; if (!value) h->ev_valid = false; return CA3D_OK; }
	if (!strcmp(name, "graph_min"))
	{
		if (value < 1 || value > kMaxGraphSteps) return fail(CA3D_ERR_INVALID_ARGUMENT, "graph_min must be in [1, %u]", kMaxGraphSteps);
		h->graph_min = (uint32_t)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "render_indirect")) { h->render_indirect = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "render_sched")) { h->render_sched = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "render_skip")) { h->render_skip = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "rows"))
	{
		h->use_rows = value ? 1 : 0;
		refresh_kernels(h);
		return CA3D_OK;
	}
	if (!strcmp(name, "render_frame_bricks")) { h->render_frame_bricks = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "render_stream")) { h->render_stream = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "render_pipeline")) // converged frames in flight (FrameLane): 0 off, 1 the default depth, 2 .. kMaxLanes that many
	{
		if (value < 0 || value > ca3d_engine::kMaxLanes) return fail(CA3D_ERR_INVALID_ARGUMENT, "render_pipeline must be 0 (off), 1 (default depth) or 2 .. %d frames in flight", ca3d_engine::kMaxLanes);
		h->render_pipeline = (int)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "render_stream_check")) { h->render_stream_check = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "render_row_begin") || !strcmp(name, "render_row_end"))
	{
		if (value < 0 || value > 16384) return fail(CA3D_ERR_INVALID_ARGUMENT, "row %lld is outside any target", (long long)value);
		if (name[11] == 'b')
		{
			if (value % 16) return fail(CA3D_ERR_INVALID_ARGUMENT, "render_row_begin must be a multiple of 16 (the renderer's tile height)");
			h->render_row0 = (uint32_t)value;
		}
		else h->render_row1 = (uint32_t)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "render_mode"))
	{
		if (value != 0 && value != 1) return fail(CA3D_ERR_INVALID_ARGUMENT, "render_mode must be 0 (converged frame) or 1 (one literal reference frame)");
		h->render_mode = (int)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "render_reset_history"))
	{
		// forget the temporal history (a fresh canvas): the next literal frame sees zeros, as on the reference's first frame
		int rc2 = bind_device(h);
		if (rc2) return rc2;
		return clear_render_history(h);
	}
	if (!strcmp(name, "fused")) { drop_graph(h); h->use_fused = value ? 1 : 0; return CA3D_OK; }
	if (!strcmp(name, "variant"))
	{
		if (value != 0 && value != 1) return fail(CA3D_ERR_INVALID_ARGUMENT, "variant must be 0 (auto) or 1 (generic kernel)");
		drop_graph(h);
		h->variant = (int)value;
		refresh_kernels(h);
		return CA3D_OK;
	}
	if (!strcmp(name, "resident"))
	{
		h->use_resident = value ? 1 : 0;
		if (value) h->res_failed = false;
		refresh_kernels(h);
		return CA3D_OK;
	}
	if (!strcmp(name, "resident_rows"))
	{
		if (value != 16 && value != 32) return fail(CA3D_ERR_INVALID_ARGUMENT, "resident_rows must be 16 or 32");
		if ((uint32_t)value != h->res_rows)
		{
			// the mailboxes are indexed by tile: start from clean ones
			int rc2 = bind_device(h);
			if (rc2) return rc2;
			HIP_TRY(hipStreamSynchronize(h->stream));
			free_resident(h);
			h->res_rows = (uint32_t)value;
			refresh_kernels(h);
		}
		return CA3D_OK;
	}
	if (!strcmp(name, "resident_pair"))
	{
		if (value != 0 && value != 1) return fail(CA3D_ERR_INVALID_ARGUMENT, "resident_pair must be 0 or 1");
		if ((value != 0) != h->res_pair)
		{
			int rc2 = bind_device(h);
			if (rc2) return rc2;
			HIP_TRY(hipStreamSynchronize(h->stream));
			free_resident(h); // the tiling may change with it (32-row tiles): start from clean mailboxes
			h->res_pair = value != 0;
			refresh_kernels(h);
		}
		return CA3D_OK;
	}
	if (!strcmp(name, "resident_zsplit"))
	{
		if (value != 1 && value != 2) return fail(CA3D_ERR_INVALID_ARGUMENT, "resident_zsplit must be 1 or 2");
		h->res_zsplit = (uint32_t)value;
		refresh_kernels(h);
		return CA3D_OK;
	}
	if (!strcmp(name, "resident_min"))
	{
		if (value < 1) return fail(CA3D_ERR_INVALID_ARGUMENT, "resident_min must be >= 1");
		h->res_min = (uint32_t)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "resident_timeout_us"))
	{
		if (value < 1 || value > 40000000) return fail(CA3D_ERR_INVALID_ARGUMENT, "resident_timeout_us must be in [1, 40000000]");
		h->res_timeout_ticks = (uint32_t)(value * 100);
		return CA3D_OK;
	}
	if (!strcmp(name, "roll_z"))
	{
		if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16 && value != 15 && value != 30) return fail(CA3D_ERR_INVALID_ARGUMENT, "roll_z must be 0 (automatic), 2, 4, 8, 16 (tile form only), or 15 / 30 (looped forms)");
		drop_graph(h);
		h->roll_z = (int)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "roll_tile"))
	{
		drop_graph(h);
		if (value < 0 || value > 3) return fail(CA3D_ERR_INVALID_ARGUMENT, "roll_tile must be 0 (every thread shifts its rows), 1 (256-thread tiles), 2 (wave tiles) or 3 (two words per thread)");
		h->roll_tile = (int)value;
		return CA3D_OK;
	}
	if (!strcmp(name, "roll"))
	{
		drop_graph(h);
		h->use_roll = value ? 1 : 0;
		refresh_kernels(h);
		return CA3D_OK;
	}
	if (!strcmp(name, "jit"))
	{
		drop_graph(h);
		h->use_jit = value ? 1 : 0;
		refresh_kernels(h);
		return CA3D_OK;
	}
	return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown option '%s'", name);
}
CA3D_API_CATCH

} // extern "C"

// ------------------------------------------------------------------------------------------------ internals for ca3d_group.cpp
namespace ca3d
{
// A full-grid engine that only ever RECEIVES its state on the device (the group's frame: peer copies of the slabs): both buffers
// cleared on the engine's stream, marked as holding a state — no host copy of the grid, no synchronous upload.
int engine_mark_state(ca3d_engine *h)
{
	if (!h || !h->configured || h->slab) return fail(CA3D_ERR_NOT_CONFIGURED, "engine_mark_state: a configured full-grid engine is needed");
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipMemsetAsync(h->buf[0], 0, h->buffer_words() * sizeof(uint32_t), h->stream));
	HIP_TRY(hipMemsetAsync(h->buf[1], 0, h->buffer_words() * sizeof(uint32_t), h->stream));
	h->step = 0;
	h->cur = 0;
	h->prev_ok = false;
	h->has_state = true;
	h->binary_state = true;
	h->state_serial++;
	h->buffers_exposed = false;
	return CA3D_OK;
}
int engine_state_buffer(ca3d_engine *h, int which, void **device_ptr, size_t *n_bytes)
{
	const bool was = h ? h->buffers_exposed : false;
	const int rc = ca3d_device_buffer(h, which, device_ptr, n_bytes);
	if (h) h->buffers_exposed = was;
	return rc;
}
} // namespace ca3d
