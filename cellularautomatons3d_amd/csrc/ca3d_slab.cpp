// Z-slab engines of the C-ABI layer: a batch of sub-steps whole or in two phases (slab_batch), and the halo transport inside the
// engine — RCCL, loaded on first use — with the entry points that run batches and exchanges together (ca3d_slab_run, ca3d_slab_gather).
#include <dlfcn.h>
#include <cstring>
#include <string>
#include <vector>

#include "ca3d_engine.h"

namespace ca3d
{

// ---------------------------------------------------------------------------------------------- RCCL transport
// librccl is loaded on first use (dlopen): single-GPU hosts and the Node.js addon never pay for it, and a process that
// has torch's copy of librccl.so.1 loaded gets that same copy.
typedef struct { char internal[128]; } ncclUniqueIdBytes; // ncclUniqueId (NCCL_UNIQUE_ID_BYTES)

struct Rccl
{
	void *lib = nullptr;
	int (*GetUniqueId)(void *) = nullptr;
	int (*CommInitRank)(void **, int, ncclUniqueIdBytes, int) = nullptr;
	int (*CommDestroy)(void *) = nullptr;
	int (*GroupStart)() = nullptr;
	int (*GroupEnd)() = nullptr;
	int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
	int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
	int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
	int (*CommCount)(void *, int *) = nullptr;
	int (*CommUserRank)(void *, int *) = nullptr;
	int (*CommCuDevice)(void *, int *) = nullptr;
	const char *(*GetErrorString)(int) = nullptr;
	std::string error;
};

static Rccl &rccl()
{
	static Rccl r;
	static bool tried = false;
	if (tried) return r;
	tried = true;
	for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
	{
		r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
		if (r.lib) break;
	}
	if (!r.lib) { r.error = std::string("librccl.so.1 could not be loaded: ") + dlerror(); return r; }
	auto sym = [&](const char *n) { void *p = dlsym(r.lib, n); if (!p && r.error.empty()) r.error = std::string("librccl lacks ") + n; return p; };
	r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
	r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
	r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
	r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
	r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
	r.Send = (decltype(r.Send))sym("ncclSend");
	r.Recv = (decltype(r.Recv))sym("ncclRecv");
	r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
	r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
	r.CommCount = (decltype(r.CommCount))sym("ncclCommCount");
	r.CommUserRank = (decltype(r.CommUserRank))sym("ncclCommUserRank");
	r.CommCuDevice = (decltype(r.CommCuDevice))sym("ncclCommCuDevice");
	return r;
}

#define NCCL_TRY(expr)                                                                                                   \
	do                                                                                                                   \
	{                                                                                                                    \
		int r_ = (expr);                                                                                                 \
		if (r_ != 0) return fail(CA3D_ERR_DEVICE, "%s: %s", #expr, rccl().GetErrorString ? rccl().GetErrorString(r_) : "?"); \
	} while (0)

constexpr int kNcclUint32 = 3; // ncclUint32 (rccl.h)

// Refresh the ghost planes of the buffer ca3d_slab_region refers to, on stream `s`: the same plan as slab.halo_plan —
// packed: open at the bottom (z == -1 is dead), closed at the top (plane G wraps to plane 0); unpacked: a ring.
static int comm_exchange(ca3d_engine *h, hipStream_t s)
{
	Rccl &r = rccl();
	const int P = h->comm_world, me = h->comm_rank, below = (me + P - 1) % P, above = (me + 1) % P;
	const bool ring = h->layout == CA3D_LAYOUT_UNPACKED, top = me == P - 1, bottom = me == 0;
	void *p[4];
	size_t bytes[4];
	for (int region = 0; region < 4; region++)
	{
		int rc = ca3d_slab_region(h, region, &p[region], &bytes[region]);
		if (rc) return rc;
	}
	const size_t n = bytes[0] / sizeof(uint32_t);
	NCCL_TRY(r.GroupStart());
	// sends low-then-high, receives high-then-low: the two messages a pair of ranks exchanges in one direction (world == 2)
	// then match in order
	NCCL_TRY(r.Send(p[CA3D_SLAB_SEND_LOW], n, kNcclUint32, below, h->comm, s));
	if (ring || !top) NCCL_TRY(r.Send(p[CA3D_SLAB_SEND_HIGH], n, kNcclUint32, above, h->comm, s));
	NCCL_TRY(r.Recv(p[CA3D_SLAB_RECV_HIGH], n, kNcclUint32, above, h->comm, s));
	if (ring || !bottom) NCCL_TRY(r.Recv(p[CA3D_SLAB_RECV_LOW], n, kNcclUint32, below, h->comm, s));
	NCCL_TRY(r.GroupEnd());
	return CA3D_OK;
}

// Slab batch of n sub-steps, whole or in two phases (include/ca3d.h). Array planes: ghost [0,K), owned [K,K+nz),
// ghost [K+nz, L). Sub-step s (1..n) of the whole batch updates [s, L-s). The phased form splits that range:
//   low edge   [s, 2K+n-s)          ends at s = n as [n, 2K): covers the planes sent down, [K, 2K)
//   high edge  [L-2K-n+s, L-s)      ends as [L-2K, L-n): covers the planes sent up, [nz, nz+K)
//   interior   [2K+n-s, L-2K-n+s)   grows by one plane per side per sub-step
// Each edge chain reads only its own previous sub-step; both zones go into ONE launch per sub-step (the packed
// class kernels take two output ranges: a second stream with fork / join events inside the captured graph cost
// ~40 us of host time per graph launch). The interior reads one plane of each edge per sub-step, which the edge
// chains — finished first — never overwrite afterwards (their ranges shrink).
static int slab_batch(ca3d_engine *h, uint32_t n_steps, int phase)
{
	int rc = check_ready(h);
	if (rc) return rc;
	if (!h->slab) return fail(CA3D_ERR_INVALID_ARGUMENT, "engine is not a slab: use ca3d_step");
	if (n_steps > h->ghost) return fail(CA3D_ERR_INVALID_ARGUMENT, "%u sub-steps exceed the ghost depth %u", n_steps, h->ghost);
	if (phase == CA3D_SLAB_PHASE_EDGES && h->pending_edges) return fail(CA3D_ERR_INVALID_ARGUMENT, "edge phase issued twice: the interior phase must follow");
	if (phase == CA3D_SLAB_PHASE_INTERIOR && h->pending_edges != n_steps) return fail(CA3D_ERR_INVALID_ARGUMENT, "interior phase of %u sub-steps does not follow an edge phase of the same length", n_steps);
	if (phase == CA3D_SLAB_PHASE_ALL && h->pending_edges) return fail(CA3D_ERR_INVALID_ARGUMENT, "an edge phase is pending: finish it with the interior phase");
	rc = bind_device(h);
	if (rc) return rc;
	if (n_steps == 0) return CA3D_OK;
	// Unpacked layout: the first sub-step of a batch reads the state as uploaded, which may hold cell values above 1 (the ballot kernel
	// must not be given those); every later one reads what a kernel wrote. The interior phase starts from that same buffer once more,
	// after the edge phase has marked the state as 0 / 1: its first sub-step (and whether the batch may be a graph) goes by what the
	// edge phase found.
	if (phase == CA3D_SLAB_PHASE_EDGES) h->pending_binary = h->binary_state;
	else if (phase == CA3D_SLAB_PHASE_INTERIOR) h->binary_state = h->pending_binary;
	h->buffers_exposed = false;
	const uint32_t L = h->nplanes, K = h->ghost, n = n_steps;
	// The packed kernel's bottom face is dead (z == -1 is dropped): the slab that owns global plane 0 never needs
	// its low ghost.
	const uint32_t lo_floor = (h->layout == CA3D_LAYOUT_PACKED32 && h->z0 == 0) ? K : 0u;
	const bool splittable = h->nz + 2u > 2u * K + 2u * n; // interior non-empty in every sub-step
	if (phase != CA3D_SLAB_PHASE_INTERIOR && h->want_stats) HIP_TRY(hipEventRecord(h->ev_start, h->stream));
	int what = phase; // what this call enqueues
	if (!splittable)
	{
		// thin slab: the edge phase does the whole batch, the interior phase only commits it
		what = phase == CA3D_SLAB_PHASE_INTERIOR ? -1 : CA3D_SLAB_PHASE_ALL;
	}
	auto enqueue_all = [&](uint32_t start_buf) -> int {
		uint32_t cur = start_buf;
		for (uint32_t s = 1; s <= n; s++, cur ^= 1u)
		{
			const uint32_t lo = s > lo_floor ? s : lo_floor, hi = L - s;
			const uint32_t e_lo = 2u * K + n - s, e_hi = L - 2u * K - n + s;
			int r2 = CA3D_OK;
			if (what == CA3D_SLAB_PHASE_ALL) r2 = enqueue_step(h, (int)cur, lo, hi, h->stream);
			else if (what == CA3D_SLAB_PHASE_INTERIOR) r2 = enqueue_step(h, (int)cur, e_lo, e_hi, h->stream);
			else r2 = enqueue_step(h, (int)cur, lo, e_lo, h->stream, false, e_hi, hi); // both edge zones, one launch
			if (r2) return r2;
		}
		return CA3D_OK;
	};
	const bool graphable = graphs_allowed(h) && n > 1;
	// (the interior phase of a thin slab commits what its edge phase ran: how that batch ran is what the edge phase noted)
	const bool resident = what < 0 ? h->pending_resident : what == CA3D_SLAB_PHASE_ALL && resident_wanted(h, n);
	if (what < 0) { /* nothing to enqueue */ }
	else if (resident)
	{
		rc = resident_slab_steps(h, n);
		if (rc) return rc;
	}
	else if (graphable)
	{
		// one graph launch per batch: the host cost of a K-step batch must stay below its GPU time for the ranks
		// to scale (8 launches of ~7 us kernels would otherwise be host-bound)
		const uint64_t key = ((uint64_t)what << 40) | ((uint64_t)h->cur << 32) | n;
		auto it = h->slab_graphs.find(key);
		if (it == h->slab_graphs.end())
		{
			hipGraphExec_t exec = nullptr;
			rc = capture_graph(h, [&]() { return enqueue_all(h->cur); }, &exec);
			if (rc) return rc;
			it = h->slab_graphs.emplace(key, exec).first;
		}
		HIP_TRY(hipGraphLaunch(it->second, h->stream));
	}
	else
	{
		rc = enqueue_all(h->cur);
		if (rc) return rc;
	}
	if (h->layout == CA3D_LAYOUT_UNPACKED) h->binary_state = true;
	if (phase == CA3D_SLAB_PHASE_EDGES)
	{
		h->pending_edges = n; // ca3d_slab_region now refers to the buffer the batch ends in
		h->pending_resident = resident;
		return CA3D_OK;
	}
	h->pending_edges = 0;
	h->step += n;
	h->cur = (h->cur + n) & 1u;
	// Sub-step n - 1 of the per-step kernels wrote planes [n - 1, L - n + 1) of the other buffer (n == 1: it is the batch's input), which
	// cover the owned planes [K, K + nz) because n <= K: they hold the state one step earlier. The resident slab launch writes its final
	// state only (for an even n into the buffer it read from): nothing is known about the other buffer then.
	h->prev_ok = !resident;
	h->ghosts_valid = false; // the caller (or ca3d_slab_run) refreshes them
	const uint32_t launches = resident ? 1u : (phase == CA3D_SLAB_PHASE_ALL || !splittable ? n : 2u * n);
	h->launches_total += launches;
	return record_batch_stats(h, n, launches, h->nz);
}

void free_slab_comm(ca3d_engine *h)
{
	if (h->comm && rccl().CommDestroy) rccl().CommDestroy(h->comm);
	if (h->ev_edges) hipEventDestroy(h->ev_edges);
	if (h->ev_comm) hipEventDestroy(h->ev_comm);
	if (h->ev_gather) hipEventDestroy(h->ev_gather);
	if (h->comm_stream) hipStreamDestroy(h->comm_stream);
}

// One communicator per slab engine, all created by THIS process (ncclCommInitAll: one host thread, n devices) — the
// single-process form of ca3d_slab_comm_init. RCCL refuses two ranks on one device.
int engines_rccl_init_all(ca3d_engine **engines, int n)
{
	Rccl &r = rccl();
	if (!r.error.empty()) return fail(CA3D_ERR_UNSUPPORTED, "%s", r.error.c_str());
	typedef int (*InitAll)(void **, int, const int *);
	InitAll init_all = (InitAll)dlsym(r.lib, "ncclCommInitAll");
	if (!init_all) return fail(CA3D_ERR_UNSUPPORTED, "librccl lacks ncclCommInitAll");
	std::vector<void *> comms((size_t)n, nullptr);
	std::vector<int> devs((size_t)n);
	for (int k = 0; k < n; k++) devs[(size_t)k] = engines[k]->device;
	NCCL_TRY(init_all(comms.data(), n, devs.data()));
	for (int k = 0; k < n; k++)
	{
		ca3d_engine *h = engines[k];
		if (h->comm) r.CommDestroy(h->comm);
		h->comm = comms[(size_t)k];
		h->comm_rank = k;
		h->comm_world = n;
		h->ghosts_valid = false;
	}
	return CA3D_OK;
}

// The ghost refresh of every rank as ONE RCCL group (a single thread cannot post rank 0's sends and wait for them before
// rank 1's receives exist): ncclGroupStart, every rank's sends and receives on its own stream, ncclGroupEnd.
int engines_rccl_exchange_all(ca3d_engine **engines, int n)
{
	Rccl &r = rccl();
	NCCL_TRY(r.GroupStart());
	for (int k = 0; k < n; k++)
	{
		int rc = bind_device(engines[k]);
		if (rc == CA3D_OK) rc = comm_exchange(engines[k], engines[k]->stream);
		if (rc) { r.GroupEnd(); return rc; }
	}
	NCCL_TRY(r.GroupEnd());
	for (int k = 0; k < n; k++) engines[k]->ghosts_valid = true;
	return CA3D_OK;
}
} // namespace ca3d

using namespace ca3d;

extern "C"
{

int ca3d_slab_step(ca3d_t *h, uint32_t n_steps) CA3D_API_TRY
{
	return slab_batch(h, n_steps, CA3D_SLAB_PHASE_ALL);
}
CA3D_API_CATCH

int ca3d_slab_step_phase(ca3d_t *h, uint32_t n_steps, int phase) CA3D_API_TRY
{
	if (phase != CA3D_SLAB_PHASE_ALL && phase != CA3D_SLAB_PHASE_EDGES && phase != CA3D_SLAB_PHASE_INTERIOR)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown slab phase %d", phase);
	return slab_batch(h, n_steps, phase);
}
CA3D_API_CATCH

int ca3d_slab_region(ca3d_t *h, int region, void **device_ptr, size_t *n_bytes) CA3D_API_TRY
{
	if (!h || !device_ptr || !n_bytes) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!h->configured || !h->slab) return fail(CA3D_ERR_NOT_CONFIGURED, "engine is not configured as a slab");
	uint32_t *base = h->buf[(h->cur + h->pending_edges) & 1u]; // after an edge phase: the buffer its results are in
	const size_t pw = h->plane_words;
	const uint32_t K = h->ghost, nz = h->nz;
	size_t first = 0, count = K;
	switch (region)
	{
	case CA3D_SLAB_SEND_LOW: first = K; break;
	case CA3D_SLAB_SEND_HIGH: first = nz; break; // K + nz - K
	case CA3D_SLAB_RECV_LOW: first = 0; break;
	case CA3D_SLAB_RECV_HIGH: first = (size_t)K + nz; break;
	case CA3D_SLAB_OWNED: first = K; count = nz; break;
	default: return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown slab region %d", region);
	}
	*device_ptr = base + first * pw;
	*n_bytes = count * pw * sizeof(uint32_t);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_comm_unique_id(void *id) CA3D_API_TRY
{
	if (!id) return fail(CA3D_ERR_INVALID_ARGUMENT, "id is NULL");
	Rccl &r = rccl();
	if (!r.error.empty()) return fail(CA3D_ERR_UNSUPPORTED, "%s", r.error.c_str());
	NCCL_TRY(r.GetUniqueId(id));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_slab_comm_init(ca3d_t *h, const void *id, int rank, int world) CA3D_API_TRY
{
	if (!h || !id) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (world < 1 || rank < 0 || rank >= world) return fail(CA3D_ERR_INVALID_ARGUMENT, "rank %d of %d", rank, world);
	Rccl &r = rccl();
	if (!r.error.empty()) return fail(CA3D_ERR_UNSUPPORTED, "%s", r.error.c_str());
	int rc = bind_device(h);
	if (rc) return rc;
	if (h->comm) { r.CommDestroy(h->comm); h->comm = nullptr; }
	ncclUniqueIdBytes uid;
	memcpy(&uid, id, sizeof uid);
	NCCL_TRY(r.CommInitRank(&h->comm, world, uid, rank));
	h->comm_rank = rank;
	h->comm_world = world;
	if (!h->comm_stream)
	{
		HIP_TRY(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&h->ev_edges, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&h->ev_comm, hipEventDisableTiming));
	}
	h->ghosts_valid = false;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_slab_comm_info(ca3d_t *h, ca3d_comm_info *out) CA3D_API_TRY
{
	if (!h || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	memset(out, 0, sizeof *out);
	out->comm_ranks = out->comm_rank = out->comm_device = -1;
	out->device = h->device;
	int rc = bind_device(h);
	if (rc) return rc;
	HIP_TRY(hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof out->pci_bus_id, h->device));
	if (h->comm)
	{
		// what the COMMUNICATOR says, not what the caller passed to ca3d_slab_comm_init
		NCCL_TRY(rccl().CommCount(h->comm, &out->comm_ranks));
		NCCL_TRY(rccl().CommUserRank(h->comm, &out->comm_rank));
		NCCL_TRY(rccl().CommCuDevice(h->comm, &out->comm_device));
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_slab_exchange(ca3d_t *h) CA3D_API_TRY
{
	int rc = check_ready(h);
	if (rc) return rc;
	if (!h->slab || !h->comm) return fail(CA3D_ERR_NOT_CONFIGURED, "engine is not a slab with a communicator (ca3d_configure_slab, ca3d_slab_comm_init)");
	rc = bind_device(h);
	if (rc) return rc;
	rc = comm_exchange(h, h->stream);
	if (rc == CA3D_OK) h->ghosts_valid = true;
	return rc;
}
CA3D_API_CATCH

int ca3d_slab_run(ca3d_t *h, uint32_t n_steps, int overlap) CA3D_API_TRY
{
	int rc = check_ready(h);
	if (rc) return rc;
	if (!h->slab || !h->comm) return fail(CA3D_ERR_NOT_CONFIGURED, "engine is not a slab with a communicator (ca3d_configure_slab, ca3d_slab_comm_init)");
	if (h->pending_edges) return fail(CA3D_ERR_INVALID_ARGUMENT, "an edge phase is pending: finish it with the interior phase");
	rc = bind_device(h);
	if (rc) return rc;
	if (!h->ghosts_valid)
	{
		rc = comm_exchange(h, h->stream);
		if (rc) return rc;
		h->ghosts_valid = true;
	}
	const bool keep_stats = h->want_stats != 0;
	uint32_t left = n_steps;
	uint64_t launches = 0;
	if (keep_stats && left) HIP_TRY(hipEventRecord(h->ev_start, h->stream));
	h->want_stats = 0; // the batches below would each re-record the pair
	auto restore = [&]() { h->want_stats = keep_stats ? 1 : 0; };
	while (left)
	{
		const uint32_t k = left < h->ghost ? left : h->ghost;
		if (overlap)
		{
			// edge zones -> their planes travel on the communication stream while the interior runs -> the next batch
			// (and anything else on the engine's stream) waits for the receives
			rc = slab_batch(h, k, CA3D_SLAB_PHASE_EDGES);
			if (rc) { restore(); return rc; }
			HIP_TRY(hipEventRecord(h->ev_edges, h->stream));
			HIP_TRY(hipStreamWaitEvent(h->comm_stream, h->ev_edges, 0));
			rc = comm_exchange(h, h->comm_stream);
			if (rc) { restore(); return rc; }
			HIP_TRY(hipEventRecord(h->ev_comm, h->comm_stream));
			rc = slab_batch(h, k, CA3D_SLAB_PHASE_INTERIOR);
			if (rc) { restore(); return rc; }
			HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_comm, 0));
		}
		else
		{
			rc = slab_batch(h, k, CA3D_SLAB_PHASE_ALL);
			if (rc) { restore(); return rc; }
			rc = comm_exchange(h, h->stream);
			if (rc) { restore(); return rc; }
		}
		h->ghosts_valid = true;
		launches += h->stats.kernel_launches;
		left -= k;
	}
	restore();
	if (keep_stats && n_steps) return record_batch_stats(h, n_steps, launches, h->nz); // (not added to launches_total: the batches did that)
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_slab_gather(ca3d_t *h, ca3d_t *full) CA3D_API_TRY
{
	if (!h || !full) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!h->slab || !h->comm || !h->has_state) return fail(CA3D_ERR_NOT_CONFIGURED, "engine is not a slab with a communicator and a state");
	if (!full->configured || full->slab || full->G != h->G || full->layout != h->layout || full->device != h->device)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "the target must be a full-grid engine of the same grid, layout and device");
	FLUSH_QUEUED(full);
	if (int rcs = settle_resident(full)) return rcs;
	if ((size_t)h->nz * h->comm_world != h->G) return fail(CA3D_ERR_UNSUPPORTED, "the slabs must split the grid evenly");
	int rc = bind_device(h);
	if (rc) return rc;
	void *owned;
	size_t bytes;
	rc = ca3d_slab_region(h, CA3D_SLAB_OWNED, &owned, &bytes);
	if (rc) return rc;
	// ncclAllGather straight between the engines' device buffers, in rank (= z) order, on the slab engine's stream. When the
	// target engine runs on another stream the gather waits for what that stream still does with the buffer (a frame being
	// rendered from it) and that stream waits for the gather before it touches the buffer again.
	const bool cross = full->stream != h->stream;
	if (cross)
	{
		if (!h->ev_gather) HIP_TRY(hipEventCreateWithFlags(&h->ev_gather, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(h->ev_gather, full->stream));
		HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_gather, 0));
	}
	NCCL_TRY(rccl().AllGather(owned, full->buf[full->cur], bytes / sizeof(uint32_t), kNcclUint32, h->comm, h->stream));
	if (cross)
	{
		HIP_TRY(hipEventRecord(h->ev_gather, h->stream));
		HIP_TRY(hipStreamWaitEvent(full->stream, h->ev_gather, 0));
	}
	full->has_state = true;
	full->state_serial++;
	full->prev_ok = false; // only the current buffer was written
	return CA3D_OK;
}
CA3D_API_CATCH

} // extern "C"
