/*
 * ca3d.h — C ABI of the MI355X-native engine for the two hot paths of lightest/cellularautomatons3d:
 * the 3D cellular-automaton step and (see ca3d_render*) the per-pixel volume renderer.
 *
 * This is the drop-in boundary: the reference drives its kernels through the browser's WebGPU API from
 * main_pathtraced.js; each entry point below names the reference call sites it replaces. Plain C, opaque handle,
 * plain pointers and sizes. Every function returns 0 (CA3D_OK) or a negative ca3d_status; ca3d_last_error()
 * gives the message for the calling thread. Caller-owned host buffers are fully consumed before a call
 * returns. Calls on one handle are not thread-safe (the reference host is a single JS thread). One engine
 * owns one HIP stream on one device; work is enqueued asynchronously exactly like the reference's
 * queue.submit — only ca3d_read_state / ca3d_synchronize / the stats getters wait for the GPU.
 *
 * There is no CPU fallback: without a usable HIP device ca3d_create fails with CA3D_ERR_DEVICE.
 */
#ifndef CA3D_H
#define CA3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CA3D_ABI_VERSION 7 /* 5: + ca3d_get_kernel_variant; 6: + ca3d_selftest_exception, the kernel cache (ca3d_get_jit_log reports it); 7: + ca3d_get_render_pipeline; still 7 (additions only): + ca3d_summarize, ca3d_group_summarize, ca3d_step_until, ca3d_get_summary_time; + ca3d_ensemble_*; + ca3d_seed_state, ca3d_group_seed_state, ca3d_ensemble_seed_state, ca3d_ensemble_set_rule_tables; + ca3d_ensemble_configure_neighbourhood, ca3d_ensemble_get_neighbourhood; + CA3D_STOP_PERIODIC, ca3d_step_until_cycle, ca3d_ensemble_step_until_cycle; + ca3d_ensemble_step_until_trace */
#define CA3D_LUT_LEN 81 /* 3 rule-sets x 27 slots (main_pathtraced.js:10, 155-159) */

typedef struct ca3d_engine ca3d_t;

enum ca3d_status
{
	CA3D_OK = 0,
	CA3D_ERR_INVALID_ARGUMENT = -1,
	CA3D_ERR_NOT_CONFIGURED = -2, /* call order: configure -> set_rules -> upload_state -> step */
	CA3D_ERR_DEVICE = -3,         /* HIP error, or no GPU */
	CA3D_ERR_OUT_OF_MEMORY = -4,
	CA3D_ERR_UNSUPPORTED = -5
};

enum ca3d_layout
{
	CA3D_LAYOUT_PACKED32 = 0, /* 32 x-adjacent cells per u32: shaders/compute_clustered.wgsl (the live kernel) */
	CA3D_LAYOUT_UNPACKED = 1  /* one u32 (0/1) per cell, toroidal: shaders/compute.wgsl (legacy kernel) */
};

int ca3d_abi_version(void);
const char *ca3d_last_error(void);
/* No C++ exception crosses this boundary: every entry point catches what the library's internals throw (host allocation
 * failures above all) and returns CA3D_ERR_OUT_OF_MEMORY for std::bad_alloc, CA3D_ERR_DEVICE for anything else, with the
 * message in ca3d_last_error(). Test hook for exactly that path, usable without a GPU: throws inside a guarded body —
 * kind 0 std::bad_alloc, 1 std::runtime_error, 2 a non-std exception, 3 a real oversized host allocation — and returns
 * the status the boundary mapped it to (any other kind: CA3D_OK). */
int ca3d_selftest_exception(int kind);
int ca3d_device_count(int *out_count);

/* navigator.gpu.requestAdapter / requestDevice (main_pathtraced.js:222-225). */
int ca3d_create(int device, ca3d_t **out);
int ca3d_destroy(ca3d_t *h);

/*
 * Grid uniform + state buffers (main_pathtraced.js:1204-1217, 635, 1241, 1314-1326). The reference always
 * writes a cubic [G,G,G]; gx == gy == gz is required. PACKED32: G a positive multiple of 32
 * (_gridSizeUIFormatter, 675-693). UNPACKED: G a positive multiple of 4 (workgroup 4x4x4, compute.wgsl:50).
 * Drops any previous state and resets the step counter (as _restartSim, 624-637).
 */
int ca3d_configure(ca3d_t *h, uint32_t gx, uint32_t gy, uint32_t gz, int layout);

/*
 * Z-slab of a G^3 grid for multi-GPU runs (no reference counterpart): this engine owns global
 * planes [z0, z0+nz) and keeps `ghost` planes below and above them. ghost >= 1. After every ca3d_slab_step
 * batch the host refreshes the ghosts (ca3d_slab_region + its transport, e.g. RCCL send/recv).
 * UNPACKED slabs need a power-of-two G (the legacy kernel's -1 wrap is only a torus then).
 */
int ca3d_configure_slab(ca3d_t *h, uint32_t g, int layout, uint32_t z0, uint32_t nz, uint32_t ghost);

/*
 * Rule buffers exactly as the reference uploads them (main_pathtraced.js:1330-1369) and binds them
 * (1647-1673: 0 main offsets, 1 edges offsets, 2 corners offsets, 3 survive, 4 born). Offset lists are flat
 * xyz triples of i32 (n_* = number of i32, a multiple of 3, every component in {-1,0,1}; duplicates and
 * (0,0,0) are legal and count as the reference kernel would count them). survive/born: 81 u32, slots
 * 0-26 main, 27-53 edges, 54-80 corners. PACKED32 treats an entry as set iff it == 1
 * (compute_clustered.wgsl:232); UNPACKED uses the main list and slots 0-26 with `> 0` (compute.wgsl:160-166).
 */
int ca3d_set_rules(ca3d_t *h,
                   const int32_t *main_offsets, uint32_t n_main,
                   const int32_t *edges_offsets, uint32_t n_edges,
                   const int32_t *corners_offsets, uint32_t n_corners,
                   const uint32_t survive[CA3D_LUT_LEN], const uint32_t born[CA3D_LUT_LEN]);

/*
 * queue.writeBuffer(cell_state_0 / cell_state_1) (main_pathtraced.js:1361-1362): the same words go to both
 * ping-pong buffers and the step counter restarts at 0. n_words must equal the state size:
 * PACKED32 (G/32)*G*G, UNPACKED G^3 (slab: the owned planes only; ghosts are filled by the halo exchange).
 */
int ca3d_upload_state(ca3d_t *h, const uint32_t *words, size_t n_words);

/* Read-back of the current state = buffer [step % 2] (no reference counterpart: parity checks, checkpoints). */
int ca3d_read_state(ca3d_t *h, uint32_t *words, size_t n_words);

/*
 * _computePass (main_pathtraced.js:1796-1809) n_steps times: step k reads buffer k % 2, writes buffer
 * (k+1) % 2; afterwards the current state is buffer [total_steps % 2] and the other buffer holds the state one
 * step earlier, as in the reference. Asynchronous.
 *
 * The reference encodes its passes into a command encoder and hands them to the GPU with ONE queue.submit per frame
 * (main_pathtraced.js:1833-1850). ca3d_set_option("queue", n > 0) gives ca3d_step that meaning: a call only ENCODES its
 * steps; they are submitted together by ca3d_flush, by any other call on the engine that looks at the state, the stream or
 * the options (read-back, render, synchronize, set_rules, get_info ...), or as soon as n steps are waiting. What a caller can
 * observe through the engine is the same either way; consecutive short batches then cost one launch of the resident
 * multi-step kernel instead of one each. A caller that records its own events on the stream calls ca3d_flush first.
 * Off by default ("queue" 0: every ca3d_step submits its own steps).
 */
int ca3d_step(ca3d_t *h, uint32_t n_steps);
int ca3d_flush(ca3d_t *h);

/* Slab mode: n_steps <= ghost sub-steps on a shrinking plane range; then the ghosts must be refreshed. */
int ca3d_slab_step(ca3d_t *h, uint32_t n_steps);

/*
 * The same batch in two phases, so that the halo exchange overlaps the bulk of the compute (BASELINE configs[4]:
 * "halo overlapped with compute"):
 *   CA3D_SLAB_PHASE_EDGES     all n sub-steps on the two edge zones only — afterwards the planes the neighbours
 *                             need (SEND_LOW / SEND_HIGH of ca3d_slab_region) hold their final values of this batch;
 *   (the caller starts the exchange of those planes into the neighbours' ghosts here)
 *   CA3D_SLAB_PHASE_INTERIOR  all n sub-steps on the planes in between, commits the batch (step counter, current
 *                             buffer). It reads no ghost plane, so the exchange may run concurrently with it.
 * EDGES then INTERIOR with the same n equals one ca3d_slab_step(n). Slabs too thin to split (nz + 2 <= 2*ghost + 2*n)
 * run the whole batch in the edge phase. Between the two phases ca3d_slab_region refers to the buffer the batch
 * ends in (where the edge results are, and where the incoming ghosts belong).
 */
enum ca3d_slab_phase
{
	CA3D_SLAB_PHASE_ALL = 0,
	CA3D_SLAB_PHASE_EDGES = 1,
	CA3D_SLAB_PHASE_INTERIOR = 2
};
int ca3d_slab_step_phase(ca3d_t *h, uint32_t n_steps, int phase);

enum ca3d_slab_region_id
{
	CA3D_SLAB_SEND_LOW = 0,  /* first `ghost` owned planes  -> lower neighbour's high ghost */
	CA3D_SLAB_SEND_HIGH = 1, /* last `ghost` owned planes   -> upper neighbour's low ghost  */
	CA3D_SLAB_RECV_LOW = 2,  /* this engine's low ghost planes  */
	CA3D_SLAB_RECV_HIGH = 3, /* this engine's high ghost planes */
	CA3D_SLAB_OWNED = 4      /* all owned planes */
};
/* Device pointer + byte size of a region of the CURRENT buffer (changes with step parity; after an edge phase: of
 * the buffer that batch ends in). */
int ca3d_slab_region(ca3d_t *h, int region, void **device_ptr, size_t *n_bytes);

/*
 * Halo transport inside the engine: RCCL send / receive over xGMI between the ranks of a Z-slab chain, one process per
 * GPU (no reference counterpart). librccl is loaded on first use. Bootstrap: rank 0 calls
 * ca3d_comm_unique_id and hands the 128 bytes to the other ranks by any means (torch.distributed, MPI, a socket, a
 * file); every rank then calls ca3d_slab_comm_init on its slab engine (collective: all ranks must call it).
 *   ca3d_slab_run(n, overlap)  n CA steps in batches of <= ghost sub-steps with the ghost planes refreshed between
 *                              batches; overlap != 0: the edge zones of a batch first, their planes travel on a second
 *                              stream while the interior runs (BASELINE configs[4]). Asynchronous; everything is
 *                              enqueued by this one call (no per-batch host work beyond the launches).
 *   ca3d_slab_exchange         one refresh of the ghost planes of the current state (ca3d_slab_run does it by itself)
 *   ca3d_slab_gather           ncclAllGather of every rank's owned planes into the current buffer of `full`, a full-grid
 *                              engine on the same device: the volume a renderer needs (shadow rays cross slabs)
 * The chain follows the kernel's boundary: packed — open at the bottom, closed at the top; unpacked — a ring.
 */
#define CA3D_COMM_ID_BYTES 128
int ca3d_comm_unique_id(void *id_bytes);
int ca3d_slab_comm_init(ca3d_t *h, const void *id_bytes, int rank, int world);
int ca3d_slab_run(ca3d_t *h, uint32_t n_steps, int overlap);
int ca3d_slab_exchange(ca3d_t *h);
/* Evidence of what a multi-GPU run really ran on (bench.py prints it per rank): the engine's HIP device and its PCI bus id
 * (hipDeviceGetPCIBusId), and — once ca3d_slab_comm_init has built the engine's RCCL communicator — what the COMMUNICATOR
 * reports: ncclCommCount, ncclCommUserRank, ncclCommCuDevice (-1 each without one). Eight ranks are eight GPUs only if
 * the eight bus ids differ. */
typedef struct ca3d_comm_info
{
	int32_t device;       /* the engine's HIP device ordinal */
	int32_t comm_ranks;   /* ncclCommCount */
	int32_t comm_rank;    /* ncclCommUserRank */
	int32_t comm_device;  /* ncclCommCuDevice */
	char pci_bus_id[32];  /* "0000:05:00.0" */
} ca3d_comm_info;
int ca3d_slab_comm_info(ca3d_t *h, ca3d_comm_info *out);
int ca3d_slab_gather(ca3d_t *h, ca3d_t *full);

/*
 * The same split driven by ONE host thread (SURVEY 8(b) sketched `ca3d_create(const int* device_ids, int n_devices, ...)`):
 * the reference's host is a single JavaScript thread that enqueues everything (main_pathtraced.js:1821-1854), and BASELINE's
 * north star keeps the host in JavaScript while the grid is Z-slabbed over the GPUs of a node. A group = one slab engine per
 * entry of the device list, rank k owning planes [k G/n, (k+1) G/n) (a device may be listed more than once: several slabs
 * on one GPU, which is how the path is tested on one GPU), plus the ghost exchange between them.
 *   ca3d_group_configure     grid, layout, ghost depth K = steps between exchanges (ca3d_configure_slab on every engine)
 *   ca3d_group_set_rules     ca3d_set_rules on every engine (payload as there)
 *   ca3d_group_upload_state  the FULL grid in the reference's layout; each slab takes its planes
 *   ca3d_group_read_state    the full grid back
 *   ca3d_group_step          n steps: batches of <= K sub-steps on every device, ghosts refreshed between batches; everything
 *                            is enqueued by this one call, nothing waits for a GPU
 *   ca3d_group_render        ca3d_render for the whole grid: every rank gets the full packed volume (peer copies), renders
 *                            its band of image rows and the bands land in the caller's buffers
 *   ca3d_group_engine        the slab engine of a rank (for ca3d_get_info, ca3d_get_stats ...); owned by the group
 *   ca3d_group_set_option    "transport" 0 (default): the ghost planes travel as peer-to-peer device copies over xGMI on the
 *                            receiving engine's stream, ordered by events; 1: ncclSend / ncclRecv on communicators from
 *                            ncclCommInitAll, one ncclGroupStart / End per exchange (one device per slab). Every other name
 *                            goes to ca3d_set_option of every engine.
 * Packed grids: the chain is open at the bottom and closed at the top; unpacked: a ring (as ca3d_slab_comm_init).
 */
typedef struct ca3d_group ca3d_group_t;
int ca3d_group_create(const int *device_ids, int n_devices, ca3d_group_t **out);
int ca3d_group_destroy(ca3d_group_t *g);
int ca3d_group_size(ca3d_group_t *g, int *out_n);
int ca3d_group_engine(ca3d_group_t *g, int rank, ca3d_t **out);
int ca3d_group_configure(ca3d_group_t *g, uint32_t grid_size, int layout, uint32_t ghost);
int ca3d_group_set_rules(ca3d_group_t *g,
                         const int32_t *main_offsets, uint32_t n_main,
                         const int32_t *edges_offsets, uint32_t n_edges,
                         const int32_t *corners_offsets, uint32_t n_corners,
                         const uint32_t survive[CA3D_LUT_LEN], const uint32_t born[CA3D_LUT_LEN]);
int ca3d_group_upload_state(ca3d_group_t *g, const uint32_t *words, size_t n_words);
int ca3d_group_read_state(ca3d_group_t *g, uint32_t *words, size_t n_words);
int ca3d_group_step(ca3d_group_t *g, uint32_t n_steps);
int ca3d_group_synchronize(ca3d_group_t *g);
int ca3d_group_set_option(ca3d_group_t *g, const char *name, int64_t value);
int ca3d_group_render(ca3d_group_t *g, const float uniforms[128], uint32_t width, uint32_t height, uint32_t spp,
                      uint8_t *presentation_rgba8, uint16_t *light_rgba16f, uint16_t *depth_rg16f);
/* ca3d_summarize (below) for the whole grid: synchronises the group, summarises every rank on its own device and combines on the host —
 * sums, the union of the boxes, the plane counts concatenated in z order (G entries, nullable), has_previous the AND of the ranks'. */
struct ca3d_summary;
int ca3d_group_summarize(ca3d_group_t *g, struct ca3d_summary *out, uint32_t *plane_population);

/* Device pointer + byte size of the targets of the last ca3d_render call: 0 presentation RGBA8, 1 light RGBA16F,
 * 2 depth RG16F (row-major, top row first) — e.g. to gather the bands of a frame shared between GPUs without a
 * round trip through the host. */
int ca3d_render_target(ca3d_t *h, int which, void **device_ptr, size_t *n_bytes);

int ca3d_synchronize(ca3d_t *h);

/*
 * State summary on the device (no reference counterpart: its UI shows no statistics): how many cells are alive, where, and whether
 * anything still changes — one pass of one kernel over the state, a few dozen bytes back over the bus instead of the state.
 *
 * What is summarised: the CURRENT state, buffer [step % 2], after everything already asked of the engine — queued steps are
 * submitted first (option "queue"), and a pending resident launch is verified and, if it gave up, recovered from (the entry guard of
 * ca3d_read_state: a summary never describes the output of a launch that would have been rolled back). Runs on the engine's stream
 * (or the one given by ca3d_set_stream), only READS the state, touches neither the step counter nor the render history; like
 * ca3d_read_state it joins frames in flight and changes no pixel of a later frame. Returns when the numbers are on the host (one
 * small copy into pinned memory; nothing state-sized moves). Not configured / nothing uploaded: CA3D_ERR_NOT_CONFIGURED.
 *
 * Layouts: PACKED32 — a cell is a bit. UNPACKED — a cell is alive exactly when its word == 1, which is what the legacy step kernel
 * (csrc/ca_unpacked.hip, ca_unpacked_literal: `st == 1u` survives, `st == 0u` may be born, anything else dies) and the legacy
 * renderer (csrc/render_device.inc: `cells[...] == 1u`) take for alive. The digest is over the words as stored, in both layouts.
 *
 * births / deaths compare the current buffer with the other ping-pong buffer, which holds the state one step earlier after every
 * full-grid step path, resident launches included (ca3d_device_buffer). has_previous is 0 — and both counts are 0 — right after
 * ca3d_upload_state / ca3d_configure (a checkpoint load is both), after ca3d_device_buffer handed the buffers out (the caller may
 * have written them) and on the target of ca3d_slab_gather, until the next step. Slab engines: after ca3d_slab_step,
 * ca3d_slab_step_phase(EDGES) + (INTERIOR) and ca3d_slab_run (with and without overlap) through the per-step kernels the owned
 * planes of the other buffer DO hold step - 1 (sub-step n - 1 of a batch of n <= ghost sub-steps still covers every owned plane) and
 * has_previous is 1; it is 0 after a batch that ran as ONE launch of the resident slab kernel (kernel name ca_resident_slab_vn:
 * that launch writes the final state only), also where a slab too thin to split ran it in the EDGES phase. population, box, digest and plane counts are exact on slabs in every case and cover
 * the OWNED planes only (ghosts are never counted). Between the EDGES and the INTERIOR phase of a batch the edge zones have been
 * ping-ponged through both buffers and neither holds a state: the call fails with CA3D_ERR_INVALID_ARGUMENT there.
 *
 * digest: the sum modulo 2^64, over all words w != 0, of mix(i, w), where i is the word's index in the FULL grid's state array (the
 * digests of the slabs of a grid add up to the digest of the grid) and mix is the splitmix64 finaliser of
 * key = ((uint64_t)i << 32) | w (i as a 64-bit integer, the shift modulo 2^64):
 *   z = key + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31.
 * A sum, so the result does not depend on the order workgroups finish in: two runs give the same 64 bits. Equal states have equal
 * digests; it is a quick equality check (and the empty state's digest is 0), NOT a cryptographic one.
 *
 * plane_population (nullable): live cells per owned z plane, nz entries (ca3d_info.nz; entry 0 = plane z0), each <= G^2.
 */
typedef struct ca3d_summary
{
	uint64_t step;          /* ca3d_info.step of the state the numbers describe */
	uint64_t population;    /* live cells (slab engine: owned planes only) */
	uint64_t births;        /* alive now, dead one step earlier */
	uint64_t deaths;        /* dead now, alive one step earlier */
	uint64_t digest;        /* order-independent 64-bit digest, defined above */
	uint32_t has_previous;  /* 1 iff births / deaths are meaningful (step >= 1 and see above); else both are 0 */
	uint32_t box_min[3];    /* x, y, z of the live cells' bounding box, inclusive, GLOBAL cell coordinates */
	uint32_t box_max[3];    /* population == 0: box_min = {G,G,G}, box_max = {0,0,0} */
} ca3d_summary;
int ca3d_summarize(ca3d_t *h, ca3d_summary *out, uint32_t *plane_population);
/* Measurement: hipEvent time of the last ca3d_summarize's clear + kernel on the engine's stream, without the copy back and the host's
 * wait (0 when option "stats" is off or nothing was summarised yet). */
int ca3d_get_summary_time(ca3d_t *h, double *gpu_ms);

/*
 * Run until something happens, without a round trip per step: checks the stop conditions on entry, then repeats
 * { ca3d_step(min(check_every, steps left)); summarise; check } until a condition in stop_mask holds or max_steps steps were taken.
 *   CA3D_STOP_EXTINCT  population == 0
 *   CA3D_STOP_STILL    has_previous && births + deaths == 0: the state is a fixed point of the rule
 * *reason (nullable) receives the bits of stop_mask that fired (0: max_steps reached; both bits if both hold), *steps_done (nullable)
 * the steps taken by this call, *out the last summary. The batches go through ca3d_step itself, so kernel selection (resident kernels
 * for batches of "resident_min" steps and more, captured graphs, option "queue") is what it is for a caller's own ca3d_step(n), and
 * the state afterwards is bit for bit the state after ca3d_step(steps_done). Conditions are only OBSERVED at the check points:
 * steps_done is a multiple of check_every (or max_steps), not the first step at which a condition became true; a state that was still
 * for a step in between and moved again is not noticed (it cannot happen: a fixed point stays one). CA3D_STOP_EXTINCT is not
 * absorbing for rules whose born list contains 0: the empty grid then fills again at the next step.
 * check_every == 0, out == NULL, unknown bits in stop_mask: CA3D_ERR_INVALID_ARGUMENT. Full-grid engines only: a slab engine gets
 * CA3D_ERR_UNSUPPORTED (its neighbours must step with it).
 */
enum
{
	CA3D_STOP_EXTINCT = 1,
	CA3D_STOP_STILL = 2,
	CA3D_STOP_PERIODIC = 4, /* ca3d_step_until_cycle / ca3d_ensemble_step_until_cycle only: the two calls above it refuse the bit */
	CA3D_STOP_MOVING = 8    /* ca3d_ensemble_step_until_moving only: every other call refuses the bit */
};
int ca3d_step_until(ca3d_t *h, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, ca3d_summary *out, uint32_t *steps_done,
                    uint32_t *reason);

/*
 * Stop on a cycle: ca3d_step_until with a third condition, exact period detection.
 *   CA3D_STOP_PERIODIC  the state at a check point equals, bit for bit, the state at an earlier check point of the same call
 * Check points are numbered j = 0 (on entry), 1, 2, ...: every check_every steps, plus a last one at max_steps if that is no multiple.
 * A call keeps ONE anchor, the state at an earlier check point of THIS call, on Brent's schedule: the entry state first; at check
 * points j = 1, 2, 4, 8, ... the anchor moves to the state just checked, AFTER that state was compared with the old anchor. At every
 * check point j > 0 the state is compared with the anchor; if they are equal the call stops with CA3D_STOP_PERIODIC in *reason and
 * *period = steps_done - (the anchor's step). In executable form, with t[k] the state k steps after the call began:
 *     k = j = anchor = 0
 *     loop: fired = (t[k] empty ? EXTINCT : 0) | ((has_previous or k > 0) and t[k] == t[k-1] ? STILL : 0)
 *                 | (j > 0 and t[k] == t[anchor] ? PERIODIC : 0),  fired &= stop_mask
 *           if fired or k == max_steps: return (steps_done = k, reason = fired, period = fired & PERIODIC ? k - anchor : 0)
 *           if j is 0 or a power of two: anchor = k
 *           k += min(check_every, max_steps - k), j += 1
 * What follows from it:
 *   - It is EXACT. Digests and hashes only filter; a stop is declared after a comparison of every word of the two states. No false stops.
 *   - PERIODIC never fires on entry, and the anchor does not survive the call: every call starts from its own entry state.
 *   - *period is a multiple of the true period: lcm(true period, check_every) when the match is at a regular check point, the least
 *     period itself when check_every == 1. 0 when PERIODIC did not fire.
 *   - A fixed point or an empty grid that has reached the anchor reports PERIODIC as well (period: a multiple of check_every), beside
 *     STILL / EXTINCT when those bits are in stop_mask.
 *   - A cycle of period p entered after a transient of m steps is found at step a + lcm(p, check_every), a the first anchor step with
 *     a >= m and the next anchor move at least that lcm away: at most about 3 x max(m, lcm) steps after the start.
 *   - The state afterwards is bit for bit the state after ca3d_step(steps_done), as for the other conditions.
 *   - Patterns that translate are not cycles: nothing is compared modulo shifts (ensembles: ca3d_ensemble_step_until_moving does that).
 * stop_mask: any subset of the three bits. *steps_done, *reason, *period are nullable. The anchor is a device copy of the state,
 * allocated at the first call and freed by ca3d_configure / ca3d_destroy; the filter is the summary's digest, which every check point
 * computes anyway, and equal digests start one compare kernel over the two buffers. Stepping goes through ca3d_step as in
 * ca3d_step_until. Both layouts, any grid; errors as ca3d_step_until (unknown bits: 8 and above). A slab engine: CA3D_ERR_UNSUPPORTED.
 */
int ca3d_step_until_cycle(ca3d_t *h, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, ca3d_summary *out, uint32_t *steps_done,
                          uint32_t *reason, uint32_t *period);

/*
 * Ensemble: B independent 64^3 universes on one device, stepped side by side by ONE kernel launch (no reference counterpart: its UI
 * runs one grid). For hosts that ask "what becomes of this rule / seed?" of thousands of pairs: one ca3d_t steps one universe on one
 * CU of 256 and pays a launch, a rule set-up and a summary pass per universe; here one workgroup holds one universe in its registers
 * (the layout of the engine's own 64^3 resident kernel), a launch is B such workgroups, and every universe has
 *   - its own RULE, as data: the payload of ca3d_set_rules, canonicalised as there, which must reduce to the table pair of the
 *     ENSEMBLE'S NEIGHBOURHOOD — main list von Neumann (7 + 7 table bits, counts 0 .. 6) or Moore (27 + 27 bits, counts 0 .. 26), edges /
 *     corners tables that cannot fire; anything else is refused with CA3D_ERR_UNSUPPORTED and a message that names the universe. The
 *     neighbourhood is chosen when the ensemble is configured and the two kinds never mix in one ensemble: a Moore ensemble refuses a von
 *     Neumann payload and the other way round. Clustered rules as data are out of scope here (a ca3d_t compiles them at run time);
 *   - its own ca3d_summary RECORD, reduced from the registers at the end of every launch: ca3d_ensemble_summarize only copies records
 *     (nothing state-sized moves). Field meanings as above with G = 64; `step` counts the universe's own steps since its last upload,
 *     has_previous is 1 once it has taken one, and the digest's word index is the index in the universe's own array, so a record
 *     equals ca3d_summarize's of a lone engine holding the same universe. No per-plane counts;
 *   - its own END in ca3d_ensemble_step_until, decided inside the kernel: ca3d_step_until's semantics per universe — conditions
 *     checked on entry and after every check_every steps (and after max_steps), steps_done[u] a multiple of check_every or max_steps,
 *     reason[u] the bits of stop_mask that fired (0: max_steps reached), the state of universe u afterwards bit for bit the state
 *     after steps_done[u] plain steps. A universe that stops stops costing anything; its workgroup's CU takes the next universe.
 *     Returns when both arrays (B entries each, nullable) are on the host.
 * grid_size: 64 only, anything else CA3D_ERR_UNSUPPORTED. Call order as for an engine: configure -> set_rules (every universe; universe
 * == CA3D_ENSEMBLE_ALL sets all at once) -> upload_state (every universe) -> step; otherwise CA3D_ERR_NOT_CONFIGURED. Universes are
 * 8192 words each in the engine's PACKED32 layout, `count` of them back to back from universe `first`. An upload resets the uploaded
 * universes' step counters and has_previous. ca3d_ensemble_step steps every universe unconditionally and is asynchronous; calls of any
 * length are cut into launches of at most 65 536 steps. ca3d_ensemble_get_stats describes the last step / step_until call: hipEvent
 * time, launches, steps = the most any universe took, cell_steps = the sum over the universes of the steps each actually took x 64^3.
 * A launch holds the CUs it runs on for up to its whole length: an engine of the same process whose resident multi-step launch needs the
 * whole chip at once ("resident", 512^3 / 256^3) should not run beside one — it would wait, and past "resident_timeout_us" recover
 * through its per-step kernels (ca3d_recovered_launches).
 * One ensemble owns one HIP stream; calls on one handle are not thread-safe. Without a gfx950 device ca3d_ensemble_create fails with
 * CA3D_ERR_DEVICE (there is no CPU fallback); a NULL handle gives CA3D_ERR_INVALID_ARGUMENT without touching a device.
 */
typedef struct ca3d_ensemble ca3d_ensemble_t;
struct ca3d_stats;
#define CA3D_ENSEMBLE_ALL 0xFFFFFFFFu
int ca3d_ensemble_create(int device, ca3d_ensemble_t **out);
int ca3d_ensemble_destroy(ca3d_ensemble_t *e);
int ca3d_ensemble_configure(ca3d_ensemble_t *e, uint32_t grid_size, uint32_t n_universes); /* the CA3D_ENSEMBLE_VON_NEUMANN case of the next one */
/* The neighbourhood every universe of the ensemble counts over (one kernel each: ca_ensemble_vn64, ca_ensemble_moore64). Configuring
 * again replaces universes, rules and neighbourhood. An unknown value: CA3D_ERR_INVALID_ARGUMENT. ca3d_ensemble_get_neighbourhood
 * before any configure: CA3D_ERR_NOT_CONFIGURED. Everything else — upload, seed, read, step, step_until, summarize, get_stats — means
 * in a Moore ensemble what it means in a von Neumann one. */
enum ca3d_ensemble_neighbourhood
{
	CA3D_ENSEMBLE_VON_NEUMANN = 0,
	CA3D_ENSEMBLE_MOORE = 1
};
int ca3d_ensemble_configure_neighbourhood(ca3d_ensemble_t *e, uint32_t grid_size, uint32_t n_universes, int neighbourhood);
int ca3d_ensemble_get_neighbourhood(ca3d_ensemble_t *e, int *out);
/* A CLUSTERED ensemble: every universe is 64^3, its main list is Moore, and it carries the reference's three rule-sets as data — a born /
 * survive table pair each for the 26 Moore neighbours (counts 0 .. 26, the cell itself not counted), the 12 edge neighbours (0 .. 12)
 * and the 8 corner neighbours (0 .. 8). A cell is alive afterwards if ANY of the three lookups says so:
 *   next = (alive ? sM[T] : bM[T]) | (alive ? sE[E] : bE[E]) | (alive ? sC[C] : bC[C])
 * (kernels ca_ensemble_clustered64 / _cycle / _trace). "Clustered" is a property beside the neighbourhood, not a third neighbourhood:
 * ca3d_ensemble_get_neighbourhood answers CA3D_ENSEMBLE_MOORE for such an ensemble and ca3d_ensemble_get_clustered 1 (0 for every other
 * configure; CA3D_ERR_NOT_CONFIGURED before any). The checks are ca3d_ensemble_configure_neighbourhood's.
 *   ca3d_ensemble_set_rules  accepts every payload that canonicalises to main list Moore with the standard edges and corners lists, silent
 *                            side tables included (a plain Moore rule is a clustered rule); the rest — von Neumann or 2D main lists,
 *                            generic lists — is CA3D_ERR_UNSUPPORTED naming the universe. Table bits no count can reach are dropped.
 *   ca3d_ensemble_set_rule_tables  sets the main pair and silences both side pairs.
 *   ca3d_ensemble_set_rule_tables_clustered  three words a rule — main, edges, corners — in born_masks and in survive_masks; n_rules == 1
 *                            (that rule for all `count` universes) or == count. A bit at position 27 / 13 / 9 or above in the respective
 *                            word: CA3D_ERR_INVALID_ARGUMENT naming the universe. Stores what ca3d_ensemble_set_rules stores for the same
 *                            rule and waits for the stream as ca3d_ensemble_set_rule_tables does. In an ensemble that is not clustered:
 *                            CA3D_ERR_UNSUPPORTED.
 * Everything else — upload, seed, read, step, step_until, step_until_cycle, step_until_trace, summarize, get_stats — means what it means
 * in any other ensemble. */
int ca3d_ensemble_configure_clustered(ca3d_ensemble_t *e, uint32_t grid_size, uint32_t n_universes);
int ca3d_ensemble_get_clustered(ca3d_ensemble_t *e, int *out);
int ca3d_ensemble_set_rule_tables_clustered(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *born_masks,
                                            const uint32_t *survive_masks, uint32_t n_rules);
/* The BOUNDARY of every universe of an ensemble: what a step sees behind the six faces of the 64^3 cube.
 *   CA3D_ENSEMBLE_BOUNDARY_REFERENCE  the reference's, and the default: the - faces are dead, the + faces wrap (cell 64 is cell 0, cell -1
 *                                     is no cell), per axis — what every engine path computes and what an ensemble always computed;
 *   CA3D_ENSEMBLE_BOUNDARY_TORUS      all six faces wrap: coordinates are taken modulo 64 on every axis;
 *   CA3D_ENSEMBLE_BOUNDARY_CLOSED     all six faces are dead: a cell outside the cube is never alive.
 * Every axis applies its own boundary to what the axis before it produced, so edge and corner neighbours of a Moore or clustered rule
 * follow the same words (kernels ca_ensemble_<kind>64[_cycle|_trace|_moving]_torus / _closed, beside the reference's twelve). In plain
 * numpy: host.ensemble_step of the Python package.
 * ca3d_ensemble_set_boundary may be called any time after a configure and applies to the launches queued after it; the steps already
 * queued keep the boundary they were queued under. It moves no state, rebuilds no record and waits for nothing. Every
 * ca3d_ensemble_configure* resets the mode to CA3D_ENSEMBLE_BOUNDARY_REFERENCE. An unknown value: CA3D_ERR_INVALID_ARGUMENT; either call
 * before any configure: CA3D_ERR_NOT_CONFIGURED.
 * ca3d_ensemble_step, _step_until, _step_until_cycle, _step_until_moving and _step_until_trace honour the mode, through every launch a
 * long call is cut into. EXTINCT, STILL, PERIODIC, records and samples are defined on the state alone and mean what they always meant.
 * MOVING keeps its definition too — anchor and state both clear of every face, d = box_min(C) - box_min(A) != 0, C equal to A translated
 * by d: in a torus a ship that crossed a seam between anchor and check point is therefore reported with a shift CONGRUENT to its true
 * displacement modulo 64 per axis (a ship that left through x = 63 and went 8 cells reports dx = -56).
 * Census, isolate, compose, canon, the sheet, seeding, upload and read never step and are allowed in every mode (ca3d_ensemble_census
 * and ca3d_ensemble_isolate keep their closed cube in every mode, as do the *_connected calls with CA3D_CONNECT_CLOSED: no face joins
 * objects; CA3D_CONNECT_TORUS is asked for by the caller, never implied by the mode); CA3D_ISOLATE_COPY_RULES and
 * CA3D_COMPOSE_COPY_RULES ignore the boundary of either ensemble.
 * ca3d_ensemble_canon_period steps inside its own kernel with the reference boundary: on an ensemble whose mode is not
 * CA3D_ENSEMBLE_BOUNDARY_REFERENCE it returns CA3D_ERR_UNSUPPORTED and touches nothing. ca3d_ensemble_envelope steps inside its own
 * kernel too and honours the source ensemble's mode, all three. */
enum ca3d_ensemble_boundary
{
	CA3D_ENSEMBLE_BOUNDARY_REFERENCE = 0,
	CA3D_ENSEMBLE_BOUNDARY_TORUS = 1,
	CA3D_ENSEMBLE_BOUNDARY_CLOSED = 2
};
int ca3d_ensemble_set_boundary(ca3d_ensemble_t *e, int boundary);
int ca3d_ensemble_get_boundary(ca3d_ensemble_t *e, int *out);
int ca3d_ensemble_set_rules(ca3d_ensemble_t *e, uint32_t universe,
                            const int32_t *main_offsets, uint32_t n_main,
                            const int32_t *edges_offsets, uint32_t n_edges,
                            const int32_t *corners_offsets, uint32_t n_corners,
                            const uint32_t survive[CA3D_LUT_LEN], const uint32_t born[CA3D_LUT_LEN]);
int ca3d_ensemble_upload_state(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *words, size_t n_words);
int ca3d_ensemble_read_state(ca3d_ensemble_t *e, uint32_t first, uint32_t count, uint32_t *words, size_t n_words);
int ca3d_ensemble_step(ca3d_ensemble_t *e, uint32_t n_steps);
int ca3d_ensemble_step_until(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                             uint32_t *reason);
/* ca3d_step_until_cycle per universe, decided inside the kernel (ca_ensemble_vn64_cycle / ca_ensemble_moore64_cycle): the definition
 * above holds for every universe on its own, with its own anchor (a third per-universe buffer on the device, B x 32 KiB, allocated at
 * the first call with CA3D_STOP_PERIODIC in stop_mask, freed by a configure), also across the launches a long call is cut into. At a
 * check point the workgroup hashes its registers (32 bits) and compares with the anchor's hash; only equal hashes start the comparison
 * of all words, and only that declares a stop. stop_mask: any subset of the three bits; without CA3D_STOP_PERIODIC the call IS
 * ca3d_ensemble_step_until. steps_done, reason, period: B entries each, nullable; period[u] is 0 unless reason[u] holds
 * CA3D_STOP_PERIODIC. Everything else — launch cutting at 65 536 steps, stats, records, readiness errors — as ca3d_ensemble_step_until. */
int ca3d_ensemble_step_until_cycle(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                                   uint32_t *reason, uint32_t *period);
/* Stop on a spaceship: ca3d_ensemble_step_until_cycle with a fourth condition, exact detection of a pattern that reproduced itself
 * somewhere else, decided inside the kernel (ca_ensemble_vn64_moving / ca_ensemble_moore64_moving / ca_ensemble_clustered64_moving).
 *   CA3D_STOP_MOVING  the state at a check point equals the anchor state translated by a vector d != 0, both clear of the faces
 * It is ca3d_ensemble_step_until_cycle's definition, per universe, with the same check points and the same ONE anchor on Brent's
 * schedule, and one more condition evaluated at every check point j > 0. With A the anchor state and C the current state, MOVING holds
 * iff both are non-empty, both bounding boxes lie strictly inside the grid (every box_min >= 1, every box_max <= 62: a pattern on a -
 * face sees the dead boundary and one on a + face wraps, so a match there says nothing about what follows), d = box_min(C) - box_min(A)
 * is not the zero vector, and C equals A translated by d, cell for cell. In the executable form above the line
 *                 | (j > 0 and inside(t[k]) and inside(t[anchor]) and d != 0 and t[k] == translate(t[anchor], d) ? MOVING : 0)
 * joins `fired`, masked by stop_mask like the rest, and the return becomes period = fired & (PERIODIC | MOVING) ? k - anchor : 0,
 * shift = fired & MOVING ? d : (0, 0, 0). What follows from it:
 *   - It is EXACT. Population, box extents and hashes only filter; a stop is declared only after every word has been compared.
 *   - PERIODIC and MOVING exclude each other (d = 0 against d != 0). Either may fire beside EXTINCT or STILL.
 *   - period[u] is a multiple of the ship's true period: lcm(true period, check_every) at a regular check point.
 *   - shift[u] is the displacement over that period; each component lies in -61 .. 61.
 *   - A ship of period p entered after a transient of m steps is found about 3 x max(m, lcm) steps after the start, provided it stays
 *     clear of the faces that long.
 *   - The call proves that the pattern reproduced itself displaced between two check points. It does not prove that the pattern goes
 *     on: it will reach a face.
 *   - MOVING never fires on entry, and the anchor does not survive the call.
 * stop_mask: any subset of the four bits. Without CA3D_STOP_MOVING the call IS ca3d_ensemble_step_until_cycle with the same mask, and
 * without CA3D_STOP_PERIODIC as well ca3d_ensemble_step_until: the launches are those calls' kernels, the results theirs, shift all
 * zero. The three other calls keep refusing the bit. steps_done, reason, period: B entries each; shift: [B][3] (dx, dy, dz); all four
 * nullable. At a check point the workgroup reduces population and bounding box on the check's own barrier; the anchor's are kept beside
 * its step and hash (B x 8 words on the device, allocated at the first call with CA3D_STOP_MOVING in stop_mask, freed by a configure;
 * the anchors themselves are ca3d_ensemble_step_until_cycle's). Equal populations, equal box extents, both boxes inside and d != 0
 * start the comparison of all words against the shifted anchor. A refused call leaves the caller's arrays as they were. Everything
 * else — launch cutting at 65 536 steps, stats, records, readiness errors — as ca3d_ensemble_step_until. */
int ca3d_ensemble_step_until_moving(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                                    uint32_t *reason, uint32_t *period, int32_t *shift /* [B][3]: dx, dy, dz */);
/* ca3d_ensemble_step_until that also RECORDS each universe's population curve, written by the kernel (ca_ensemble_vn64_trace /
 * ca_ensemble_moore64_trace): one sample — population, births, deaths, meaning what they mean in ca3d_summary, births and deaths against
 * the state one step earlier — per check point and universe, with no launch, synchronisation or read-back per sample.
 * The definition. A call (max_steps, check_every, stop_mask) visits the check points of ca3d_ensemble_step_until: steps 0, check_every,
 * 2 check_every ... of the call, and one last at max_steps when max_steps is no multiple of check_every. Check point number j of
 * universe u fills samples[u][j]:
 *   j = 0 (entry): the universe's stored record as it stands — its population, births, deaths; births and deaths are 0 when
 *     has_previous is 0, as after an upload or a seed;
 *   j > 0: from the registers, the current state against the state one step earlier.
 * A universe that stops at a check point has that check point's sample as its last: the sample is taken before the stop decision.
 * n_samples[u] is the number of check points the universe reached, entry included; slots past it are zero.
 * samples: [B][samples_per_universe][3] words (population, births, deaths), required. samples_per_universe must be at least
 * K = ceil(max_steps / check_every) + 1, else CA3D_ERR_INVALID_ARGUMENT with a message that names K; slots K and above are zeroed.
 * steps_done, reason, n_samples: B entries each, nullable. stop_mask: any subset of CA3D_STOP_EXTINCT | CA3D_STOP_STILL; 0 is allowed —
 * nothing stops, every universe has K samples and steps_done[u] == max_steps. CA3D_STOP_PERIODIC is refused here (unknown bits,
 * CA3D_ERR_INVALID_ARGUMENT) as ca3d_ensemble_step_until refuses it. The samples live in a device array on the handle (B x K x 3 words,
 * grown when a call needs more, freed by a configure; CA3D_ERR_OUT_OF_MEMORY when it cannot be had, the other arrays untouched). A
 * refused call leaves the caller's arrays as they were. Everything else — steps_done and reason, states and records after the call,
 * stats, readiness errors, launch cutting at 65 536 steps — as ca3d_ensemble_step_until. */
int ca3d_ensemble_step_until_trace(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                                   uint32_t *reason, uint32_t *samples, uint32_t samples_per_universe, uint32_t *n_samples);
int ca3d_ensemble_summarize(ca3d_ensemble_t *e, uint32_t first, uint32_t count, ca3d_summary *out);
/*
 * The census (no reference counterpart): the connected OBJECTS of universes first .. first + count - 1, one by one — a soup's ash as a
 * list — found by one launch of ca_ensemble_census64 (csrc/ca_census.hip, one workgroup a universe, bit-parallel flood fills in
 * registers) behind whatever is queued on the ensemble's stream. Nothing state-sized leaves the device. host.census restates it.
 *
 * The definition.
 *   Cells and adjacency: the cells are the live bits of the universe's current state. Two live cells are adjacent when they differ by
 *     at most 1 on every axis (the 26-neighbourhood) INSIDE THE CUBE. The census treats the universe as a CLOSED BOX: no face wraps, on
 *     any axis. (The dynamics' + faces wrap and their - faces are dead; that relation is not symmetric and cannot define objects.)
 *   Components and order: a component is a maximal set of cells connected through adjacent cells. A component's first cell is its
 *     cell with the smallest x + 64 y + 4096 z (the bit order of the packed state); components are ordered by their first cells.
 *   With C the number of components: n_components[u] = min(C, max_components); out[u][0 .. n_components[u]) holds the first
 *     components in that order and every slot behind them is zero in every byte; remaining[u] is the number of live cells in no
 *     listed component — 0 exactly when the list is complete. max_components is 1 .. 1024.
 *   The record: population (cells), first_cell (x + 64 y + 4096 z), box_min and box_max (the bounding box, inclusive, each packed
 *     x | y << 8 | z << 16), digest, reserved (zero).
 *   The digest is the `digest` of ca3d_summary for the 64^3 state that holds only this component translated by -box_min
 *     (host.state_summary(64, translated)["digest"]): equal shapes have equal digests wherever they lie. It is not invariant under
 *     rotation, reflection or an oscillator's phase.
 *
 * The call only reads: states, records, step counters, anchors and steps_done are unchanged, and a later step call behaves as if the
 * census had not happened. It needs no rules. It waits for its own result, as ca3d_ensemble_summarize does. gpu_ms (nullable) receives
 * the hipEvent time around the launch. The result is staged in device arrays on the handle (count x max_components records and 2 x
 * count words, grown when a call needs more — the new array is allocated before the old one is freed, so CA3D_ERR_OUT_OF_MEMORY leaves
 * the handle as it was — freed by a configure and by destroy).
 *
 * Errors: NULL handle, out, n_components or remaining — CA3D_ERR_INVALID_ARGUMENT without touching a device; not configured —
 * CA3D_ERR_NOT_CONFIGURED; count == 0, first + count > n, max_components outside 1 .. 1024 — CA3D_ERR_INVALID_ARGUMENT; a universe
 * of the range without a state — CA3D_ERR_NOT_CONFIGURED, the message names the first such universe. A refused call touches none of
 * the caller's arrays.
 */
typedef struct ca3d_component
{
	uint32_t population;
	uint32_t first_cell;       /* x + 64 y + 4096 z of the component's lowest cell */
	uint32_t box_min, box_max; /* x | y << 8 | z << 16, inclusive */
	uint64_t digest;           /* of the component translated by -box_min */
	uint32_t reserved[2];      /* zero */
} ca3d_component;              /* 32 bytes */
int ca3d_ensemble_census(ca3d_ensemble_t *e, uint32_t first, uint32_t count, uint32_t max_components, ca3d_component *out /* [count][max_components] */,
                         uint32_t *n_components /* [count] */, uint32_t *remaining /* [count] */, float *gpu_ms /* may be NULL */);
/*
 * Isolate (no reference counterpart): an object a census named becomes the only thing in a universe of its own, with room around it
 * and the rule of the universe it came from, without a state leaving the device — ca3d_ensemble_step_until_cycle, _moving, _trace and
 * ca3d_ensemble_render_sheet then classify and draw every object of every soup side by side. One launch of ca_ensemble_isolate64
 * (csrc/ca_isolate.hip, one workgroup a job: the census' flood fill, then a translated write). host.isolate restates it.
 *
 * The definition. Job k writes universe dst_first + k of `dst`. Its state becomes the connected component of universe jobs[k].universe
 *   of `src` that contains the cell jobs[k].cell (x + 64 y + 4096 z) — connectivity is the census': the 26-neighbourhood inside the
 *   closed cube, no face wraps — translated by `shift`, and everything else is zero. ANY live cell of the object selects it, not only
 *   the census' first_cell. A dead cell gives an empty universe, population 0 and a zero shift.
 *   The shift, with the component's box (min, max) and extent e = max - min + 1 per axis, by the placement in the low byte of `flags`:
 *     CA3D_ISOLATE_KEEP    0: the object stays where it was;
 *     CA3D_ISOLATE_ORIGIN  -min: the state's ca3d_summary digest is then the census record's digest;
 *     CA3D_ISOLATE_CENTRE  (64 - e) / 2 - min (integer division): about 30 cells of room each way for a small object.
 *   The translated box is always inside the cube: nothing is clipped.
 *   Both ping-pong buffers get the words, as with upload and seed; the destination universes' records are rebuilt at step 0 with no
 *   previous state (the launch ca3d_ensemble_upload_state ends in), and those universes count as having a state.
 *   CA3D_ISOLATE_COPY_RULES copies the source universe's stored rule words to the destination universe on the device: `src` and `dst`
 *   must have the same neighbourhood and the same clustered property, every source universe named must have rules, and the
 *   destinations count as having rules afterwards. Without the flag rules are untouched and the two ensembles may differ in kind.
 *   out[k] (nullable array): the object's population and the shift applied.
 *
 * `src` and `dst` may be the same handle or two handles on the same device; when they are the same no job's universe may lie in
 * [dst_first, dst_first + n_jobs). The launch runs on dst's stream behind what is queued there and behind what is queued on src's
 * stream at the time of the call (an event recorded there, waited for on dst's). The call waits for its own result, as
 * ca3d_ensemble_census does, so src may go on afterwards; src's states, records and counters are only read. gpu_ms (nullable) receives
 * the hipEvent time around the launch. Jobs and results are staged in one device array on dst's handle (24 bytes a job, grown when a
 * call needs more — the new array is allocated before the old one is freed — freed by a configure and by destroy).
 *
 * Errors — a refused call touches neither ensemble nor `out`, and names the job where there is one: a NULL handle or jobs, n_jobs == 0
 * or more jobs than fit behind dst_first, a `universe` out of range, cell >= 1 << 18, an unknown placement or flag bit, handles on
 * different devices, a source universe among the destinations — CA3D_ERR_INVALID_ARGUMENT; either ensemble not configured, a source
 * universe without a state, with CA3D_ISOLATE_COPY_RULES one without rules — CA3D_ERR_NOT_CONFIGURED; with CA3D_ISOLATE_COPY_RULES
 * ensembles of different kinds — CA3D_ERR_UNSUPPORTED.
 */
typedef struct ca3d_isolate_job
{
	uint32_t universe; /* of src */
	uint32_t cell;     /* x + 64 y + 4096 z: any cell of the object */
} ca3d_isolate_job;
typedef struct ca3d_isolated
{
	uint32_t population;
	int32_t shift[3]; /* dx, dy, dz applied */
} ca3d_isolated;      /* 16 bytes */
enum
{
	CA3D_ISOLATE_KEEP = 0,
	CA3D_ISOLATE_CENTRE = 1,
	CA3D_ISOLATE_ORIGIN = 2
}; /* placement: the low byte of flags */
#define CA3D_ISOLATE_COPY_RULES 0x100u
int ca3d_ensemble_isolate(ca3d_ensemble_t *dst, uint32_t dst_first, ca3d_ensemble_t *src, uint32_t n_jobs, const ca3d_isolate_job *jobs, uint32_t flags,
                          ca3d_isolated *out /* [n_jobs], may be NULL */, float *gpu_ms /* may be NULL */);
/*
 * Census and isolate with the connectivity named (no reference counterpart): on a torus ensemble (CA3D_ENSEMBLE_BOUNDARY_TORUS) an
 * object that lies on a face is one object, not two fragments. `connectivity` is a parameter of these two calls, not a flag and not
 * implied by the ensemble's boundary mode. An unknown value: CA3D_ERR_INVALID_ARGUMENT, nothing is touched, the message names the value.
 *
 * CA3D_CONNECT_CLOSED: the two calls ARE ca3d_ensemble_census and ca3d_ensemble_isolate — the same kernels, the same bytes out; those
 *   two entry points are calls of these with CA3D_CONNECT_CLOSED.
 * CA3D_CONNECT_TORUS (kernels ca_ensemble_census64_torus / ca_ensemble_isolate64_torus, csrc/ca_objects_torus.hip; host.census and
 *   host.isolate with connectivity="torus" restate them):
 *   Adjacency: two live cells are adjacent when they differ by at most 1 MODULO 64 on every axis, the 26-neighbourhood of Z_64^3.
 *     Components, first_cell (the smallest x + 64 y + 4096 z of the component), the order of the list, n_components, remaining and the
 *     zeroed slots are defined as for ca3d_ensemble_census.
 *   The box, per axis, with S the set of coordinates (a subset of Z_64) the component occupies: box_min is the start s in S of the
 *     shortest cyclic interval {s, ..., s + e - 1 mod 64} that covers S, ties going to the smallest s; box_max = box_min + e - 1, NOT
 *     reduced: it is >= 64 on an axis exactly when the box runs through that axis' seam, the cell is at box_max & 63, and the 8-bit
 *     fields hold up to 126. S = all 64 gives box_min = 0, box_max = 63. (A connected component's S is a single cyclic run, adjacent
 *     cells differing by at most 1 on the axis: the start is the one coordinate of S whose predecessor is not in S, and e = |S|.)
 *   The digest is the ca3d_summary digest of the 64^3 state that holds only the component, translated CYCLICALLY by -box_min: equal
 *     shapes have equal digests wherever they lie, across seams too, and a shape clear of the faces has the digest the closed census
 *     gives it. This fails only for a component that spans a whole ring (e = 64 on an axis): along that axis nothing is translated,
 *     so two such components that differ by a translation along the ring have different digests.
 *   Isolate takes the torus component that holds the job's cell. The shift is ca3d_ensemble_isolate's formula on the torus box —
 *     KEEP 0, ORIGIN -min, CENTRE (64 - e) / 2 - min, within -63 .. 31 as there — applied MODULO 64: the destination holds the object
 *     in one piece, unwrapped unless it spans a ring, and nothing is clipped. out[k].shift is the formula's value. A dead cell gives
 *     an empty universe and a zero shift. With ORIGIN the state's ca3d_summary digest is the torus census record's digest.
 * Everything else — both buffers written, records rebuilt at step 0, CA3D_ISOLATE_COPY_RULES, unknown flag bits refused, ordering across
 * streams, staging, gpu_ms, every other refusal — is ca3d_ensemble_census' and ca3d_ensemble_isolate's.
 */
enum
{
	CA3D_CONNECT_CLOSED = 0,
	CA3D_CONNECT_TORUS = 1
};
int ca3d_ensemble_census_connected(ca3d_ensemble_t *e, uint32_t first, uint32_t count, uint32_t max_components, uint32_t connectivity,
                                   ca3d_component *out /* [count][max_components] */, uint32_t *n_components /* [count] */,
                                   uint32_t *remaining /* [count] */, float *gpu_ms /* may be NULL */);
int ca3d_ensemble_isolate_connected(ca3d_ensemble_t *dst, uint32_t dst_first, ca3d_ensemble_t *src, uint32_t n_jobs, const ca3d_isolate_job *jobs,
                                    uint32_t flags, uint32_t connectivity, ca3d_isolated *out /* [n_jobs], may be NULL */,
                                    float *gpu_ms /* may be NULL */);
/*
 * Compose (no reference counterpart): the inverse of isolate. A destination universe becomes the union of several pieces, each the
 * WHOLE current state of a source universe — usually an isolated object — turned by one of the 48 symmetries of the cube and put where
 * the caller says, without a state leaving the device: a glider thrown at a block from every direction, two ships on a collision
 * course, an object dropped into a living soup. One launch of ca_ensemble_compose64 (csrc/ca_compose.hip, one workgroup a destination)
 * for all destinations of a call. host.compose restates it in plain numpy; host.orientation_matrix, orientation_from_matrix and
 * orient_vector speak about the orientations.
 *
 * The definition. Destination dst_first + k of `dst` takes parts part_begin[k] .. part_begin[k + 1] - 1; part_begin[0] is 0 and the
 *   array does not decrease. A destination with no parts becomes empty, or stays as it is under CA3D_COMPOSE_OVER.
 *   Orientation o is a signed permutation: perm = PERMS[o % 6] with PERMS = (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0), and
 *   bit i of f = o / 6 mirrors OUTPUT axis i. With the piece's bounding box (min, max) and extent e = max - min + 1, a live cell c of
 *   the piece goes to q + at, where
 *     r[i] = c[perm[i]] - min[perm[i]],   e'[i] = e[perm[i]],   q[i] = e'[i] - 1 - r[i] when bit i of f is set, else r[i]:
 *   `at` is where box_min of the TURNED piece goes. The cell is set when all three coordinates lie in 0 .. 63; otherwise it counts as
 *   clipped. An empty piece contributes nothing. Orientation 0 with at = min reproduces the piece; the 24 orientations whose matrix
 *   has determinant +1 are the rotations, the other 24 reflections.
 *   The result is the OR of the base (zero, or the destination's current state under CA3D_COMPOSE_OVER) and all parts: it does not
 *   depend on the order of the parts. Both ping-pong buffers get the words; the destinations' records are rebuilt at step 0 with no
 *   previous state (the launch ca3d_ensemble_upload_state and ca3d_ensemble_isolate end in), and they count as having a state.
 *   CA3D_COMPOSE_COPY_RULES: a destination takes the stored rule words of its FIRST part's source universe, on the device, under
 *   isolate's conditions — both ensembles of one kind, every source universe named by a first part with rules; those destinations
 *   count as having rules afterwards. A destination without parts keeps the rules it has.
 *   out[k] (nullable array): population of the destination afterwards; placed, the cells of its parts that landed inside the cube,
 *   summed over the parts; overlap = base population + placed - population, the cells that landed on a live cell; clipped, the cells
 *   of its parts that fell outside the cube (all four modulo 2^32).
 *
 * `src` and `dst` may be the same handle or two handles on the same device; when they are the same no part's universe may lie in
 * [dst_first, dst_first + n_dst). Ordering is isolate's: the launch runs on dst's stream behind what is queued there and behind what
 * is queued on src's stream at the time of the call, and the call waits for dst's stream. gpu_ms (nullable) receives the hipEvent time
 * around the launch. Records, parts and part_begin are staged in one device array on dst's handle (grown when a call needs more,
 * freed by a configure and by destroy).
 *
 * Errors — everything is checked before anything is queued; a refused call touches neither ensemble nor `out`: a NULL handle, a NULL
 * part_begin, NULL parts where there are parts, n_dst == 0 or more destinations than fit behind dst_first, part_begin[0] != 0 or a
 * decreasing part_begin, more than 1 << 20 parts, a `universe` out of range, orientation >= 48, an `at` outside -64 .. 64, reserved
 * != 0, an unknown flag bit, handles on different devices, a source universe among the destinations — CA3D_ERR_INVALID_ARGUMENT;
 * either ensemble not configured, a source universe without a state, CA3D_COMPOSE_OVER on a destination without a state, with
 * CA3D_COMPOSE_COPY_RULES a first part's source without rules — CA3D_ERR_NOT_CONFIGURED; with CA3D_COMPOSE_COPY_RULES ensembles of
 * different kinds — CA3D_ERR_UNSUPPORTED.
 */
typedef struct ca3d_compose_part
{
	uint32_t universe;    /* of src: its whole current state is the piece */
	uint32_t orientation; /* 0 .. 47 */
	int32_t at[3];        /* x, y, z: where box_min of the TURNED piece goes; -64 .. 64 each */
	uint32_t reserved;    /* 0 */
} ca3d_compose_part;      /* 24 bytes */
typedef struct ca3d_composed
{
	uint32_t population; /* of the destination afterwards */
	uint32_t placed;     /* cells of its parts that landed inside the cube, summed over parts */
	uint32_t overlap;    /* base population + placed - population: cells that landed on a live cell */
	uint32_t clipped;    /* cells of its parts that fell outside the cube */
} ca3d_composed;         /* 16 bytes */
#define CA3D_COMPOSE_OVER 0x1u         /* start from the destination's current state, not from zero */
#define CA3D_COMPOSE_COPY_RULES 0x100u /* a destination takes the rule of its FIRST part's source universe */
#define CA3D_COMPOSE_MAX_PARTS (1u << 20)
int ca3d_ensemble_compose(ca3d_ensemble_t *dst, uint32_t dst_first, uint32_t n_dst, ca3d_ensemble_t *src, const ca3d_compose_part *parts,
                          const uint32_t *part_begin /* [n_dst + 1] */, uint32_t flags, ca3d_composed *out /* [n_dst], may be NULL */,
                          float *gpu_ms /* may be NULL */);
/*
 * Canon (no reference counterpart): a universe's name up to the 48 symmetries of the cube and any translation, so that a census becomes
 * a catalogue — a glider flying along +x+y and one flying along -z+x, or the 24 turned copies of a still life, get ONE key. One launch
 * of ca_ensemble_canon64 (csrc/ca_canon.hip, one workgroup a universe) for universes first .. first + count - 1, behind whatever is
 * queued on the ensemble's stream. Nothing state-sized leaves the device. host.canon restates it in plain numpy;
 * host.symmetry_orientations and host.is_chiral read the symmetry mask.
 *
 * The definition. For the packed 64^3 state S of a universe and an orientation o in 0 .. 47 (ca3d_ensemble_compose's numbering), T_o(S)
 *   is S turned by o with the turned bounding box's minimum at the origin: what ca3d_ensemble_compose makes of the one part
 *   (universe, o, at = (0, 0, 0)). T_0(S) is S translated to the origin. Nothing is ever clipped.
 *   digests[o] is the `digest` of ca3d_summary for T_o(S): the digest_mix sum over the non-zero words, word index (z * 64 + y) * 2 + h.
 *     For a universe that holds one object digests[0] is that object's census digest.
 *   key is the smallest of the 48 digests as an unsigned 64-bit number; orientation the smallest o with digests[o] == key. The key is
 *     equal for all 48 turned and arbitrarily translated copies of a state (they have the same 48 states T_o, in another order).
 *   symmetry has bit o set exactly when T_o(S) equals T_0(S) WORD FOR WORD — an exact comparison, never one of digests: the symmetry
 *     group of the state in the numbering of the orientations. Bit 0 is always set; bits 48 .. 63 are zero.
 *   population, box_min and box_max are those of a census record: the live cells, and the bounding box of S, inclusive, each corner
 *     packed x | y << 8 | z << 16.
 *   An empty universe gives key 0, orientation 0, symmetry 2^48 - 1, population 0 and both boxes 0.
 *   The call works on the WHOLE state of a universe, as compose does: several objects in one universe are one constellation with one
 *   key. It is not invariant under an oscillator's or a ship's phase (Ensemble.canon_phases takes the smallest key over a period).
 *
 * The call only reads: states, records, step counters, anchors and steps_done are unchanged. It needs no rules. It waits for its own
 * result, as ca3d_ensemble_census does. digests (nullable) receives all 48 digests of every universe: the minimum alone would hide a
 * wrong digest in 47 of 48 orientations. gpu_ms (nullable) receives the hipEvent time around the launch. The result is staged in one
 * device array on the handle (32 + 384 bytes a universe, grown when a call needs more — the new array is allocated before the old one
 * is freed — freed by a configure and by destroy).
 *
 * Errors: NULL handle or out — CA3D_ERR_INVALID_ARGUMENT without touching a device; not configured — CA3D_ERR_NOT_CONFIGURED;
 * count == 0, first + count > n — CA3D_ERR_INVALID_ARGUMENT; a universe of the range without a state — CA3D_ERR_NOT_CONFIGURED, the
 * message names the first such universe. A refused call touches none of the caller's arrays.
 */
typedef struct ca3d_canon
{
	uint64_t key;              /* the smallest of the 48 digests */
	uint64_t symmetry;         /* bit o: T_o equals T_0 word for word */
	uint32_t orientation;      /* the smallest o whose digest is the key */
	uint32_t population;
	uint32_t box_min, box_max; /* of the state as it lies: x | y << 8 | z << 16, inclusive */
} ca3d_canon;                  /* 32 bytes */
int ca3d_ensemble_canon(ca3d_ensemble_t *e, uint32_t first, uint32_t count, ca3d_canon *out /* [count] */,
                        uint64_t *digests /* [count][48], may be NULL */, float *gpu_ms /* may be NULL */);
/*
 * Canon over a period (no reference counterpart): what moves or oscillates named as still lifes are — all phases of a glider, in all 48
 * orientations, get ONE key — with the proof that the period given closes. One launch of ca_ensemble_canon_period_vn64, _moore64 or
 * _clustered64 (csrc/ca_canon_period.hip, by the ensemble's kind, one workgroup a universe) for universes first .. first + count - 1,
 * behind whatever is queued on the ensemble's stream. Universe first + k is followed over periods[k] steps of its own INSIDE the
 * kernel; nothing is written back to the ensemble. host.canon_period restates it in plain numpy over host.canon.
 *
 * The definition. Let S_0 be the universe's current state and S_t what the ensemble's own step makes of it after t steps: the
 *   universe's rule, - faces dead, + faces wrapping, exactly as ca3d_ensemble_step does. k_t is ca3d_ensemble_canon's record of S_t.
 *   key is the smallest k_t.key for t < period, as an unsigned 64-bit number; phase the smallest t that reaches it; orientation,
 *     symmetry and population are that k_t's.
 *   keys[u][t] is k_t.key for t < period; the slots from period up to keys_stride are zero. keys is part of the interface on purpose,
 *     as digests is for canon: the minimum alone would hide a wrong key in all phases but one.
 *   CLOSED (bit 0 of flags_shift) is set exactly when T_0(S_period) equals T_0(S_0) WORD FOR WORD, T_0 being canon's "translated to
 *     the origin" — a comparison of words, never of digests. The state is then back up to a translation, and the period given is a
 *     multiple of the true one.
 *   dx, dy, dz (bits 8 .. 15, 16 .. 23, 24 .. 31 of flags_shift, signed bytes) are box_min(S_period) - box_min(S_0) per axis when CLOSED
 *     is set and S_0 is not empty, and zero otherwise. (0, 0, 0) with CLOSED is an oscillator or a still life, anything else a ship.
 *   An empty S_0 gives key 0, phase 0, symmetry 2^48 - 1, population 0 and shift 0; CLOSED is then set exactly when S_period is empty.
 *   A ship that meets a face within the period is whatever the definition gives: usually not CLOSED.
 *
 * The call only reads: states, records, step counters, anchors, steps_done and stats are unchanged. It needs a rule on every universe
 * of the range. It waits for its own result, as ca3d_ensemble_canon does. gpu_ms (nullable) receives the hipEvent time around the
 * launch. The result is staged in canon's device array on the handle: the records, count * keys_stride keys, then the periods.
 *
 * Errors: NULL handle, periods or out — CA3D_ERR_INVALID_ARGUMENT without touching a device; not configured — CA3D_ERR_NOT_CONFIGURED;
 * count == 0, first + count > n, a period of 0 or above CA3D_CANON_MAX_PERIOD, keys given with keys_stride < max(periods) —
 * CA3D_ERR_INVALID_ARGUMENT; a universe of the range without a state, or without a rule — CA3D_ERR_NOT_CONFIGURED, the message names
 * the first such universe. A refused call touches none of the caller's arrays.
 */
#define CA3D_CANON_CLOSED 1u          /* flags_shift bit 0 */
#define CA3D_CANON_MAX_PERIOD 4096u
typedef struct ca3d_canon_period
{
	uint64_t key;          /* smallest ca3d_canon key over phases t = 0 .. period - 1 */
	uint64_t symmetry;     /* of the smallest t that reaches the key */
	uint32_t orientation;  /* likewise */
	uint32_t phase;        /* that t */
	uint32_t population;   /* of that phase */
	uint32_t flags_shift;  /* bit 0 CLOSED; bits 8..15, 16..23, 24..31: dx, dy, dz as int8 */
} ca3d_canon_period;       /* 32 bytes */
int ca3d_ensemble_canon_period(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *periods /* [count] */,
                               ca3d_canon_period *out /* [count] */, uint64_t *keys /* [count][keys_stride], may be NULL */,
                               uint32_t keys_stride, float *gpu_ms /* may be NULL */);
/*
 * Envelope over a period (no reference counterpart): HOW a universe oscillates — which cells ever live, which always live, which
 * change, and how much changes a step. One launch of ca_ensemble_envelope_{vn,moore,clustered}64[_torus|_closed]
 * (csrc/ca_envelope.hip, by the source ensemble's kind and its CURRENT boundary mode, one workgroup a universe) for universes
 * first .. first + count - 1 of `src`. Universe first + k is followed over periods[k] steps of its own INSIDE the kernel; nothing is
 * written back to `src`. host.envelope restates it in plain numpy over host.ensemble_step.
 *
 * The definition. For universe first + k let P = periods[k], 1 <= P <= CA3D_CANON_MAX_PERIOD, S_0 its current state and S_t what the
 *   ensemble's own step makes of it after t steps: the universe's rule and the ensemble's current boundary mode (reference, torus or
 *   closed), exactly as ca3d_ensemble_step does.
 *   E = S_0 | ... | S_(P-1) is the envelope, A = S_0 & ... & S_(P-1) the stator, E & ~A the rotor.
 *   heat = sum over t = 0 .. P - 1 of popcount(S_t ^ S_(t+1)); S_P is computed for it. At most 2^18 * 2^12 = 2^30.
 *   population_sum = sum over t < P of popcount(S_t). envelope_population = popcount(E), stator_population = popcount(A).
 *   envelope_min / envelope_max and rotor_min / rotor_max are the inclusive bounding boxes of E and of the rotor, x, y, z and a zero
 *     byte; an empty set has min = max = 0.
 *   flags bit 0, CA3D_ENVELOPE_RETURNS, is set exactly when S_P equals S_0 WORD FOR WORD: no translation and no digests are involved.
 *     An oscillator whose period divides P returns; a ship gives its swept volume and no RETURNS.
 *   period echoes P. The two reserved words are zero.
 *   The rest follows on the host: rotor_population = envelope_population - stator_population, volatility = rotor / envelope,
 *   heat / period.
 *
 * Images. `flags` selects any subset of CA3D_ENVELOPE_IMAGE_ENVELOPE, _STATOR and _ROTOR. With n images selected, source k writes
 *   them in bit order (envelope, stator, rotor) into universes dst_first + k * n + i of `dst`, which is `src` itself or a second
 *   ensemble on the same device: both ping-pong buffers are written and the records rebuilt at step 0, as ca3d_ensemble_isolate
 *   does. CA3D_ENVELOPE_COPY_RULES copies the source universe's rule words to each of its destinations as CA3D_ISOLATE_COPY_RULES
 *   does: `src` and `dst` must then be of one kind. The boundary of `dst` is not looked at. With no image bit set `dst` must be NULL.
 *
 * Ordering. The launch runs behind what is queued on both ensembles' streams, on the destination's when there is one. `src` is only
 * read: states, records, step counters, anchors, steps_done and stats are unchanged. It needs a rule on every universe of the range.
 * The call waits for its own result. gpu_ms (nullable) receives the hipEvent time around the launch. Records and periods are staged in
 * a device array of the call's own on the handle the launch runs on.
 *
 * Errors: NULL `src`, periods or out — CA3D_ERR_INVALID_ARGUMENT without touching a device; `src` (or `dst`) not configured —
 * CA3D_ERR_NOT_CONFIGURED; count == 0, first + count > n, a period of 0 or above CA3D_CANON_MAX_PERIOD, unknown bits in flags, image
 * bits without `dst` or `dst` without image bits, destinations past dst's n, a source universe among the destinations of the same
 * ensemble, different devices — CA3D_ERR_INVALID_ARGUMENT; a universe of the range without a state, or without a rule —
 * CA3D_ERR_NOT_CONFIGURED, the message names the first such universe; CA3D_ENVELOPE_COPY_RULES across kinds — CA3D_ERR_UNSUPPORTED. A
 * refused call touches none of the caller's arrays and nothing on the device.
 */
#define CA3D_ENVELOPE_RETURNS 1u /* ca3d_envelope.flags bit 0 */
#define CA3D_ENVELOPE_IMAGE_ENVELOPE 1u
#define CA3D_ENVELOPE_IMAGE_STATOR 2u
#define CA3D_ENVELOPE_IMAGE_ROTOR 4u
#define CA3D_ENVELOPE_COPY_RULES 0x100u
typedef struct ca3d_envelope
{
	uint32_t period;              /* echoed */
	uint32_t flags;               /* bit 0 CA3D_ENVELOPE_RETURNS */
	uint32_t heat;                /* cells changed, summed over the P steps */
	uint32_t population_sum;      /* of S_0 .. S_(P-1) */
	uint32_t envelope_population;
	uint32_t stator_population;
	uint8_t envelope_min[4], envelope_max[4]; /* x, y, z, 0: inclusive; both zero for an empty set */
	uint8_t rotor_min[4], rotor_max[4];
	uint32_t reserved[2];         /* zero */
} ca3d_envelope;                  /* 48 bytes */
int ca3d_ensemble_envelope(ca3d_ensemble_t *src, uint32_t first, uint32_t count, const uint32_t *periods /* [count] */,
                           ca3d_ensemble_t *dst /* NULL without images */, uint32_t dst_first, uint32_t flags,
                           ca3d_envelope *out /* [count] */, float *gpu_ms /* may be NULL */);
/*
 * Damage spreading (no reference counterpart): flip a cell — does the difference die out, stay put, or take over the universe? The
 * Hamming distance between a state and a perturbed twin over time, the standard classifier of ordered, critical and chaotic rules.
 * One launch of ca_ensemble_damage_{vn,moore,clustered}64[_torus|_closed] (csrc/ca_damage.hip, by the source ensemble's kind and its
 * CURRENT boundary mode, one workgroup a universe) for universes first .. first + count - 1 of `src`. Both trajectories of universe
 * first + k are followed over steps[k] steps INSIDE the kernel; nothing is written back to `src`. host.damage restates it in plain
 * numpy over host.ensemble_step.
 *
 * The definition. For source universe u = first + k let P = steps[k], 1 <= P <= CA3D_CANON_MAX_PERIOD, and S_0 its current state.
 *   The twin starts as T_0 = W ^ F. W is S_0 when twins is NULL or twins[k] == CA3D_DAMAGE_SELF, else the current state of universe
 *   twins[k] of the same ensemble. F has exactly the cells of flips[k][0 .. CA3D_DAMAGE_FLIPS - 1] set, XORed in one after another,
 *   so a cell listed twice cancels; a flip is x | y << 8 | z << 16 with x, y, z < 64, or CA3D_DAMAGE_NO_FLIP; flips == NULL: none.
 *   S_(t+1) = step(S_t) and T_(t+1) = step(T_t) by the ensemble's own step: u's rule (a twin's rule is never read) and the ensemble's
 *   current boundary mode (reference, torus or closed), exactly as ca3d_ensemble_step does.
 *   D_t = S_t ^ T_t and d_t = popcount(D_t) for t = 0 .. P.
 *   steps echoes P. flags bit 0, CA3D_DAMAGE_HEALED, is set exactly when some d_t == 0 with t <= P, and healed_at is the first such
 *   t, 0xFFFFFFFF if none: from there on the trajectories are equal for good, every later sample is 0 and D_P is empty. (A kernel may
 *   stop stepping there; the definition does not depend on whether it does.)
 *   final_distance = d_P, initial_distance = d_0, max_distance the largest d_t and max_at the first t that reaches it,
 *   distance_sum = the sum of d_t over t = 0 .. P: at most 262 144 * 4 097 = 1 074 003 968, which fits a word.
 *   damage_min / damage_max are the inclusive bounding box of D_P, touched_min / touched_max that of D_0 | ... | D_P, the cone the
 *   damage swept: x, y, z and a zero byte; an empty set has min = max = 0.
 *
 * The curve. With curve != NULL, curve[k * curve_stride + t] = d_t for t <= P and 0 for P < t < curve_stride;
 *   curve_stride >= max(steps) + 1. curve_stride is not looked at when curve is NULL.
 *
 * The image. CA3D_DAMAGE_IMAGE_DAMAGE writes D_P as universe dst_first + k of `dst`, which is `src` itself or a second ensemble on the
 *   same device: both ping-pong buffers are written and the records rebuilt at step 0, as ca3d_ensemble_envelope's images are.
 *   CA3D_DAMAGE_COPY_RULES copies u's rule words to its destination as CA3D_ENVELOPE_COPY_RULES does: `src` and `dst` must then be of
 *   one kind. The boundary of `dst` is not looked at. Without the image bit `dst` must be NULL.
 *
 * Ordering. The launch runs behind what is queued on both ensembles' streams, on the destination's when there is one. `src` is only
 * read: states, records, step counters, anchors, steps_done and stats are unchanged. It needs a state on every source and twin
 * universe and a rule on every source universe. The call waits for its own result. gpu_ms (nullable) receives the hipEvent time around
 * the launch. Records, curve, steps, twins and flips are staged in a device array of the call's own on the handle the launch runs on.
 *
 * Errors: NULL `src`, steps or out — CA3D_ERR_INVALID_ARGUMENT without touching a device; `src` (or `dst`) not configured —
 * CA3D_ERR_NOT_CONFIGURED; count == 0, first + count > n, a step count of 0 or above CA3D_CANON_MAX_PERIOD, a twin that is neither
 * CA3D_DAMAGE_SELF nor a universe of `src`, a flip that is neither CA3D_DAMAGE_NO_FLIP nor three coordinates below 64 with a zero top
 * byte, curve with curve_stride < max(steps) + 1, unknown bits in flags, the image bit without `dst`, `dst` without the image bit,
 * CA3D_DAMAGE_COPY_RULES without the image bit, destinations past dst's n, a source or twin universe among the destinations of the
 * same ensemble, different devices — CA3D_ERR_INVALID_ARGUMENT; a source or twin universe without a state, a source universe without
 * a rule — CA3D_ERR_NOT_CONFIGURED; CA3D_DAMAGE_COPY_RULES across kinds — CA3D_ERR_UNSUPPORTED. Each message names its argument and
 * the first offending universe. A refused call touches none of the caller's arrays and nothing on the device.
 */
#define CA3D_DAMAGE_HEALED 1u /* ca3d_damage.flags bit 0 */
#define CA3D_DAMAGE_FLIPS 4u  /* flip words a universe */
#define CA3D_DAMAGE_SELF 0xFFFFFFFFu
#define CA3D_DAMAGE_NO_FLIP 0xFFFFFFFFu
#define CA3D_DAMAGE_IMAGE_DAMAGE 1u
#define CA3D_DAMAGE_COPY_RULES 0x100u
typedef struct ca3d_damage
{
	uint32_t steps;            /* echoed */
	uint32_t flags;            /* bit 0 CA3D_DAMAGE_HEALED */
	uint32_t healed_at;        /* the first t with d_t == 0; 0xFFFFFFFF if none */
	uint32_t final_distance;   /* d_P */
	uint32_t initial_distance; /* d_0 */
	uint32_t max_distance;     /* the largest d_t */
	uint32_t max_at;           /* the first t that reaches it */
	uint32_t distance_sum;     /* of d_0 .. d_P */
	uint8_t damage_min[4], damage_max[4];   /* of D_P: x, y, z, 0: inclusive; both zero for an empty set */
	uint8_t touched_min[4], touched_max[4]; /* of D_0 | ... | D_P */
} ca3d_damage;                 /* 48 bytes */
int ca3d_ensemble_damage(ca3d_ensemble_t *src, uint32_t first, uint32_t count, const uint32_t *steps /* [count] */,
                         const uint32_t *twins /* [count] or NULL */, const uint32_t *flips /* [count][CA3D_DAMAGE_FLIPS] or NULL */,
                         ca3d_ensemble_t *dst /* NULL without the image */, uint32_t dst_first, uint32_t flags,
                         ca3d_damage *out /* [count] */, uint32_t *curve /* [count][curve_stride], may be NULL */,
                         uint32_t curve_stride, float *gpu_ms /* may be NULL */);
/*
 * Rule usage (no reference counterpart): which entries of its born / survive tables does a universe's run actually read? Two rules
 * that differ only in entries a seed never reads have the same trajectory; the histogram of neighbour counts, split by alive and
 * dead, is the input of every mean-field estimate; births and deaths follow from it and the table alone. One launch of
 * ca_ensemble_usage_{vn,moore,clustered}64[_torus|_closed] (csrc/ca_usage.hip, by the ensemble's kind and its CURRENT boundary mode,
 * one workgroup a universe) for universes first .. first + count - 1. Universe first + k is followed over steps[k] steps INSIDE the
 * kernel; nothing is written back to the ensemble. host.usage restates it in plain numpy over host.ensemble_step.
 *
 * The definition. For universe u = first + k let P = steps[k], 1 <= P <= CA3D_CANON_MAX_PERIOD, and S_0 its current state.
 *   S_(t+1) = step(S_t) by the ensemble's own step: u's rule and the ensemble's current boundary mode (reference, torus or closed),
 *   exactly as ca3d_ensemble_step does.
 *   The counts of a cell of S_t are the counts that step forms (host.ensemble_step): every axis applies its boundary to what the axis
 *   before it produced. von Neumann: F, the six face neighbours, 0 .. 6, in the main class. Moore: the 26-neighbour count, 0 .. 26, in
 *   the main class. Clustered: the main table is indexed by T = F + E + C (0 .. 26), the edges table by E (0 .. 12), the corners table
 *   by C (0 .. 8), and a cell adds one to each of the three histograms every step.
 *   A class's bins start at CA3D_USAGE_MAIN, _EDGES, _CORNERS. dead[base + c] (alive[base + c]) is the number of pairs (t, cell) with
 *   t < P, the cell dead (alive) in S_t and that class's count equal to c: at most 2^18 * 2^12 = 2^30. Bins of a class the kind does
 *   not look up, and main bins 7 .. 26 of a von Neumann ensemble, are zero.
 *   used_born[i] has bit c set exactly when dead[base_i + c] != 0 — born_c was read — and used_survive[i] the same for alive[]
 *   (i = 0 main, 1 edges, 2 corners). Flipping a table bit that is NOT set there leaves S_1 .. S_P as they are.
 *   steps echoes P; flags and reserved are zero.
 *   Per class that the kind looks up, sum(dead) + sum(alive) = 262 144 * P, and the sum of the class's alive[] is the population summed
 *   over S_0 .. S_(P-1), ca3d_envelope.population_sum.
 *
 * Ordering. As ca3d_ensemble_envelope without images: the launch runs behind what is queued on the ensemble's stream, and the ensemble
 * is only read: states, records, step counters, anchors, steps_done and stats are byte for byte as they were. It needs a state and a
 * rule on every universe of the range. The call waits for its own result. gpu_ms (nullable) receives the hipEvent time around the
 * launch. Records and steps are staged in a device array of the call's own.
 *
 * Errors: NULL `e`, steps or out — CA3D_ERR_INVALID_ARGUMENT without touching a device; `e` not configured —
 * CA3D_ERR_NOT_CONFIGURED; count == 0, first + count > n, a step count of 0 or above CA3D_CANON_MAX_PERIOD —
 * CA3D_ERR_INVALID_ARGUMENT; a universe without a state or without a rule — CA3D_ERR_NOT_CONFIGURED. Each message names its argument
 * and the first offending universe. A refused call touches none of the caller's arrays and nothing on the device.
 */
#define CA3D_USAGE_MAIN 0u      /* bins 0..26 (von Neumann: 0..6, the rest zero) */
#define CA3D_USAGE_EDGES 27u    /* bins 27..39, clustered only */
#define CA3D_USAGE_CORNERS 40u  /* bins 40..48, clustered only */
#define CA3D_USAGE_BINS 49u
typedef struct ca3d_usage
{
	uint32_t steps;            /* echoed P */
	uint32_t flags;            /* zero for now */
	uint32_t used_born[3];     /* main, edges, corners: bit c set iff dead[class base + c] != 0 */
	uint32_t used_survive[3];  /* the same for alive[] */
	uint32_t dead[49];         /* cells DEAD in S_t with count c, summed over t = 0..P-1 */
	uint32_t alive[49];
	uint32_t reserved[2];      /* zero */
} ca3d_usage;                  /* 432 bytes, a multiple of 16 */
int ca3d_ensemble_usage(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *steps /* [count] */,
                        ca3d_usage *out /* [count] */, float *gpu_ms /* may be NULL */);
int ca3d_ensemble_synchronize(ca3d_ensemble_t *e);
int ca3d_ensemble_get_stats(ca3d_ensemble_t *e, struct ca3d_stats *out);

/*
 * Seed states on the device (no reference counterpart: its start-up blob is drawn from Math.random on the host): the counter-based
 * fill every test, bench.py, tools/ and js/ca3d.js already share (host.random_fill / randomFill), produced where the state lives —
 * nothing state-sized crosses the bus, one kernel (csrc/ca_seed.hip) writes BOTH ping-pong buffers in one pass.
 *
 * The definition (host.seeded_state / seededState in executable form). With mix32(seed, i, r):
 *   x = (uint32_t)i * 0x9E3779B9 + seed + r * 0x85EBCA6B   (all modulo 2^32: i enters the hash modulo 2^32)
 *   x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
 * fill(i) = AND over r = 0 .. and_rounds of mix32(seed, i, r): every bit is set with probability 2^-(1 + and_rounds).
 * PACKED32: with cols = G / 32, the word at i = (x >> 5) + y * cols + z * cols * G — its index in the FULL grid, the index the digest
 * uses, so slabs compose — is fill(i) ANDed with the mask of its bits whose x lies in [box_min.x, box_max.x], and 0 when y or z is
 * outside the box. With the whole-grid box the state equals host.random_fill(state_words, seed, and_rounds) exactly.
 * UNPACKED: cell (x, y, z) is 1 exactly when it is inside the box and bit x & 31 of fill((x >> 5) + y * ceil(G / 32) + z * ceil(G / 32) * G)
 * is set, else 0 — the same universe in both layouts when G is a multiple of 32, defined for every legal unpacked G.
 * Slab engines fill their owned planes from the global indices and zero their ghosts. Ensembles index words inside the universe's own
 * 8192-word array, as their digest does.
 *
 * A seed REPLACES the state exactly as ca3d_upload_state does (one function decides it for both): the same words in both ping-pong
 * buffers, step counter 0, has_previous 0, queued steps dropped, pending resident launches forgotten, a pending edge phase abandoned,
 * what the renderer derived from the state stale, frames in flight joined. Unlike an upload, ca3d_seed_state and ca3d_group_seed_state
 * only ENQUEUE and return (the one exception: behind a resident multi-step launch whose completion has not been looked at yet the call
 * waits for the stream first, as that launch's verdict must not arrive after the state it belonged to has gone). Rules need not be set.
 *   ca3d_group_seed_state     one ca3d_seed_state per rank on that rank's device, nothing staged on the host; leaves the group as
 *                             ca3d_group_upload_state does (ghosts not valid: refreshed by the next ca3d_group_step)
 *   ca3d_ensemble_seed_state  universes [first, first + count): n_specs == 1 — every one of them gets specs[0] — or n_specs == count;
 *                             followed by the zero-step record launch of ca3d_ensemble_upload_state (records at step 0, has_previous
 *                             0); `specs` is consumed when the call returns, the fill may still be running. Universes outside the
 *                             range keep state, step counter and record.
 *   ca3d_ensemble_set_rule_tables  the tables of universes [first, first + count) as plain masks, in one copy: bit c of
 *                             born_masks[k] / survive_masks[k] = born / survive at count c (born "2,4", survive "1,3,5": 0x14, 0x2A);
 *                             c is 0..6 in a von Neumann ensemble and 0..26 in a Moore one (27-bit masks: born "5-7", survive
 *                             "4-6": 0xE0, 0x70). n_masks == 1 (every universe of the range gets the pair) or == count. What is
 *                             stored is what ca3d_ensemble_set_rules derives for the same rule. A bit at position 7 (27 in a Moore
 *                             ensemble) or above: CA3D_ERR_INVALID_ARGUMENT naming the universe. Unlike the seed calls this one WAITS for the stream
 *                             (as ca3d_ensemble_set_rules does): the masks are consumed and the copy is done on return.
 * NULL handle / spec: CA3D_ERR_INVALID_ARGUMENT ("NULL"), without touching a device. box_min > box_max on an axis, box_max >= G,
 * and_rounds > 31, n_specs / n_masks neither 1 nor count: CA3D_ERR_INVALID_ARGUMENT. Not configured: CA3D_ERR_NOT_CONFIGURED.
 */
typedef struct ca3d_seed
{
	uint32_t seed;        /* host.random_fill's seed */
	uint32_t and_rounds;  /* 0..31: density 2^-(1+and_rounds); > 31: CA3D_ERR_INVALID_ARGUMENT */
	uint32_t box_min[3];  /* x, y, z inclusive, GLOBAL cell coordinates (as ca3d_summary's box) */
	uint32_t box_max[3];  /* cells outside the box are dead; the whole grid is {0,0,0}..{G-1,G-1,G-1} */
} ca3d_seed;
int ca3d_seed_state(ca3d_t *h, const ca3d_seed *spec);
int ca3d_group_seed_state(ca3d_group_t *g, const ca3d_seed *spec);
int ca3d_ensemble_seed_state(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const ca3d_seed *specs, uint32_t n_specs);
int ca3d_ensemble_set_rule_tables(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *born_masks, const uint32_t *survive_masks,
                                  uint32_t n_masks);

/* Resident launches that gave up (a wait for neighbour tile faces timed out: not all workgroups were on the chip) and
 * whose steps the engine re-ran through the per-step kernels, since ca3d_create. The calls that noticed returned CA3D_OK
 * with the final state intact; ca3d_last_error() carried a note and the resident path stays off until
 * ca3d_set_option("resident", 1). Slab engines do not recover (the neighbours' ghosts came from the failed launch):
 * they return CA3D_ERR_DEVICE and want a new upload. */
int ca3d_recovered_launches(ca3d_t *h, uint32_t *out_count);

/* Interop: run on a caller-owned hipStream_t (e.g. torch's current stream). NULL is HIP's legacy default stream
 * (what torch uses unless told otherwise), not "none". ca3d_use_own_stream goes back to the engine's stream. */
int ca3d_set_stream(ca3d_t *h, void *hip_stream);
int ca3d_use_own_stream(ca3d_t *h);
/* Device pointer of ping-pong buffer `which` (0/1) — whole allocation including ghosts. Valid until the next ca3d_step /
 * ca3d_upload_state / ca3d_configure on the engine: a resident multi-step launch writes its result to a third buffer and
 * rotates the three (buffer [step % 2] is always the current state, the other one the state one step earlier).
 * The caller may WRITE the state through the pointer (on the engine's stream, or ordered against it) without telling the
 * engine: while the pointer is valid every ca3d_render rebuilds what it derives from the state (occupancy bits, the bricked
 * copy) instead of reusing an earlier frame's — one extra pass over the state per frame, the price of not having to
 * announce writes. */
int ca3d_device_buffer(ca3d_t *h, int which, void **device_ptr, size_t *n_bytes);

typedef struct ca3d_info
{
	uint32_t grid_size;
	int32_t layout;
	uint32_t z0, nz, ghost; /* slab (full grid: 0, G, 0) */
	uint64_t step;          /* steps since the last upload */
	uint64_t state_words;   /* words ca3d_upload_state / ca3d_read_state expect */
	int32_t current_buffer; /* step % 2 */
	int32_t device;
	char kernel_name[64]; /* kernel variant the current rules select */
	uint64_t launches_total; /* kernel launches issued by the step calls since ca3d_create */
} ca3d_info;
int ca3d_get_info(ca3d_t *h, ca3d_info *out);

/*
 * createShaderModule / createComputePipeline (main_pathtraced.js:1421-1433) report compile problems through the
 * browser console; here the step kernel is specialised for the rule at run time inside ca3d_set_rules /
 * ca3d_configure (option "jit"), and a failed compile does NOT fail those calls — the pre-built kernels take over,
 * ca3d_get_info().kernel_name lacks its "(jit)" suffix, ca3d_last_error() holds the message right after the call and
 * this getter returns the compiler log of the most recent attempt (empty string: no failure). `needed` (nullable)
 * receives the size including the terminator; the text is truncated to n_bytes.
 */
int ca3d_get_jit_log(ca3d_t *h, char *buf, size_t n_bytes, size_t *needed);

/*
 * The run-time compiler's bookkeeping for THIS PROCESS (all engines): how many programs were compiled, how many came
 * from the on-disk cache of code objects ($CA3D_CACHE_DIR, else $XDG_CACHE_HOME/ca3d, else $HOME/.cache/ca3d;
 * CA3D_JIT_CACHE=0 turns it off; files are keyed on architecture, compiler version, options and the full program
 * text, so they never go stale) and how many were already loaded, with the milliseconds each kind cost. A process
 * that finds its rules in the cache compiles nothing: programs_compiled == 0 — `_restartSim` (main_pathtraced.js:
 * 624-637) stays cheap from the second start on. Needs no engine.
 */
typedef struct ca3d_jit_stats
{
	uint64_t programs_compiled;    /* hiprtc compiles */
	uint64_t programs_from_disk;   /* code objects read from the cache directory */
	uint64_t programs_from_memory; /* requests answered by a module this process had loaded already */
	double compile_ms;             /* inside hiprtc */
	double disk_read_ms;           /* reading + verifying cached objects */
	double load_ms;                /* hipModuleLoadData (+ writing new objects to the cache) */
	char cache_dir[256];           /* "" when the disk cache is off or its directory cannot be created */
} ca3d_jit_stats;
int ca3d_get_jit_stats(ca3d_jit_stats *out);

/*
 * Diagnostics (no reference counterpart): everything that decides WHICH instruction stream the next step batch runs, as one
 * string — kernel name, grid, a hash of the rule payload, the resident-kernel form options, a hash of the device sources the
 * run-time compiler is given. A profile (instruction counts per step, tools/pmc_sq_reduce.py) is only comparable with a run
 * whose string is the same: bench.py / js/bench.js price a resident kernel's time against a committed profile only then.
 * `needed` (nullable) receives the size including the terminator; the text is truncated to n_bytes.
 */
int ca3d_get_kernel_variant(ca3d_t *h, char *buf, size_t n_bytes, size_t *needed);

typedef struct ca3d_stats
{
	uint64_t steps;          /* steps in the last ca3d_step / ca3d_slab_step batch */
	uint64_t kernel_launches; /* kernel launches that batch issued */
	double gpu_ms;           /* hipEvent time around the batch on the engine's stream (waits for it) */
	double cell_steps;       /* cells updated x steps */
	double algorithmic_bytes; /* 0.25 B (PACKED32) or 8 B (UNPACKED) per cell-step: SURVEY 8(d) */
} ca3d_stats;
int ca3d_get_stats(ca3d_t *h, ca3d_stats *out);

/*
 * _updateUniforms + _renderPass (main_pathtraced.js:1747-1750, 1775-1794) and the history textures (729-779):
 * renders the CURRENT state (buffer step % 2, as bind group 2 of the render pass, 1788) through the volume
 * renderer. `uniforms` is the reference's 128-float common block verbatim (MemoryManager.bufferf32; layout
 * pathtraced_fragment_clustered.wgsl:17-34); width/height give the pixel grid (the shader's windowSize
 * uniform supplies the aspect ratio, as in the reference). spp is 1 (pixel centre) or 4 (2x2 stratified
 * sub-samples averaged in linear light before gamma). Outputs, each nullable, row-major, top row first:
 *   presentation_rgba8  width*height*4 bytes   pow(rgb, 1/gamma), alpha  -> the canvas attachment
 *   light_rgba16f       width*height*4 halfs   linear rgb, 1              -> light history attachment
 *   depth_rg16f         width*height*2 halfs   distance from camera, 1    -> depth history attachment
 * The engine keeps the device-side targets and swaps its two history surfaces per call (1793). Full grid only.
 * Synchronous only when an output pointer is given.
 *
 * What a frame is: by default the frame the reference's jittered, temporally accumulated process converges to
 * under a static camera (exact cell walk). ca3d_set_option("render_mode", 1) switches to ONE literal
 * reference frame per call (jittered marches + history look-ups + temporal blend; spp must be 1; packed layout);
 * "render_reset_history" clears the history surfaces. An engine configured with CA3D_LAYOUT_UNPACKED renders
 * through the legacy shader model (shaders/pathtraced_fragment.wgsl).
 *
 * A call without output pointers only enqueues and does NOT wait for a pending resident multi-step launch to be
 * verified (ca3d_recovered_launches): should that launch later turn out to have timed out, the frame was drawn from
 * its unwritten output — wrong once; the engine then re-runs the steps and clears the history surfaces, so the
 * literal mode does not keep blending that frame in. A call WITH an output pointer settles the launch first.
 */
int ca3d_render(ca3d_t *h, const float uniforms[128], uint32_t width, uint32_t height, uint32_t spp,
                uint8_t *presentation_rgba8, uint16_t *light_rgba16f, uint16_t *depth_rg16f);

/* Measurement helper (no reference counterpart; SURVEY 8(d) "also report against a measured device-to-device copy
 * ceiling"): `reps` float4-per-lane copies of n_bytes between two scratch buffers on the engine's stream, HIP events
 * around them; *gb_per_s = bytes read + bytes written per second / 1e9. Waits for the GPU. */
int ca3d_measure_copy(ca3d_t *h, size_t n_bytes, uint32_t reps, double *gb_per_s);

typedef struct ca3d_render_stats
{
	double gpu_ms;          /* hipEvent time of the last ca3d_render kernel */
	uint64_t primary_rays;  /* width * height * spp */
	uint64_t shadow_rays;   /* samples that reached the shading gate and traced a shadow ray */
	uint64_t primary_cell_visits, shadow_cell_visits; /* cells the two walks stepped through */
} ca3d_render_stats;
int ca3d_get_render_stats(ca3d_t *h, ca3d_render_stats *out);

/*
 * The ensemble's contact sheet (no reference counterpart: its UI shows one grid): universes first .. first + count - 1 of a
 * configured ensemble, each rendered as one tile of a sheet, in ONE launch (kernel ca_render_sheet64, csrc/render_sheet.hip: a
 * workgroup copies its universe's 32 KiB into LDS and walks every view and shadow ray of its pixels there).
 *
 * The definition has no arithmetic of its own. Tile k is, bit for bit and in all three targets, the converged frame that
 *   ca3d_render(uniforms, tile_w, tile_h, spp)
 * draws on an engine configured at 64^3, CA3D_LAYOUT_PACKED32, holding universe first + k's current state, with "render_skip" 0 (the
 * cell-by-cell walk; the skipping walk is only within tolerance of it) and "render_indirect" 0. ONE uniform block serves every tile;
 * its windowSize is taken as given, exactly as ca3d_render takes it. Light gizmo, depth overlay, gamma and material colour are part of
 * the frame and therefore of every tile. spp is 1 or 4 as in ca3d_render.
 *
 * Layout: the sheet is W = columns * tile_w pixels wide and H = ceil(count / columns) * tile_h high, row-major, top row first; tile k
 * sits at column k % columns, row k / columns. Tile slots past `count` in the last row are zero in every byte of every target.
 * Outputs, each nullable, sized as ca3d_render's for a W x H target:
 *   presentation_rgba8  W*H*4 bytes    light_rgba16f  W*H*4 halfs    depth_rg16f  W*H*2 halfs
 * The call runs on the ensemble's stream, behind whatever steps are queued, and draws the states those steps leave. With a pointer
 * given it returns when that sheet is on the host; with all three NULL it draws into device targets the ensemble owns (grown on
 * demand, freed by a configure and by destroy) and does not wait. Rules are not needed: a configured ensemble with a state in every
 * universe of the range is enough.
 *
 * Errors: NULL handle or NULL uniforms — CA3D_ERR_INVALID_ARGUMENT without touching a device; not configured —
 * CA3D_ERR_NOT_CONFIGURED; count == 0 or first + count > n, columns == 0, tile_w or tile_h not a multiple of 16 in [16, 1024], spp
 * not 1 or 4, W * H > 2^26 pixels — CA3D_ERR_INVALID_ARGUMENT; a universe of the range without a state — CA3D_ERR_NOT_CONFIGURED,
 * the message names the first such universe.
 *
 * ca3d_ensemble_get_sheet_stats describes the last sheet and waits for it: gpu_ms the hipEvent time around its launch, primary_rays =
 * count * tile_w * tile_h * spp, shadow rays and both visit counts summed over the tiles — the sums of ca3d_get_render_stats over the
 * frames that define the tiles. Before any sheet (or after a configure): CA3D_ERR_NOT_CONFIGURED.
 */
int ca3d_ensemble_render_sheet(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const float uniforms[128], uint32_t tile_w, uint32_t tile_h,
                               uint32_t columns, uint32_t spp, uint8_t *presentation_rgba8, uint16_t *light_rgba16f, uint16_t *depth_rg16f);
int ca3d_ensemble_get_sheet_stats(ca3d_ensemble_t *e, ca3d_render_stats *out);

/*
 * Windows (no reference counterpart): 64^3 regions of an engine's grid cut into universes of an ensemble, and universes stamped back
 * into the grid, without a state leaving the device — what the ensemble's census, isolate, compose and canon found can be put into a
 * big world and rendered, the objects of a region of a running world can be counted, and a pattern can be pasted. Both calls work
 * between a PACKED, FULL-GRID engine and an ensemble on the same device, one launch per phase (csrc/ca_window.hip), behind what is
 * queued. host.cut_window and host.stamp_windows restate them.
 *
 * The window map. A window at origin (ox, oy, oz), each below G, maps window cell (i, j, k), each 0 .. 63, to grid cell
 *   ((ox + i) mod G, (oy + j) mod G, (oz + k) mod G): the grid is addressed as a torus whatever the step's boundary is, and G >= 64
 *   makes the map injective. G is any grid the engine accepts from 64 up, the multiples of 32 that are no power of two included.
 * Cut. Universe w[k].universe of `dst` becomes window k of the engine's current state — after every step requested so far: queued steps
 *   are submitted and a resident launch is settled first, as ca3d_read_state does. Both ping-pong buffers of the universe get the
 *   words, its record is rebuilt at step 0 with no previous state (the launch ca3d_ensemble_upload_state ends in) and it counts as
 *   having a state; rules are untouched. The universes of one call must be distinct. The engine is only read.
 * Stamp. The three modes commute: a call's result does not depend on the order of its windows, and windows may overlap freely.
 *     CA3D_STAMP_OR       every live cell of universe w[k].universe of `src`, mapped through window k, is set in the grid;
 *     CA3D_STAMP_ERASE    those cells are cleared;
 *     CA3D_STAMP_REPLACE  first every cell of every window's box is cleared, then every universe is ORed in (two launches).
 *   The engine afterwards: the step counter is unchanged; there is no previous state (has_previous is 0, births and deaths are 0 in
 *   the next summary, until the next step); what the renderer derived from the state is rebuilt by the next frame, and frames in
 *   flight are joined before the stamp; queued steps are submitted and a resident launch is settled before the stamp. A configured
 *   engine that has no state yet is taken as all dead, at step 0: a world can be built from objects alone. The ensemble is only read.
 * Ordering is ca3d_ensemble_isolate's: the launches run on the destination's stream (a cut: the ensemble's, a stamp: the engine's)
 *   behind what is queued there and behind an event recorded on the source's stream at the call, and the call waits for its own
 *   result. gpu_ms (nullable) receives the hipEvent time around the launches. The windows are staged in a device array on the
 *   ensemble's handle (16 bytes a window, grown when a call needs more, freed by a configure and by destroy).
 *
 * Errors — a refused call touches neither handle, and names the window where there is one: a NULL handle or array, n == 0 or above
 * 1 << 20, a universe out of range, an origin >= G, the same destination universe twice in a cut, an unknown mode, handles on
 * different devices — CA3D_ERR_INVALID_ARGUMENT; either handle not configured, a cut from an engine without a state, a stamp from a
 * universe without a state — CA3D_ERR_NOT_CONFIGURED; the unpacked layout, a slab engine (ca3d_configure_slab, and so every rank of
 * a group), G < 64 — CA3D_ERR_UNSUPPORTED.
 */
typedef struct ca3d_window
{
	uint32_t universe;  /* of the ensemble */
	uint32_t origin[3]; /* x, y, z of window cell (0, 0, 0) in the grid, each < G */
} ca3d_window;          /* 16 bytes */
enum
{
	CA3D_STAMP_OR = 0,
	CA3D_STAMP_REPLACE = 1,
	CA3D_STAMP_ERASE = 2
};
int ca3d_cut_windows(ca3d_t *src, ca3d_ensemble_t *dst, uint32_t n, const ca3d_window *w, float *gpu_ms /* may be NULL */);
int ca3d_stamp_windows(ca3d_t *dst, ca3d_ensemble_t *src, uint32_t n, const ca3d_window *w, uint32_t mode, float *gpu_ms /* may be NULL */);

/* How many converged frames the engine keeps in flight (option "render_pipeline" below): the number of internal streams — on pairwise
 * different hardware queues, probed when the first pipelined frame is drawn — that such frames alternate between; 0 before that frame,
 * with the option off, or when the runtime gave the engine no two streams that run side by side. Does not wait for the GPU. */
int ca3d_get_render_pipeline(ca3d_t *h, int32_t *frames_in_flight);

/* Options (not part of the reference surface): "queue" n: queued submission (see ca3d_step; 0 = off); "graph" 0/1 hipGraph batching; "stats" 0/1: record the event pair
 * ca3d_get_stats reads around every ca3d_step batch (on by default; a host that steps in small batches and never asks
 * for stats saves two marker packets per call); "graph_prepare" n builds now the
 * graphs a later ca3d_step(n) replays — a batch of any length up to 1024 steps is one graph of exactly that many
 * steps (otherwise built on first use); "fused" 0/1 two-step fused kernel
 * (bit-exact, off by default); "variant" 1 forces the generic / literal kernels; "jit" 0/1 run-time (hiprtc) specialisation of the step
 * kernel for the current rule, compiled inside ca3d_set_rules / ca3d_configure (on by default; a failed compile
 * keeps the pre-built kernels and is reported through ca3d_get_jit_log); "resident" 0/1: batches of "resident_min" (default 8) steps and more run as ONE launch of
 * the resident multi-step kernel where one exists (512^3 and 256^3 — von Neumann rule tables, and rule-sets with diagonal classes
 * compiled at run time: the state stays in registers and only tile faces cross the chip; 64^3, von Neumann rule tables: the
 * whole grid in one workgroup; a resident kernel is only selected when the runtime says all its workgroups fit on the CUs the
 * engine's stream may use; every in-kernel wait is bounded by "resident_timeout_us", default 200 000 — after a timeout the
 * engine re-runs the affected steps through the per-step kernels at the next call that looks at the state and turns the
 * path off: ca3d_recovered_launches; "resident_fault_tile" t: diagnostics, tile t - 1 of the next resident launch leaves at
 * once, which makes that launch time out);
 * "roll" 0/1 the rolling-window form of the run-time compiled class kernels (on by
 * default where it applies), "roll_tile" 0-3 which of its forms (0 every thread shifts its three rows, 1 workgroup tiles sharing the
 * shifted rows through LDS, 2 wave tiles, 3 two words per thread), "roll_z" 0/2/4/8/16/15/30 its planes per thread
 * (0: chosen per launch); "resident_zsplit" 1/2, "resident_rows" 32/16: tiling of the resident von Neumann kernels, "resident_pair" 1/0: at 512^3 with the
 * default tiling a thread owns two adjacent rows x 16 planes instead of one row x 32 (less LDS traffic; default 1); "graph_min" n: batches shorter than n
 * steps are launched kernel by kernel instead of as a captured graph; "render_mode" 0/1; "render_row_begin" / "render_row_end":
 * ca3d_render then fills image rows [begin, end) only (begin a multiple of 16; 0 / 0 = the whole frame) — a rank's
 * band when the GPUs of a node share one frame; "render_skip" 0/1 empty-space skipping by
 * 32x8x8-cell occupancy blocks, active on sparse volumes only (on by default; within the renderer's tolerance of
 * the cell-by-cell walk, not bit-identical to it); "render_sched" 0/1 dynamic ray
 * scheduling inside each wave of the renderer (on by default; the frame is the same bit for bit);
 * "render_reset_history"; "render_indirect" 0/1 adds the one-bounce neighbour lighting of calculateIndirectLighting
 * (pathtraced_fragment_clustered.wgsl:307-377 — present in the reference, its call commented out at :424; off by
 * default like there; converged-frame mode, packed layout); "render_stream" 0/1 the converged frame of a dense packed volume as
 * ray-stream passes (render_stream.hip; on by default; 0: the in-wave scheduled kernel; the same frame bit for bit);
 * "render_stream_check" 0/1 diagnostics: the stream passes count where their interval filter and the slab test disagree and which
 * answers were looked up unset — ca3d_render fails with CA3D_ERR_DEVICE if any (off by default; takes the frame off the pipeline);
 * "render_pipeline" 0 / 1 / 2-4 converged frames in flight (1, the default: four up to 24 M samples a frame, three above; 0: none;
 * 2-4: that many): frames that stay on the device (no host pointers), are drawn by the stream passes and go down the engine's OWN
 * stream alternate between that many internal streams; a frame that finds another one still in flight sizes its persistent walk
 * launches for its share of the chip, so that the frames' walks run side by side (a frame that finds the engine idle takes the whole
 * chip: a host that draws one frame per display refresh loses nothing; the first frame after a step, an upload or any other call
 * on the engine's stream is drawn on that stream); the engine's stream waits for them at the next call that
 * touches the state, a render target (ca3d_render_target, ca3d_get_render_stats) or the stream. Each frame is the frame of
 * one-at-a-time rendering, bit for bit; a caller on a stream of its own (ca3d_set_stream), a frame with host pointers, a band or a
 * literal frame is never pipelined; ca3d_get_render_pipeline reports the depth in use; the first pipelined frame of an engine probes
 * the runtime's streams for separate hardware queues (a few milliseconds per pair, once);
 * "render_frame_bricks" 0/1 the literal frame as a batched march over the bricked volume (on by default; 0: the statement-by-
 * statement form, the same frame bit for bit); it also decides whether the converged frame's ray-stream walks read the bricked
 * copy or the row-major state (grids up to 2048; above, always the state) — the same pixels either way; "rows" 0/1 the run-time compiled rows kernel on grids that are not a power of two (on by
 * default; 0: the kernels that served them before — tests, tuning). */
int ca3d_set_option(ca3d_t *h, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* CA3D_H */
