// ca3d_ensemble_*: many independent 64^3 universes side by side on one device (include/ca3d.h). One workgroup of ca_ensemble_vn64,
// ca_ensemble_moore64 or ca_ensemble_clustered64 (ca_ensemble.hip; the ensemble's neighbourhood and `clustered` decide) steps one
// universe with its state in registers; a launch
// over B workgroups is B universes, each with its own rule table pair, its own step counter, its own summary record and — in
// ca3d_ensemble_step_until / ca3d_ensemble_step_until_cycle / ca3d_ensemble_step_until_moving / ca3d_ensemble_step_until_trace — its own moment to stop. The host side is bookkeeping: the per-universe arrays, the rule canonicalisation
// (the engine's own, rules.cpp), and cutting long calls into launches of at most kEnsembleMaxSteps steps.
// ca3d_ensemble_set_boundary chooses what the steps queued from then on see behind a universe's faces (ca_ensemble_boundary.hip holds the
// torus and closed-cube forms of the kernels); it is a field of the handle that launch_of copies into every launch.
// ca3d_ensemble_render_sheet draws a range of universes as the tiles of one contact sheet (render_sheet.hip).
// ca3d_ensemble_census lists the connected objects of a range of universes (ca_census.hip).
// ca3d_ensemble_isolate makes objects a census named the only thing in universes of their own (ca_isolate.hip).
// ca3d_ensemble_compose stages whole universes, turned and shifted, into universes of their union (ca_compose.hip).
// ca3d_ensemble_canon names universes up to the 48 symmetries of the cube and translation (ca_canon.hip).
// ca3d_ensemble_canon_period does so over a period of each universe's own steps, inside the kernel (ca_canon_period.hip).
// ca3d_ensemble_envelope takes envelope, stator, rotor and heat over such a period, and may write them as universes (ca_envelope.hip).
// ca3d_ensemble_damage follows a universe and a perturbed twin and takes their Hamming distance at every step (ca_damage.hip).
// ca3d_cut_windows / ca3d_stamp_windows move 64^3 regions between an engine's grid and universes (ca_window.hip); they live here because
// the ensemble record is private to this file, and reach the engine through ca3d_engine.h.
// What these calls share is written once, in the unnamed namespace: a staging array on the handle (Scratch) and the event pair around a
// launch (Timer), both had from `reserve`; reset_records and mark_state / mark_rules for universes that were just written; and, for
// isolate, compose, envelope and damage, the checks on two handles, the wait on the source's stream and the end of the call (finish_destinations).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ca3d_engine.h"

using namespace ca3d;

struct ca3d_ensemble
{
	// a device staging array of the handle and its size: a call that needs more grows it (`reserve`), a smaller one reuses it, and it goes
	// with the other arrays at a configure
	struct Scratch
	{
		uint8_t *array = nullptr;
		size_t bytes = 0;
		template <class T> T *at(size_t offset = 0) const { return reinterpret_cast<T *>(array + offset); }
	};
	// the event pair around the launch of one kind of call, created at the first such call and kept until the handle goes
	struct Timer
	{
		hipEvent_t start = nullptr, stop = nullptr;
	};
	int device = 0;
	hipStream_t stream = nullptr;
	Timer run_time; // around the launches of the last step call; created with the handle
	uint32_t n = 0; // universes; 0: not configured
	int neighbourhood = CA3D_ENSEMBLE_VON_NEUMANN; // of every universe: the kernel, and ensemble_rule_words() words of `rules` each
	bool clustered = false;                        // Moore with edges and corners table pairs of their own (ca3d_ensemble_configure_clustered)
	int boundary = CA3D_ENSEMBLE_BOUNDARY_REFERENCE; // of the launches queued from now on (ca3d_ensemble_set_boundary); a configure resets it
	uint32_t *state = nullptr, *prev = nullptr, *rules = nullptr, *steps_done = nullptr, *reason = nullptr;
	ca3d_summary *records = nullptr;
	// ca3d_ensemble_step_until_cycle: every universe's anchor state (n x 32 KiB) and its anchor step / anchor hash / period / unused
	// (n x 4 words), allocated at the first call that watches CA3D_STOP_PERIODIC, gone with the other arrays at a configure
	uint32_t *anchor = nullptr, *cycle = nullptr;
	// ca3d_ensemble_step_until_moving: the same record with the found shift and the anchor's population and box behind it (n x 8 words:
	// what the *_moving kernels take for `cycle`), allocated at the first call that watches CA3D_STOP_MOVING; the anchors are shared
	uint32_t *moving = nullptr;
	// ca3d_ensemble_step_until_trace: the samples of the call under way, [n][K][3] words
	Scratch trace;
	// ca3d_ensemble_seed_state with one spec per universe: the specs on the device, their pinned staging copy (n entries each, allocated
	// at the first such call) and the event behind the copy out of it
	ca3d_seed *seed_dev = nullptr, *seed_host = nullptr;
	hipEvent_t ev_seed = nullptr;
	std::vector<uint8_t> has_rules, has_state;
	uint32_t missing_rules = 0, missing_state = 0; // universes without either
	// the last step call, for ca3d_ensemble_get_stats
	bool timed = false;
	uint64_t last_steps = 0, last_launches = 0;
	double last_cell_steps = 0;
	// ca3d_ensemble_render_sheet: the sheet's three device targets (presentation RGBA8, light RGBA16F, depth RG16F), grown when a sheet
	// has more than sheet_px pixels, gone with the other arrays at a configure; its three counters, its event pair and what
	// ca3d_ensemble_get_sheet_stats says of the last one
	uint32_t *sheet_present = nullptr, *sheet_depth = nullptr;
	uint2 *sheet_light = nullptr;
	size_t sheet_px = 0;
	unsigned long long *sheet_counters = nullptr;
	Timer sheet_time;
	bool sheet_drawn = false;
	uint64_t sheet_primary_rays = 0;
	// ca3d_ensemble_census: the result of the call under way — [count][max_components] records, then n_components[count], then
	// remaining[count]
	Scratch census;
	Timer census_time;
	// ca3d_ensemble_isolate, on the DESTINATION handle: the results of the call under way, [n_jobs] of 16 bytes, then its jobs, [n_jobs]
	// of 8 bytes; the event that orders the launch behind the source's stream (created with the pair, without timing)
	Scratch isolate;
	Timer isolate_time;
	hipEvent_t isolate_src = nullptr;
	// ca3d_ensemble_compose, on the DESTINATION handle: the records of the call under way, [n_dst] of 16 bytes, then its parts, [n_parts]
	// of 24 bytes, then part_begin, [n_dst + 1] words; the event that orders the launch behind the source's stream
	Scratch compose;
	Timer compose_time;
	hipEvent_t compose_src = nullptr;
	// ca3d_ensemble_canon: the result of the call under way — [count] records of 32 bytes, then [count][48] digests.
	// ca3d_ensemble_canon_period stages in the same array — [count] records of 32 bytes, then [count][keys_stride] keys, then the
	// uploaded periods, [count] words — and has an event pair of its own
	Scratch canon;
	Timer canon_time, canon_period_time;
	// ca3d_ensemble_envelope, on the handle the launch runs on (the destination, or the source when there is none): the records of the
	// call under way, [count] of 48 bytes, then the uploaded periods, [count] words; the event that orders the launch behind the
	// source's stream
	Scratch envelope;
	Timer envelope_time;
	hipEvent_t envelope_src = nullptr;
	// ca3d_ensemble_damage, on the handle the launch runs on, as the envelope's: the records of the call under way, [count] of 48 bytes,
	// then the uploaded steps, twins and flips, [count] x 6 words, then the curve, [count][curve_stride] words, when one is asked for
	Scratch damage;
	Timer damage_time;
	hipEvent_t damage_src = nullptr;
	// ca3d_ensemble_usage: the records of the call under way, [count] of 432 bytes, then the uploaded step counts, [count] words
	Scratch usage;
	Timer usage_time;
	// ca3d_cut_windows / ca3d_stamp_windows, whichever way the words go: the windows of the call under way, [n] of 16 bytes; the event
	// that orders the launches behind the source's stream
	Scratch windows;
	Timer windows_time;
	hipEvent_t windows_src = nullptr;
};

namespace
{

using Scratch = ca3d_ensemble::Scratch;
using Timer = ca3d_ensemble::Timer;

void free_arrays(ca3d_ensemble *e)
{
	for (void *p : {(void *)e->state, (void *)e->prev, (void *)e->rules, (void *)e->steps_done, (void *)e->reason, (void *)e->records, (void *)e->anchor, (void *)e->cycle, (void *)e->moving})
		if (p) hipFree(p);
	e->state = e->prev = e->rules = e->steps_done = e->reason = e->anchor = e->cycle = e->moving = nullptr;
	e->records = nullptr;
	if (e->seed_dev) hipFree(e->seed_dev);
	if (e->seed_host) hipHostFree(e->seed_host);
	e->seed_dev = e->seed_host = nullptr;
	for (void *p : {(void *)e->sheet_present, (void *)e->sheet_light, (void *)e->sheet_depth, (void *)e->sheet_counters})
		if (p) hipFree(p);
	e->sheet_present = e->sheet_depth = nullptr;
	e->sheet_light = nullptr;
	e->sheet_counters = nullptr;
	e->sheet_px = 0;
	e->sheet_drawn = false;
	for (Scratch *s : {&e->trace, &e->census, &e->isolate, &e->compose, &e->canon, &e->envelope, &e->damage, &e->usage, &e->windows})
	{
		if (s->array) hipFree(s->array);
		*s = Scratch{};
	}
	e->n = 0;
	e->timed = false;
}

int check_range(const ca3d_ensemble *e, uint32_t first, uint32_t count)
{
	if (!e->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called");
	if (count == 0 || first >= e->n || count > e->n - first) return fail(CA3D_ERR_INVALID_ARGUMENT, "universes [%u, %u + %u) of %u", first, first, count, e->n);
	return CA3D_OK;
}

// every universe of a checked range holds a state
int require_state(const ca3d_ensemble *e, uint32_t first, uint32_t count)
{
	for (uint32_t u = first; u < first + count; u++)
		if (!e->has_state[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_upload_state has not been called for universe %u", u);
	return CA3D_OK;
}

// configure -> set_rules (every universe) -> upload (every universe) -> step
int ensemble_ready(const ca3d_ensemble *e)
{
	if (!e->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called");
	if (e->missing_rules) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_set_rules has not been called for %u of %u universes", e->missing_rules, e->n);
	if (e->missing_state) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_upload_state has not been called for %u of %u universes", e->missing_state, e->n);
	return CA3D_OK;
}

EnsembleLaunch launch_of(const ca3d_ensemble *e)
{
	EnsembleLaunch l{};
	l.state = e->state; l.prev = e->prev;
	l.rules = e->rules;
	l.neighbourhood = e->neighbourhood;
	l.clustered = e->clustered;
	l.boundary = e->boundary;
	l.records = e->records;
	l.steps_done = e->steps_done; l.reason = e->reason;
	l.anchor = e->anchor; l.cycle = e->cycle;
	l.first = 0; l.count = e->n;
	return l;
}

// the records of states just written into universes [first, first + count): step 0, no previous state. One launch that steps nothing,
// behind the writes on the handle's stream
int reset_records(ca3d_ensemble *e, uint32_t first, uint32_t count)
{
	EnsembleLaunch l = launch_of(e);
	l.first = first; l.count = count;
	l.reset = true;
	l.final = true;
	HIP_TRY(launch_ensemble(l, e->stream));
	return CA3D_OK;
}

// universes [first, first + count) now hold a state (mark_state) / rules (mark_rules): what ensemble_ready and require_state ask for
void mark(std::vector<uint8_t> &has, uint32_t &missing, uint32_t first, uint32_t count)
{
	for (uint32_t u = first; u < first + count; u++)
		if (!has[u]) { has[u] = 1; missing--; }
}
void mark_state(ca3d_ensemble *e, uint32_t first, uint32_t count) { mark(e->has_state, e->missing_state, first, count); }
void mark_rules(ca3d_ensemble *e, uint32_t first, uint32_t count) { mark(e->has_rules, e->missing_rules, first, count); }

bool moore(const ca3d_ensemble *e) { return e->neighbourhood == CA3D_ENSEMBLE_MOORE; }
uint32_t table_bits(const ca3d_ensemble *e) { return moore(e) ? 27u : 7u; } // counts 0 .. 26 / 0 .. 6

uint32_t rule_words(const ca3d_ensemble *e) { return ensemble_rule_words(e->neighbourhood, e->clustered); }
constexpr uint32_t kClusteredBits[3] = {27u, 13u, 9u}; // main 0 .. 26, edges 0 .. 12, corners 0 .. 8

// what a universe's born / survive masks are stored as (ca_ensemble.hip reads it back: VnStep::load, MooreStep::load, ClusteredStep::load);
// in a clustered ensemble the main pair with both side pairs silent
void pack_rule(const ca3d_ensemble *e, uint32_t born, uint32_t survive, uint32_t *out)
{
	if (e->clustered) { out[0] = born; out[1] = survive; out[2] = out[3] = out[4] = out[5] = 0u; }
	else if (moore(e)) { out[0] = born; out[1] = survive; }
	else out[0] = survive | born << 8;
}
// a clustered universe's three pairs (main, edges, corners); bits no count can reach are dropped
void pack_clustered(const uint32_t born[3], const uint32_t survive[3], uint32_t *out)
{
	for (int s = 0; s < 3; s++)
	{
		const uint32_t mask = (1u << kClusteredBits[s]) - 1u;
		out[2 * s] = born[s] & mask;
		out[2 * s + 1] = survive[s] & mask;
	}
}

// `words`: ensemble_rule_words() words for each of universes [first, first + count)
int store_rules(ca3d_ensemble *e, uint32_t first, uint32_t count, const std::vector<uint32_t> &words)
{
	const uint32_t per = rule_words(e);
	HIP_TRY(hipSetDevice(e->device));
	// stream-ordered behind the steps already enqueued, which keep the rules they were enqueued under; the source is consumed on return
	HIP_TRY(hipMemcpyAsync(e->rules + (size_t)first * per, words.data(), (size_t)count * per * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	mark_rules(e, first, count);
	return CA3D_OK;
}

// `one`: one universe's packed rule, stored for each of universes [first, first + count)
int store_rule_repeated(ca3d_ensemble *e, uint32_t first, uint32_t count, const uint32_t *one)
{
	const uint32_t per = rule_words(e);
	std::vector<uint32_t> words((size_t)count * per);
	for (size_t k = 0; k < words.size(); k++) words[k] = one[k % per];
	return store_rules(e, first, count, words);
}

int configure_ensemble(ca3d_ensemble *e, uint32_t grid_size, uint32_t n_universes, int neighbourhood, bool clustered = false)
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (neighbourhood != CA3D_ENSEMBLE_VON_NEUMANN && neighbourhood != CA3D_ENSEMBLE_MOORE)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown ensemble neighbourhood %d (CA3D_ENSEMBLE_VON_NEUMANN = 0, CA3D_ENSEMBLE_MOORE = 1)", neighbourhood);
	if (grid_size != 64u) return fail(CA3D_ERR_UNSUPPORTED, "an ensemble steps 64^3 universes only (got %u): one workgroup holds one universe in its registers", grid_size);
	if (n_universes == 0 || n_universes > (1u << 20)) return fail(CA3D_ERR_INVALID_ARGUMENT, "an ensemble holds 1 to %u universes (got %u)", 1u << 20, n_universes);
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	free_arrays(e);
	const size_t state_bytes = (size_t)n_universes * kEnsembleWords * sizeof(uint32_t), word_bytes = (size_t)n_universes * sizeof(uint32_t);
	hipError_t err = hipMalloc((void **)&e->state, state_bytes);
	if (err == hipSuccess) err = hipMalloc((void **)&e->prev, state_bytes);
	if (err == hipSuccess) err = hipMalloc((void **)&e->rules, word_bytes * ensemble_rule_words(neighbourhood, clustered));
	if (err == hipSuccess) err = hipMalloc((void **)&e->steps_done, word_bytes);
	if (err == hipSuccess) err = hipMalloc((void **)&e->reason, word_bytes);
	if (err == hipSuccess) err = hipMalloc((void **)&e->records, (size_t)n_universes * sizeof(ca3d_summary));
	if (err != hipSuccess)
	{
		free_arrays(e);
		(void)hipGetLastError();
		return fail(err == hipErrorOutOfMemory ? CA3D_ERR_OUT_OF_MEMORY : CA3D_ERR_DEVICE, "allocating %u universes: %s", n_universes, hipGetErrorString(err));
	}
	e->n = n_universes;
	e->neighbourhood = neighbourhood;
	e->clustered = clustered;
	e->boundary = CA3D_ENSEMBLE_BOUNDARY_REFERENCE;
	e->has_rules.assign(n_universes, 0);
	e->has_state.assign(n_universes, 0);
	e->missing_rules = e->missing_state = n_universes;
	return CA3D_OK;
}

// the events of a pair that are not there yet
int create_timer(Timer &t)
{
	if (!t.start) HIP_TRY(hipEventCreate(&t.start));
	if (!t.stop) HIP_TRY(hipEventCreate(&t.stop));
	return CA3D_OK;
}

// room for `bytes` bytes in a staging array of the handle, and the events of the call that asks: its pair (`timer`) and, for a call that
// reads another handle, the event that orders it behind that handle's stream (`order`, without timing), each created when it is not there
// yet. The new array first: a failure leaves the handle as it was; then the stream is drained, since a call that was only enqueued may still
// be using the old one. `what` and its arguments word what could not be had: "allocating <what>: <HIP's reason>".
__attribute__((format(printf, 6, 7))) int reserve(ca3d_ensemble *e, Scratch &s, size_t bytes, Timer *timer, hipEvent_t *order, const char *what, ...)
{
	if (timer)
	{
		const int rc = create_timer(*timer);
		if (rc) return rc;
	}
	if (order && !*order) HIP_TRY(hipEventCreateWithFlags(order, hipEventDisableTiming));
	if (bytes <= s.bytes) return CA3D_OK;
	uint8_t *grown = nullptr;
	const hipError_t err = hipMalloc((void **)&grown, bytes);
	if (err != hipSuccess)
	{
		(void)hipGetLastError();
		char noun[256];
		va_list ap;
		va_start(ap, what);
		vsnprintf(noun, sizeof noun, what, ap);
		va_end(ap);
		return fail(err == hipErrorOutOfMemory ? CA3D_ERR_OUT_OF_MEMORY : CA3D_ERR_DEVICE, "allocating %s: %s", noun, hipGetErrorString(err));
	}
	if (s.array)
	{
		HIP_TRY(hipStreamSynchronize(e->stream));
		hipFree(s.array);
	}
	s.array = grown;
	s.bytes = bytes;
	return CA3D_OK;
}

// `total` steps at most for every universe, as launches of at most kEnsembleMaxSteps steps whose ends fall on check points; with a
// stop mask a universe leaves at the first check point at which one of its conditions holds. samples_per_universe != 0: a traced run —
// check points are reached whatever the mask, and each leaves a sample in e->trace
int run(ca3d_ensemble *e, uint32_t total, uint32_t check_every, uint32_t stop_mask, uint32_t samples_per_universe = 0)
{
	const bool checks = stop_mask || samples_per_universe;
	HIP_TRY(hipEventRecord(e->run_time.start, e->stream));
	uint64_t launches = 0;
	uint32_t base = 0;
	do
	{
		uint32_t n = total - base;
		if (n > kEnsembleMaxSteps)
		{
			n = kEnsembleMaxSteps;
			if (checks && check_every <= kEnsembleMaxSteps) n -= (base + n) % check_every; // end on a check point (base is one)
		}
		EnsembleLaunch l = launch_of(e);
		l.steps = n;
		l.base = base;
		l.check_every = check_every;
		l.stop_mask = stop_mask;
		if (stop_mask & CA3D_STOP_MOVING) l.cycle = e->moving; // the *_moving kernels' wider record
		l.final = base + n == total;
		if (samples_per_universe) { l.samples = e->trace.at<uint32_t>(); l.sample_stride = samples_per_universe; }
		HIP_TRY(launch_ensemble(l, e->stream));
		launches++;
		base += n;
	} while (base < total);
	HIP_TRY(hipEventRecord(e->run_time.stop, e->stream));
	e->timed = true;
	e->last_launches = launches;
	return CA3D_OK;
}

// ca3d_ensemble_step_until (known: EXTINCT | STILL, period null) and ca3d_ensemble_step_until_cycle (known: + PERIODIC). Without
// CA3D_STOP_PERIODIC in the mask the launches are the first call's whatever the entry point: the *_cycle kernels run only when asked for.
// ca3d_ensemble_step_until_moving (known: + MOVING, shift): the *_moving kernels run only with CA3D_STOP_MOVING in the mask.
// ca3d_ensemble_step_until_trace passes `trace` (known: EXTINCT | STILL): the *_trace kernels run whatever the mask, 0 included.
struct TraceOut
{
	uint32_t *samples, samples_per_universe, *n_samples;
};
// samples of one universe in a traced call: check points 0, check_every, ... and the last one at max_steps
uint64_t trace_capacity(uint32_t max_steps, uint32_t check_every) { return ((uint64_t)max_steps + check_every - 1u) / check_every + 1u; }

int step_until(ca3d_ensemble *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t known, uint32_t *steps_done, uint32_t *reason,
               uint32_t *period, const TraceOut *trace = nullptr, int32_t *shift = nullptr)
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (check_every == 0) return fail(CA3D_ERR_INVALID_ARGUMENT, "check_every must be at least 1");
	if (stop_mask & ~known) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in stop_mask %#x", stop_mask);
	int rc = ensemble_ready(e);
	if (rc) return rc;
	const uint64_t K = trace ? trace_capacity(max_steps, check_every) : 0u;
	if (trace && !trace->samples) return fail(CA3D_ERR_INVALID_ARGUMENT, "samples is NULL");
	if (trace && trace->samples_per_universe < K)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "samples_per_universe %u: %u steps checked every %u leave K = %llu samples per universe", trace->samples_per_universe,
		            max_steps, check_every, (unsigned long long)K);
	HIP_TRY(hipSetDevice(e->device));
	const size_t word_bytes = (size_t)e->n * sizeof(uint32_t);
	const bool moving = (stop_mask & CA3D_STOP_MOVING) != 0u;   // the *_moving kernels: their record is e->moving, eight words a universe
	const bool cycle = (stop_mask & CA3D_STOP_PERIODIC) != 0u && !moving; // the *_cycle kernels: e->cycle, four words
	const uint32_t rec_words = moving ? 8u : 4u;
	uint32_t *&rec = moving ? e->moving : e->cycle;
	const size_t sample_words = (size_t)e->n * (size_t)K * 3u;
	if (trace && (rc = reserve(e, e->trace, sample_words * sizeof(uint32_t), nullptr, nullptr, "%llu samples of %u universes", (unsigned long long)K, e->n))) return rc;
	if ((cycle || moving) && (!e->anchor || !rec))
	{
		const bool had_anchor = e->anchor != nullptr;
		hipError_t err = had_anchor ? hipSuccess : hipMalloc((void **)&e->anchor, (size_t)e->n * kEnsembleWords * sizeof(uint32_t));
		if (err == hipSuccess && !rec) err = hipMalloc((void **)&rec, rec_words * word_bytes);
		if (err != hipSuccess)
		{
			if (!had_anchor && e->anchor) hipFree(e->anchor);
			if (!had_anchor) e->anchor = nullptr;
			(void)hipGetLastError();
			return fail(err == hipErrorOutOfMemory ? CA3D_ERR_OUT_OF_MEMORY : CA3D_ERR_DEVICE, "allocating the anchors of %u universes: %s", e->n, hipGetErrorString(err));
		}
	}
	std::vector<uint32_t> done(e->n, stop_mask ? 0u : max_steps), fired(e->n, 0u), cyc(cycle || moving ? rec_words * (size_t)e->n : 0u, 0u);
	std::vector<uint32_t> got(sample_words); // [n][K][3]: staged, so that a failure below leaves the caller's array as it was
	e->last_launches = 0;
	e->timed = false;
	if (stop_mask || trace)
	{
		if (stop_mask)
		{
			// the kernel keeps both arrays: a universe whose reason word is set leaves the later launches of this call at once
			HIP_TRY(hipMemsetAsync(e->steps_done, 0, word_bytes, e->stream));
			HIP_TRY(hipMemsetAsync(e->reason, 0, word_bytes, e->stream));
		}
		if (cycle || moving) HIP_TRY(hipMemsetAsync(rec, 0, rec_words * word_bytes, e->stream)); // no anchor survives a call
		if (trace) HIP_TRY(hipMemsetAsync(e->trace.array, 0, sample_words * sizeof(uint32_t), e->stream)); // slots no check point reaches stay zero
		rc = run(e, max_steps, check_every, stop_mask, trace ? (uint32_t)K : 0u); // max_steps == 0: one launch that only checks
		if (rc) return rc;
		if (stop_mask)
		{
			HIP_TRY(hipMemcpyAsync(done.data(), e->steps_done, word_bytes, hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipMemcpyAsync(fired.data(), e->reason, word_bytes, hipMemcpyDeviceToHost, e->stream));
		}
		if (cycle || moving) HIP_TRY(hipMemcpyAsync(cyc.data(), rec, rec_words * word_bytes, hipMemcpyDeviceToHost, e->stream));
		if (trace) HIP_TRY(hipMemcpyAsync(got.data(), e->trace.array, sample_words * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
	}
	else if (max_steps)
	{
		rc = run(e, max_steps, 1u, 0u); // nothing to watch: plain stepping
		if (rc) return rc;
	}
	HIP_TRY(hipStreamSynchronize(e->stream));
	uint64_t sum = 0, most = 0;
	for (uint32_t d : done) { sum += d; most = d > most ? d : most; }
	e->last_steps = most;
	e->last_cell_steps = (double)sum * (double)(64 * 64 * 64);
	if (steps_done) memcpy(steps_done, done.data(), word_bytes);
	if (reason) memcpy(reason, fired.data(), word_bytes);
	if (period)
		for (uint32_t u = 0; u < e->n; u++) period[u] = cycle || moving ? cyc[rec_words * (size_t)u + 2u] : 0u;
	if (shift)
		for (uint32_t u = 0; u < e->n; u++)
		{
			// word 3 of a universe's record: dx, dy, dz as signed bytes, zero unless CA3D_STOP_MOVING fired
			const uint32_t packed = moving ? cyc[8u * (size_t)u + 3u] : 0u;
			for (int i = 0; i < 3; i++) shift[3u * (size_t)u + i] = (int32_t)(int8_t)(uint8_t)(packed >> (8 * i));
		}
	if (trace)
	{
		const size_t per = (size_t)trace->samples_per_universe * 3u, mine = (size_t)K * 3u;
		for (uint32_t u = 0; u < e->n; u++)
		{
			memcpy(trace->samples + u * per, got.data() + u * mine, mine * sizeof(uint32_t));
			memset(trace->samples + u * per + mine, 0, (per - mine) * sizeof(uint32_t));
			// a universe reached the check points up to the one it left at: steps_done is a multiple of check_every, or max_steps
			if (trace->n_samples) trace->n_samples[u] = (uint32_t)trace_capacity(done[u], check_every);
		}
	}
	return CA3D_OK;
}

// room for a sheet of `px` pixels in the three targets, and the counters; a failure leaves the handle with what it had
int size_sheet_targets(ca3d_ensemble *e, size_t px)
{
	if (!e->sheet_counters) HIP_TRY(hipMalloc((void **)&e->sheet_counters, 3u * sizeof(unsigned long long)));
	const int rc = create_timer(e->sheet_time);
	if (rc) return rc;
	if (px <= e->sheet_px) return CA3D_OK;
	uint32_t *present = nullptr, *depth = nullptr;
	uint2 *light = nullptr;
	hipError_t err = hipMalloc((void **)&present, px * 4u);
	if (err == hipSuccess) err = hipMalloc((void **)&light, px * 8u);
	if (err == hipSuccess) err = hipMalloc((void **)&depth, px * 4u);
	if (err != hipSuccess)
	{
		for (void *p : {(void *)present, (void *)light, (void *)depth})
			if (p) hipFree(p);
		(void)hipGetLastError();
		return fail(err == hipErrorOutOfMemory ? CA3D_ERR_OUT_OF_MEMORY : CA3D_ERR_DEVICE, "allocating a sheet of %zu pixels: %s", px, hipGetErrorString(err));
	}
	if (e->sheet_px)
	{
		HIP_TRY(hipStreamSynchronize(e->stream)); // a sheet that was only enqueued may still be drawing into the old targets
		for (void *p : {(void *)e->sheet_present, (void *)e->sheet_light, (void *)e->sheet_depth}) hipFree(p);
	}
	e->sheet_present = present; e->sheet_light = light; e->sheet_depth = depth;
	e->sheet_px = px;
	return CA3D_OK;
}

// ca3d_ensemble_isolate_connected and ca3d_ensemble_compose write universes [dst_first, dst_first + n) of `dst` from universes of `src`,
// which may be the same handle. The three checks below are called where each entry point has always made them, between its own.
// `into`: "jobs into" / "destinations in"
int check_destinations(const ca3d_ensemble *dst, const ca3d_ensemble *src, uint32_t dst_first, uint32_t n, const char *into)
{
	if (!dst->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called for the destination ensemble");
	if (!src->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called for the source ensemble");
	if (n == 0 || dst_first >= dst->n || n > dst->n - dst_first)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "%u %s universes [%u, %u + %u) of %u", n, into, dst_first, dst_first, n, dst->n);
	return CA3D_OK;
}

// `flag`: the name of the call's COPY_RULES flag
int check_same_device_and_kind(const ca3d_ensemble *dst, const ca3d_ensemble *src, bool copy_rules, const char *flag)
{
	if (src->device != dst->device) return fail(CA3D_ERR_INVALID_ARGUMENT, "the source ensemble is on device %d, the destination on device %d", src->device, dst->device);
	if (copy_rules && (src->neighbourhood != dst->neighbourhood || src->clustered != dst->clustered))
		return fail(CA3D_ERR_UNSUPPORTED, "%s: source and destination ensemble differ in neighbourhood or in being clustered (%u and %u rule words a universe)", flag,
		            rule_words(src), rule_words(dst));
	return CA3D_OK;
}

// item `index` (`item`: "job" / "part") reads source universe u, which the caller has found to be one of src's: not a destination of
// the same call, and with a state and, where the item's rule is copied, a rule. (Inlined: a call has tens of thousands of items, and with this
// check as a call of its own a compose of 25 000 parts took up to 0.2 ms longer on the host in two of six measured layouts)
__attribute__((always_inline)) inline int check_source(const ca3d_ensemble *dst, const ca3d_ensemble *src, uint32_t dst_first, uint32_t n, const char *item, uint32_t index, uint32_t u, bool need_rules)
{
	if (src == dst && u >= dst_first && u - dst_first < n)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "%s %u: source universe %u lies among the destinations [%u, %u + %u) of the same ensemble", item, index, u, dst_first, dst_first, n);
	if (!src->has_state[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "%s %u: ca3d_ensemble_upload_state has not been called for source universe %u", item, index, u);
	if (need_rules && !src->has_rules[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "%s %u: ca3d_ensemble_set_rules has not been called for source universe %u", item, index, u);
	return CA3D_OK;
}

// what follows on dst's stream comes behind what is queued on the source's stream now
int wait_for_source(ca3d_ensemble *dst, ca3d_ensemble *src, hipEvent_t order)
{
	if (src == dst) return CA3D_OK;
	HIP_TRY(hipEventRecord(order, src->stream));
	HIP_TRY(hipStreamWaitEvent(dst->stream, order, 0));
	return CA3D_OK;
}

// behind the launch that wrote the destinations: their records, the call's own records (the head of `staged`, `out_bytes` bytes) into
// `out` when it is asked for, and the wait — the caller's jobs or parts are consumed, and the source may go on
int finish_destinations(ca3d_ensemble *dst, uint32_t dst_first, uint32_t n, const Scratch &staged, const Timer &timer, void *out, size_t out_bytes, float *gpu_ms)
{
	const int rc = reset_records(dst, dst_first, n);
	if (rc) return rc;
	if (out) HIP_TRY(hipMemcpyAsync(out, staged.array, out_bytes, hipMemcpyDeviceToHost, dst->stream));
	HIP_TRY(hipStreamSynchronize(dst->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, timer.start, timer.stop));
	mark_state(dst, dst_first, n);
	return CA3D_OK;
}

// ca3d_cut_windows (`cut`: the ensemble is written, its universes must be distinct) and ca3d_stamp_windows (the ensemble is read, its
// universes must hold a state): everything the two calls refuse, looked at before either handle is touched
int check_windows(const ca3d_engine *h, const ca3d_ensemble *e, uint32_t n, const ca3d_window *w, bool cut)
{
	if (!h) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL engine handle");
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!w) return fail(CA3D_ERR_INVALID_ARGUMENT, "windows is NULL");
	if (n == 0 || n > kWindowsMax) return fail(CA3D_ERR_INVALID_ARGUMENT, "a call takes 1 to %u windows (got %u)", kWindowsMax, n);
	if (!h->configured) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_configure has not been called for the engine");
	if (!e->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called for the ensemble");
	if (h->layout != CA3D_LAYOUT_PACKED32) return fail(CA3D_ERR_UNSUPPORTED, "windows are cut from and stamped into the packed layout only");
	if (h->slab) return fail(CA3D_ERR_UNSUPPORTED, "windows are cut from and stamped into a full-grid engine, not a slab (ca3d_configure_slab, the ranks of a group)");
	if (h->G < 64u) return fail(CA3D_ERR_UNSUPPORTED, "a window is 64^3 cells: the grid must be 64 or more a side (got %u)", h->G);
	if (h->device != e->device) return fail(CA3D_ERR_INVALID_ARGUMENT, "the engine is on device %d, the ensemble on device %d", h->device, e->device);
	if (cut && !h->has_state) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_upload_state has not been called for the engine: no state to cut from");
	std::vector<uint8_t> taken(cut && n > 1u ? e->n : 0u, 0);
	for (uint32_t k = 0; k < n; k++)
	{
		const uint32_t u = w[k].universe;
		if (u >= e->n) return fail(CA3D_ERR_INVALID_ARGUMENT, "window %u: universe %u of %u", k, u, e->n);
		for (int i = 0; i < 3; i++)
			if (w[k].origin[i] >= h->G) return fail(CA3D_ERR_INVALID_ARGUMENT, "window %u: origin[%d] = %u — an origin lies below the grid size %u", k, i, w[k].origin[i], h->G);
		if (!cut && !e->has_state[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "window %u: ca3d_ensemble_upload_state has not been called for universe %u", k, u);
		if (!taken.empty())
		{
			if (taken[u]) return fail(CA3D_ERR_INVALID_ARGUMENT, "window %u: universe %u is the destination of an earlier window of the call", k, u);
			taken[u] = 1;
		}
	}
	return CA3D_OK;
}

// the engine's state as it is after every step requested so far, on its stream: what ca3d_read_state does before it looks
int settle_engine(ca3d_engine *h)
{
	FLUSH_QUEUED(h);
	const int rc = bind_device(h); // (joins the frames in flight)
	if (rc) return rc;
	return settle_resident(h);
}

// the call's windows into the ensemble's staging array, on `stream`, behind what `behind` holds now
int stage_windows(ca3d_ensemble *e, uint32_t n, const ca3d_window *w, hipStream_t stream, hipStream_t behind)
{
	HIP_TRY(hipEventRecord(e->windows_src, behind));
	HIP_TRY(hipStreamWaitEvent(stream, e->windows_src, 0));
	// (from pageable memory: the copy has left the caller's array when the call returns)
	HIP_TRY(hipMemcpyAsync(e->windows.array, w, (size_t)n * sizeof(ca3d_window), hipMemcpyHostToDevice, stream));
	return CA3D_OK;
}

// the three getters of what a configure or ca3d_ensemble_set_boundary chose
template <class T> int get_setting(const ca3d_ensemble *e, int *out, T ca3d_ensemble::*setting)
{
	if (!e || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!e->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called");
	*out = (int)(e->*setting);
	return CA3D_OK;
}

} // namespace

extern "C"
{

int ca3d_ensemble_create(int device, ca3d_ensemble_t **out) CA3D_API_TRY
{
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	*out = nullptr;
	int n = 0;
	hipError_t err = hipGetDeviceCount(&n);
	if (err != hipSuccess || n <= 0)
		return fail(CA3D_ERR_DEVICE, "no HIP device available (%s); an ensemble has no CPU fallback", err != hipSuccess ? hipGetErrorString(err) : "device count is 0");
	if (device < 0 || device >= n) return fail(CA3D_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, n);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(CA3D_ERR_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
	ca3d_ensemble *e = new (std::nothrow) ca3d_ensemble();
	if (!e) return fail(CA3D_ERR_OUT_OF_MEMORY, "out of host memory");
	e->device = device;
	err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
	if (err == hipSuccess) err = hipEventCreate(&e->run_time.start);
	if (err == hipSuccess) err = hipEventCreate(&e->run_time.stop);
	if (err != hipSuccess)
	{
		ca3d_ensemble_destroy(e);
		return fail(CA3D_ERR_DEVICE, "ensemble set-up failed: %s", hipGetErrorString(err));
	}
	*out = e;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_destroy(ca3d_ensemble_t *e) CA3D_API_TRY
{
	if (!e) return CA3D_OK;
	hipSetDevice(e->device);
	if (e->stream) hipStreamSynchronize(e->stream);
	free_arrays(e);
	for (const Timer &t : {e->run_time, e->sheet_time, e->census_time, e->isolate_time, e->compose_time, e->canon_time, e->canon_period_time, e->envelope_time, e->damage_time, e->usage_time, e->windows_time})
		for (hipEvent_t ev : {t.start, t.stop})
			if (ev) hipEventDestroy(ev);
	for (hipEvent_t ev : {e->ev_seed, e->isolate_src, e->compose_src, e->envelope_src, e->damage_src, e->windows_src})
		if (ev) hipEventDestroy(ev);
	if (e->stream) hipStreamDestroy(e->stream);
	delete e;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_configure(ca3d_ensemble_t *e, uint32_t grid_size, uint32_t n_universes) CA3D_API_TRY
{
	return configure_ensemble(e, grid_size, n_universes, CA3D_ENSEMBLE_VON_NEUMANN);
}
CA3D_API_CATCH

int ca3d_ensemble_configure_neighbourhood(ca3d_ensemble_t *e, uint32_t grid_size, uint32_t n_universes, int neighbourhood) CA3D_API_TRY
{
	return configure_ensemble(e, grid_size, n_universes, neighbourhood);
}
CA3D_API_CATCH

int ca3d_ensemble_configure_clustered(ca3d_ensemble_t *e, uint32_t grid_size, uint32_t n_universes) CA3D_API_TRY
{
	return configure_ensemble(e, grid_size, n_universes, CA3D_ENSEMBLE_MOORE, true);
}
CA3D_API_CATCH

int ca3d_ensemble_get_clustered(ca3d_ensemble_t *e, int *out) CA3D_API_TRY
{
	return get_setting(e, out, &ca3d_ensemble::clustered);
}
CA3D_API_CATCH

int ca3d_ensemble_get_neighbourhood(ca3d_ensemble_t *e, int *out) CA3D_API_TRY
{
	return get_setting(e, out, &ca3d_ensemble::neighbourhood);
}
CA3D_API_CATCH

// (host state only: the launches already queued carry the boundary they were queued under in their kernel)
int ca3d_ensemble_set_boundary(ca3d_ensemble_t *e, int boundary) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!e->n) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_configure has not been called");
	if (boundary != CA3D_ENSEMBLE_BOUNDARY_REFERENCE && boundary != CA3D_ENSEMBLE_BOUNDARY_TORUS && boundary != CA3D_ENSEMBLE_BOUNDARY_CLOSED)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown ensemble boundary %d (CA3D_ENSEMBLE_BOUNDARY_REFERENCE = 0, CA3D_ENSEMBLE_BOUNDARY_TORUS = 1, CA3D_ENSEMBLE_BOUNDARY_CLOSED = 2)",
		            boundary);
	e->boundary = boundary;
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_get_boundary(ca3d_ensemble_t *e, int *out) CA3D_API_TRY
{
	return get_setting(e, out, &ca3d_ensemble::boundary);
}
CA3D_API_CATCH

int ca3d_ensemble_set_rules(ca3d_ensemble_t *e, uint32_t universe, const int32_t *main_offsets, uint32_t n_main, const int32_t *edges_offsets,
                            uint32_t n_edges, const int32_t *corners_offsets, uint32_t n_corners, const uint32_t survive[CA3D_LUT_LEN],
                            const uint32_t born[CA3D_LUT_LEN]) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	const bool all = universe == CA3D_ENSEMBLE_ALL;
	int rc = check_range(e, all ? 0u : universe, all ? e->n : 1u);
	if (rc) return rc;
	const std::string who = all ? std::string("every universe") : "universe " + std::to_string(universe);
	CanonRules r;
	std::string err;
	rc = canonicalize_rules(main_offsets, n_main, edges_offsets, n_edges, corners_offsets, n_corners, survive, born, &r, &err);
	if (rc) return fail(rc, "%s: %s", who.c_str(), err.c_str());
	uint32_t lut_s, lut_b;
	const uint32_t first = all ? 0u : universe, count = all ? e->n : 1u;
	if (e->clustered)
	{
		// r.fast: a side list whose count matters IS the standard one; a side table whose count does not matter is a constant over the
		// counts its own list can reach (slot 0 is always one of them), and is stored as that constant over the standard list's counts
		if (r.main != MAIN_MOORE || !r.fast)
			return fail(CA3D_ERR_UNSUPPORTED, "%s: this ensemble is clustered and takes rules whose main list is Moore and whose edges / corners lists are the standard ones",
			            who.c_str());
		uint32_t b3[3] = {r.onset_born[0], 0u, 0u}, s3[3] = {r.onset_survive[0], 0u, 0u};
		for (int s = 1; s < 3; s++)
		{
			b3[s] = r.need[s] ? r.onset_born[s] : 0u - (r.onset_born[s] & 1u);
			s3[s] = r.need[s] ? r.onset_survive[s] : 0u - (r.onset_survive[s] & 1u);
		}
		uint32_t one[6];
		pack_clustered(b3, s3, one);
		return store_rule_repeated(e, first, count, one);
	}
	if (moore(e))
	{
		if (r.main != MAIN_MOORE || !side_tables_silent(r))
			return fail(CA3D_ERR_UNSUPPORTED, "%s: this ensemble is Moore and takes rules that reduce to a Moore table pair (main list Moore, edges / corners tables that cannot fire; "
			                                  "tables that fire want a clustered ensemble, ca3d_ensemble_configure_clustered)",
			            who.c_str());
		lut_s = r.onset_survive[0];
		lut_b = r.onset_born[0];
	}
	else
	{
		if (!vn_rule_applies(r, -1))
			return fail(CA3D_ERR_UNSUPPORTED, "%s: an ensemble takes rules that reduce to a von Neumann table pair (main list von Neumann, edges / corners tables that cannot fire)",
			            who.c_str());
		vn_tables(r, &lut_s, &lut_b);
	}
	const uint32_t mask = (1u << table_bits(e)) - 1u;
	uint32_t one[2];
	pack_rule(e, lut_b & mask, lut_s & mask, one);
	return store_rule_repeated(e, first, count, one);
}
CA3D_API_CATCH

int ca3d_ensemble_upload_state(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *words, size_t n_words) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (!words || n_words != (size_t)count * kEnsembleWords)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "%u universes take %zu words (got %zu)", count, (size_t)count * kEnsembleWords, n_words);
	HIP_TRY(hipSetDevice(e->device));
	const size_t off = (size_t)first * kEnsembleWords, bytes = n_words * sizeof(uint32_t);
	HIP_TRY(hipMemcpyAsync(e->state + off, words, bytes, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->prev + off, e->state + off, bytes, hipMemcpyDeviceToDevice, e->stream)); // the same words in both buffers, as ca3d_upload_state
	if ((rc = reset_records(e, first, count))) return rc;
	HIP_TRY(hipStreamSynchronize(e->stream)); // the caller's buffer is consumed when the call returns
	mark_state(e, first, count);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_seed_state(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const ca3d_seed *specs, uint32_t n_specs) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!specs) return fail(CA3D_ERR_INVALID_ARGUMENT, "specs is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (n_specs != 1u && n_specs != count) return fail(CA3D_ERR_INVALID_ARGUMENT, "%u universes take 1 or %u specs (got %u)", count, count, n_specs);
	for (uint32_t k = 0; k < n_specs; k++)
		if (const char *why = seed_spec_error(specs[k], 64u))
			return fail(CA3D_ERR_INVALID_ARGUMENT, "seed spec of universe %u: %s (box (%u, %u, %u) .. (%u, %u, %u), and_rounds %u)", first + k, why, specs[k].box_min[0],
			            specs[k].box_min[1], specs[k].box_min[2], specs[k].box_max[0], specs[k].box_max[1], specs[k].box_max[2], specs[k].and_rounds);
	HIP_TRY(hipSetDevice(e->device));
	const ca3d_seed *on_device = nullptr; // one spec for all travels as a kernel argument
	if (n_specs > 1u)
	{
		if (!e->seed_dev) HIP_TRY(hipMalloc((void **)&e->seed_dev, (size_t)e->n * sizeof(ca3d_seed)));
		if (!e->seed_host) HIP_TRY(hipHostMalloc((void **)&e->seed_host, (size_t)e->n * sizeof(ca3d_seed), hipHostMallocDefault));
		if (!e->ev_seed) HIP_TRY(hipEventCreateWithFlags(&e->ev_seed, hipEventDisableTiming));
		else HIP_TRY(hipEventSynchronize(e->ev_seed)); // the staging copy is free again once the last call's copy out of it is done
		// the caller's array is consumed here; the copy and the fill are stream-ordered behind whatever still reads the device copy
		memcpy(e->seed_host, specs, (size_t)count * sizeof(ca3d_seed));
		HIP_TRY(hipMemcpyAsync(e->seed_dev, e->seed_host, (size_t)count * sizeof(ca3d_seed), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipEventRecord(e->ev_seed, e->stream));
		on_device = e->seed_dev;
	}
	HIP_TRY(launch_seed_ensemble(e->state, e->prev, first, count, on_device, specs[0], e->stream)); // both buffers of every universe in one pass
	if ((rc = reset_records(e, first, count))) return rc;
	mark_state(e, first, count);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_set_rule_tables(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *born_masks, const uint32_t *survive_masks,
                                  uint32_t n_masks) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!born_masks || !survive_masks) return fail(CA3D_ERR_INVALID_ARGUMENT, "a mask array is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (n_masks != 1u && n_masks != count) return fail(CA3D_ERR_INVALID_ARGUMENT, "%u universes take 1 or %u mask pairs (got %u)", count, count, n_masks);
	const uint32_t bits = table_bits(e), per = rule_words(e);
	std::vector<uint32_t> words((size_t)count * per);
	for (uint32_t k = 0; k < count; k++)
	{
		const uint32_t b = born_masks[n_masks == 1u ? 0u : k], s = survive_masks[n_masks == 1u ? 0u : k];
		if ((b | s) >> bits)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "universe %u: born mask %#x / survive mask %#x — a %s count is 0 .. %u, bits %u and above mean nothing", first + k, b, s,
			            moore(e) ? "Moore" : "von Neumann", bits - 1u, bits);
		pack_rule(e, b, s, &words[(size_t)k * per]); // what ca3d_ensemble_set_rules stores
	}
	return store_rules(e, first, count, words);
}
CA3D_API_CATCH

int ca3d_ensemble_set_rule_tables_clustered(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *born_masks, const uint32_t *survive_masks,
                                            uint32_t n_rules) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!born_masks || !survive_masks) return fail(CA3D_ERR_INVALID_ARGUMENT, "a mask array is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (!e->clustered) return fail(CA3D_ERR_UNSUPPORTED, "this ensemble is not clustered (ca3d_ensemble_configure_clustered): a universe has one table pair, ca3d_ensemble_set_rule_tables sets it");
	if (n_rules != 1u && n_rules != count) return fail(CA3D_ERR_INVALID_ARGUMENT, "%u universes take 1 or %u rules (got %u)", count, count, n_rules);
	static const char *names[3] = {"main", "edges", "corners"};
	std::vector<uint32_t> words((size_t)count * 6u);
	for (uint32_t k = 0; k < count; k++)
	{
		const uint32_t *b = born_masks + (n_rules == 1u ? 0u : 3u * (size_t)k), *s = survive_masks + (n_rules == 1u ? 0u : 3u * (size_t)k);
		for (int i = 0; i < 3; i++)
			if ((b[i] | s[i]) >> kClusteredBits[i])
				return fail(CA3D_ERR_INVALID_ARGUMENT, "universe %u: %s born mask %#x / survive mask %#x — the count is 0 .. %u, bits %u and above mean nothing", first + k,
				            names[i], b[i], s[i], kClusteredBits[i] - 1u, kClusteredBits[i]);
		pack_clustered(b, s, &words[(size_t)k * 6u]); // what ca3d_ensemble_set_rules stores
	}
	return store_rules(e, first, count, words);
}
CA3D_API_CATCH

int ca3d_ensemble_read_state(ca3d_ensemble_t *e, uint32_t first, uint32_t count, uint32_t *words, size_t n_words) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (!words || n_words != (size_t)count * kEnsembleWords)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "%u universes hold %zu words (got %zu)", count, (size_t)count * kEnsembleWords, n_words);
	if ((rc = require_state(e, first, count))) return rc;
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipMemcpyAsync(words, e->state + (size_t)first * kEnsembleWords, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_step(ca3d_ensemble_t *e, uint32_t n_steps) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	int rc = ensemble_ready(e);
	if (rc) return rc;
	e->last_steps = n_steps;
	e->last_cell_steps = (double)n_steps * e->n * (double)(64 * 64 * 64);
	e->last_launches = 0;
	e->timed = false;
	if (n_steps == 0) return CA3D_OK;
	HIP_TRY(hipSetDevice(e->device));
	return run(e, n_steps, 1u, 0u);
}
CA3D_API_CATCH

int ca3d_ensemble_step_until(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                             uint32_t *reason) CA3D_API_TRY
{
	return step_until(e, max_steps, check_every, stop_mask, CA3D_STOP_EXTINCT | CA3D_STOP_STILL, steps_done, reason, nullptr);
}
CA3D_API_CATCH

int ca3d_ensemble_step_until_cycle(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                                   uint32_t *reason, uint32_t *period) CA3D_API_TRY
{
	return step_until(e, max_steps, check_every, stop_mask, CA3D_STOP_EXTINCT | CA3D_STOP_STILL | CA3D_STOP_PERIODIC, steps_done, reason, period);
}
CA3D_API_CATCH

int ca3d_ensemble_step_until_moving(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                                    uint32_t *reason, uint32_t *period, int32_t *shift) CA3D_API_TRY
{
	return step_until(e, max_steps, check_every, stop_mask, CA3D_STOP_EXTINCT | CA3D_STOP_STILL | CA3D_STOP_PERIODIC | CA3D_STOP_MOVING, steps_done, reason, period,
	                  nullptr, shift);
}
CA3D_API_CATCH

int ca3d_ensemble_step_until_trace(ca3d_ensemble_t *e, uint32_t max_steps, uint32_t check_every, uint32_t stop_mask, uint32_t *steps_done,
                                   uint32_t *reason, uint32_t *samples, uint32_t samples_per_universe, uint32_t *n_samples) CA3D_API_TRY
{
	const TraceOut out{samples, samples_per_universe, n_samples};
	return step_until(e, max_steps, check_every, stop_mask, CA3D_STOP_EXTINCT | CA3D_STOP_STILL, steps_done, reason, nullptr, &out);
}
CA3D_API_CATCH

int ca3d_ensemble_summarize(ca3d_ensemble_t *e, uint32_t first, uint32_t count, ca3d_summary *out) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if ((rc = require_state(e, first, count))) return rc;
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipMemcpyAsync(out, e->records + first, (size_t)count * sizeof(ca3d_summary), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_synchronize(ca3d_ensemble_t *e) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_get_stats(ca3d_ensemble_t *e, ca3d_stats *out) CA3D_API_TRY
{
	if (!e || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	*out = ca3d_stats{};
	out->steps = e->last_steps;
	out->kernel_launches = e->last_launches;
	out->cell_steps = e->last_cell_steps;
	out->algorithmic_bytes = 0.25 * e->last_cell_steps;
	if (e->timed)
	{
		HIP_TRY(hipSetDevice(e->device));
		HIP_TRY(hipEventSynchronize(e->run_time.stop));
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, e->run_time.start, e->run_time.stop));
		out->gpu_ms = ms;
	}
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_render_sheet(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const float uniforms[128], uint32_t tile_w, uint32_t tile_h,
                               uint32_t columns, uint32_t spp, uint8_t *presentation_rgba8, uint16_t *light_rgba16f, uint16_t *depth_rg16f) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!uniforms) return fail(CA3D_ERR_INVALID_ARGUMENT, "uniforms is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (columns == 0) return fail(CA3D_ERR_INVALID_ARGUMENT, "a sheet has at least one column of tiles");
	for (uint32_t t : {tile_w, tile_h})
		if (t < 16u || t > 1024u || t % 16u)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "bad tile size %ux%u: width and height are multiples of 16 from 16 to 1024", tile_w, tile_h);
	if (spp != 1 && spp != 4) return fail(CA3D_ERR_INVALID_ARGUMENT, "spp must be 1 or 4");
	const uint64_t rows = ((uint64_t)count + columns - 1u) / columns, W = (uint64_t)columns * tile_w, H = rows * tile_h;
	if (W * H > (1ull << 26)) // (columns < 2^32, tile_w <= 2^10, H <= 2^30: no overflow)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "a sheet of %llu x %llu pixels: at most 2^26 pixels", (unsigned long long)W, (unsigned long long)H);
	if ((rc = require_state(e, first, count))) return rc;
	HIP_TRY(hipSetDevice(e->device));
	const size_t px = (size_t)(W * H);
	if ((rc = size_sheet_targets(e, px))) return rc;
	SheetLaunch l{};
	l.state = e->state;
	l.first = first; l.count = count;
	l.tile_w = tile_w; l.tile_h = tile_h; l.columns = columns; l.spp = spp;
	l.uniforms = uniforms;
	l.presentation = e->sheet_present; l.light = e->sheet_light; l.depth = e->sheet_depth;
	l.counters = e->sheet_counters;
	e->sheet_drawn = false;
	HIP_TRY(hipMemsetAsync(e->sheet_counters, 0, 3u * sizeof(unsigned long long), e->stream));
	HIP_TRY(hipEventRecord(e->sheet_time.start, e->stream));
	HIP_TRY(launch_render_sheet(l, e->stream));
	HIP_TRY(hipEventRecord(e->sheet_time.stop, e->stream));
	e->sheet_drawn = true;
	e->sheet_primary_rays = (uint64_t)count * tile_w * tile_h * spp;
	if (presentation_rgba8) HIP_TRY(hipMemcpyAsync(presentation_rgba8, e->sheet_present, px * 4u, hipMemcpyDeviceToHost, e->stream));
	if (light_rgba16f) HIP_TRY(hipMemcpyAsync(light_rgba16f, e->sheet_light, px * 8u, hipMemcpyDeviceToHost, e->stream));
	if (depth_rg16f) HIP_TRY(hipMemcpyAsync(depth_rg16f, e->sheet_depth, px * 4u, hipMemcpyDeviceToHost, e->stream));
	if (presentation_rgba8 || light_rgba16f || depth_rg16f) HIP_TRY(hipStreamSynchronize(e->stream));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_get_sheet_stats(ca3d_ensemble_t *e, ca3d_render_stats *out) CA3D_API_TRY
{
	if (!e || !out) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL argument");
	if (!e->sheet_drawn) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_render_sheet has not been called yet");
	HIP_TRY(hipSetDevice(e->device));
	HIP_TRY(hipEventSynchronize(e->sheet_time.stop));
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, e->sheet_time.start, e->sheet_time.stop));
	unsigned long long c[3] = {0, 0, 0};
	HIP_TRY(hipMemcpyAsync(c, e->sheet_counters, sizeof c, hipMemcpyDeviceToHost, e->stream)); // behind the sheet; a sheet enqueued later has zeroed them
	HIP_TRY(hipStreamSynchronize(e->stream));
	*out = ca3d_render_stats{};
	out->gpu_ms = ms;
	out->primary_rays = e->sheet_primary_rays;
	out->shadow_rays = c[0];
	out->primary_cell_visits = c[1];
	out->shadow_cell_visits = c[2];
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_census(ca3d_ensemble_t *e, uint32_t first, uint32_t count, uint32_t max_components, ca3d_component *out, uint32_t *n_components,
                         uint32_t *remaining, float *gpu_ms) CA3D_API_TRY
{
	return ca3d_ensemble_census_connected(e, first, count, max_components, CA3D_CONNECT_CLOSED, out, n_components, remaining, gpu_ms);
}
CA3D_API_CATCH

int ca3d_ensemble_census_connected(ca3d_ensemble_t *e, uint32_t first, uint32_t count, uint32_t max_components, uint32_t connectivity,
                                   ca3d_component *out, uint32_t *n_components, uint32_t *remaining, float *gpu_ms) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!out || !n_components || !remaining) return fail(CA3D_ERR_INVALID_ARGUMENT, "out, n_components or remaining is NULL");
	if (connectivity > CA3D_CONNECT_TORUS) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown connectivity %u (CA3D_CONNECT_CLOSED = 0, CA3D_CONNECT_TORUS = 1)", connectivity);
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if (max_components == 0 || max_components > kCensusMaxComponents)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "max_components %u: a census lists 1 to %u components a universe", max_components, kCensusMaxComponents);
	if ((rc = require_state(e, first, count))) return rc;
	HIP_TRY(hipSetDevice(e->device));
	const size_t rec_bytes = (size_t)count * max_components * sizeof(ca3d_component), word_bytes = (size_t)count * sizeof(uint32_t), bytes = rec_bytes + 2u * word_bytes;
	if ((rc = reserve(e, e->census, bytes, &e->census_time, nullptr, "a census of %zu bytes", bytes))) return rc;
	CensusLaunch l{};
	l.state = e->state;
	l.first = first; l.count = count;
	l.max_components = max_components;
	l.connectivity = connectivity;
	l.out = e->census.at<ca3d_component>();
	l.n_components = e->census.at<uint32_t>(rec_bytes);
	l.remaining = l.n_components + count;
	HIP_TRY(hipEventRecord(e->census_time.start, e->stream));
	HIP_TRY(launch_census(l, e->stream));
	HIP_TRY(hipEventRecord(e->census_time.stop, e->stream));
	HIP_TRY(hipMemcpyAsync(out, l.out, rec_bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipMemcpyAsync(n_components, l.n_components, word_bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipMemcpyAsync(remaining, l.remaining, word_bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, e->census_time.start, e->census_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_isolate(ca3d_ensemble_t *dst, uint32_t dst_first, ca3d_ensemble_t *src, uint32_t n_jobs, const ca3d_isolate_job *jobs, uint32_t flags,
                          ca3d_isolated *out, float *gpu_ms) CA3D_API_TRY
{
	return ca3d_ensemble_isolate_connected(dst, dst_first, src, n_jobs, jobs, flags, CA3D_CONNECT_CLOSED, out, gpu_ms);
}
CA3D_API_CATCH

int ca3d_ensemble_isolate_connected(ca3d_ensemble_t *dst, uint32_t dst_first, ca3d_ensemble_t *src, uint32_t n_jobs, const ca3d_isolate_job *jobs,
                                    uint32_t flags, uint32_t connectivity, ca3d_isolated *out, float *gpu_ms) CA3D_API_TRY
{
	if (!dst || !src) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!jobs) return fail(CA3D_ERR_INVALID_ARGUMENT, "jobs is NULL");
	if (connectivity > CA3D_CONNECT_TORUS) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown connectivity %u (CA3D_CONNECT_CLOSED = 0, CA3D_CONNECT_TORUS = 1)", connectivity);
	int rc = check_destinations(dst, src, dst_first, n_jobs, "jobs into");
	if (rc) return rc;
	const uint32_t placement = flags & 0xFFu;
	const bool copy_rules = (flags & CA3D_ISOLATE_COPY_RULES) != 0u;
	if (placement > CA3D_ISOLATE_ORIGIN) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown placement %u (CA3D_ISOLATE_KEEP = 0, CA3D_ISOLATE_CENTRE = 1, CA3D_ISOLATE_ORIGIN = 2)", placement);
	if (flags & ~(0xFFu | CA3D_ISOLATE_COPY_RULES)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in flags %#x", flags);
	if ((rc = check_same_device_and_kind(dst, src, copy_rules, "CA3D_ISOLATE_COPY_RULES"))) return rc;
	for (uint32_t k = 0; k < n_jobs; k++)
	{
		const uint32_t u = jobs[k].universe;
		if (u >= src->n) return fail(CA3D_ERR_INVALID_ARGUMENT, "job %u: universe %u of %u", k, u, src->n);
		if (jobs[k].cell >= 1u << 18) return fail(CA3D_ERR_INVALID_ARGUMENT, "job %u: cell %u — a cell is x + 64 y + 4096 z, below %u", k, jobs[k].cell, 1u << 18);
		if ((rc = check_source(dst, src, dst_first, n_jobs, "job", k, u, copy_rules))) return rc;
	}
	HIP_TRY(hipSetDevice(dst->device));
	const size_t out_bytes = (size_t)n_jobs * sizeof(ca3d_isolated), job_bytes = (size_t)n_jobs * sizeof(ca3d_isolate_job), bytes = out_bytes + job_bytes;
	if ((rc = reserve(dst, dst->isolate, bytes, &dst->isolate_time, &dst->isolate_src, "%zu bytes of isolate jobs", bytes))) return rc;
	IsolateLaunch l{};
	l.src_state = src->state;
	l.dst_state = dst->state; l.dst_prev = dst->prev;
	l.src_rules = src->rules; l.dst_rules = dst->rules;
	l.out = dst->isolate.at<ca3d_isolated>();
	l.jobs = dst->isolate.at<const ca3d_isolate_job>(out_bytes);
	l.dst_first = dst_first; l.n_jobs = n_jobs;
	l.placement = placement;
	l.rule_words = copy_rules ? rule_words(dst) : 0u;
	l.connectivity = connectivity;
	if ((rc = wait_for_source(dst, src, dst->isolate_src))) return rc;
	HIP_TRY(hipMemcpyAsync(dst->isolate.array + out_bytes, jobs, job_bytes, hipMemcpyHostToDevice, dst->stream));
	HIP_TRY(hipEventRecord(dst->isolate_time.start, dst->stream));
	HIP_TRY(launch_isolate(l, dst->stream));
	HIP_TRY(hipEventRecord(dst->isolate_time.stop, dst->stream));
	if ((rc = finish_destinations(dst, dst_first, n_jobs, dst->isolate, dst->isolate_time, out, out_bytes, gpu_ms))) return rc;
	if (copy_rules) mark_rules(dst, dst_first, n_jobs);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_compose(ca3d_ensemble_t *dst, uint32_t dst_first, uint32_t n_dst, ca3d_ensemble_t *src, const ca3d_compose_part *parts,
                          const uint32_t *part_begin, uint32_t flags, ca3d_composed *out, float *gpu_ms) CA3D_API_TRY
{
	if (!dst || !src) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!part_begin) return fail(CA3D_ERR_INVALID_ARGUMENT, "part_begin is NULL");
	int rc = check_destinations(dst, src, dst_first, n_dst, "destinations in");
	if (rc) return rc;
	const bool over = (flags & CA3D_COMPOSE_OVER) != 0u, copy_rules = (flags & CA3D_COMPOSE_COPY_RULES) != 0u;
	if (flags & ~(CA3D_COMPOSE_OVER | CA3D_COMPOSE_COPY_RULES)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in flags %#x", flags);
	if (part_begin[0] != 0u) return fail(CA3D_ERR_INVALID_ARGUMENT, "part_begin[0] is %u, not 0", part_begin[0]);
	for (uint32_t k = 0; k < n_dst; k++)
		if (part_begin[k + 1] < part_begin[k])
			return fail(CA3D_ERR_INVALID_ARGUMENT, "part_begin decreases: part_begin[%u] = %u, part_begin[%u] = %u", k, part_begin[k], k + 1, part_begin[k + 1]);
	const uint32_t n_parts = part_begin[n_dst];
	if (n_parts > CA3D_COMPOSE_MAX_PARTS) return fail(CA3D_ERR_INVALID_ARGUMENT, "%u parts: a call takes %u at most", n_parts, CA3D_COMPOSE_MAX_PARTS);
	if (n_parts && !parts) return fail(CA3D_ERR_INVALID_ARGUMENT, "parts is NULL");
	if ((rc = check_same_device_and_kind(dst, src, copy_rules, "CA3D_COMPOSE_COPY_RULES"))) return rc;
	for (uint32_t k = 0; k < n_dst; k++)
	{
		if (over && !dst->has_state[dst_first + k])
			return fail(CA3D_ERR_NOT_CONFIGURED, "CA3D_COMPOSE_OVER: ca3d_ensemble_upload_state has not been called for destination universe %u", dst_first + k);
		for (uint32_t i = part_begin[k]; i < part_begin[k + 1]; i++)
		{
			const ca3d_compose_part &p = parts[i];
			if (p.universe >= src->n) return fail(CA3D_ERR_INVALID_ARGUMENT, "part %u: universe %u of %u", i, p.universe, src->n);
			if (p.orientation >= 48u) return fail(CA3D_ERR_INVALID_ARGUMENT, "part %u: orientation %u — an orientation is 0 .. 47", i, p.orientation);
			for (int d = 0; d < 3; d++)
				if (p.at[d] < -64 || p.at[d] > 64) return fail(CA3D_ERR_INVALID_ARGUMENT, "part %u: at[%d] = %d lies outside -64 .. 64", i, d, p.at[d]);
			if (p.reserved != 0u) return fail(CA3D_ERR_INVALID_ARGUMENT, "part %u: reserved is %u, not 0", i, p.reserved);
			// (a destination takes the rule of its first part)
			if ((rc = check_source(dst, src, dst_first, n_dst, "part", i, p.universe, copy_rules && i == part_begin[k]))) return rc;
		}
	}
	HIP_TRY(hipSetDevice(dst->device));
	const size_t out_bytes = (size_t)n_dst * sizeof(ca3d_composed), part_bytes = (size_t)n_parts * sizeof(ca3d_compose_part),
	             begin_bytes = ((size_t)n_dst + 1u) * sizeof(uint32_t), bytes = out_bytes + part_bytes + begin_bytes;
	if ((rc = reserve(dst, dst->compose, bytes, &dst->compose_time, &dst->compose_src, "%zu bytes of compose parts", bytes))) return rc;
	ComposeLaunch l{};
	l.src_state = src->state;
	l.dst_state = dst->state; l.dst_prev = dst->prev;
	l.src_rules = src->rules; l.dst_rules = dst->rules;
	l.out = dst->compose.at<ca3d_composed>();
	l.parts = dst->compose.at<const ca3d_compose_part>(out_bytes);
	l.part_begin = dst->compose.at<const uint32_t>(out_bytes + part_bytes);
	l.dst_first = dst_first; l.n_dst = n_dst;
	l.over = over;
	l.rule_words = copy_rules ? rule_words(dst) : 0u;
	if ((rc = wait_for_source(dst, src, dst->compose_src))) return rc;
	if (n_parts) HIP_TRY(hipMemcpyAsync(dst->compose.array + out_bytes, parts, part_bytes, hipMemcpyHostToDevice, dst->stream));
	HIP_TRY(hipMemcpyAsync(dst->compose.array + out_bytes + part_bytes, part_begin, begin_bytes, hipMemcpyHostToDevice, dst->stream));
	HIP_TRY(hipEventRecord(dst->compose_time.start, dst->stream));
	HIP_TRY(launch_compose(l, dst->stream));
	HIP_TRY(hipEventRecord(dst->compose_time.stop, dst->stream));
	if ((rc = finish_destinations(dst, dst_first, n_dst, dst->compose, dst->compose_time, out, out_bytes, gpu_ms))) return rc;
	for (uint32_t k = 0; copy_rules && k < n_dst; k++)
		if (part_begin[k + 1] > part_begin[k]) mark_rules(dst, dst_first + k, 1u); // a destination without parts keeps its rule
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_canon(ca3d_ensemble_t *e, uint32_t first, uint32_t count, ca3d_canon *out, uint64_t *digests, float *gpu_ms) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	if ((rc = require_state(e, first, count))) return rc;
	HIP_TRY(hipSetDevice(e->device));
	const size_t rec_bytes = (size_t)count * sizeof(ca3d_canon), dig_bytes = (size_t)count * 48u * sizeof(uint64_t), bytes = rec_bytes + dig_bytes;
	if ((rc = reserve(e, e->canon, bytes, &e->canon_time, nullptr, "%zu bytes of canon records", bytes))) return rc;
	CanonLaunch l{};
	l.state = e->state;
	l.first = first; l.count = count;
	l.out = e->canon.at<ca3d_canon>();
	l.digests = digests ? e->canon.at<uint64_t>(rec_bytes) : nullptr;
	HIP_TRY(hipEventRecord(e->canon_time.start, e->stream));
	HIP_TRY(launch_canon(l, e->stream));
	HIP_TRY(hipEventRecord(e->canon_time.stop, e->stream));
	HIP_TRY(hipMemcpyAsync(out, l.out, rec_bytes, hipMemcpyDeviceToHost, e->stream));
	if (digests) HIP_TRY(hipMemcpyAsync(digests, l.digests, dig_bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, e->canon_time.start, e->canon_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_canon_period(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *periods, ca3d_canon_period *out, uint64_t *keys,
                               uint32_t keys_stride, float *gpu_ms) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!periods) return fail(CA3D_ERR_INVALID_ARGUMENT, "periods is NULL");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	uint32_t longest = 0;
	for (uint32_t k = 0; k < count; k++)
	{
		if (periods[k] == 0 || periods[k] > CA3D_CANON_MAX_PERIOD)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "periods[%u] is %u: a period is 1 .. %u", k, periods[k], (unsigned)CA3D_CANON_MAX_PERIOD);
		if (periods[k] > longest) longest = periods[k];
	}
	if (keys && keys_stride < longest) return fail(CA3D_ERR_INVALID_ARGUMENT, "keys_stride is %u: less than the largest period, %u", keys_stride, longest);
	if (e->boundary != CA3D_ENSEMBLE_BOUNDARY_REFERENCE)
		return fail(CA3D_ERR_UNSUPPORTED, "this ensemble's boundary is %s: ca3d_ensemble_canon_period steps inside its own kernel with the reference boundary only "
		                                  "(ca3d_ensemble_set_boundary(e, CA3D_ENSEMBLE_BOUNDARY_REFERENCE), or step and ca3d_ensemble_canon phase by phase)",
		            e->boundary == CA3D_ENSEMBLE_BOUNDARY_TORUS ? "CA3D_ENSEMBLE_BOUNDARY_TORUS" : "CA3D_ENSEMBLE_BOUNDARY_CLOSED");
	if ((rc = require_state(e, first, count))) return rc;
	for (uint32_t u = first; u < first + count; u++)
		if (!e->has_rules[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_set_rules has not been called for universe %u", u);
	HIP_TRY(hipSetDevice(e->device));
	const size_t rec_bytes = (size_t)count * sizeof(ca3d_canon_period), key_bytes = keys ? (size_t)count * keys_stride * sizeof(uint64_t) : 0,
	             period_bytes = (size_t)count * sizeof(uint32_t);
	const size_t bytes = rec_bytes + key_bytes + period_bytes;
	if ((rc = reserve(e, e->canon, bytes, &e->canon_period_time, nullptr, "%zu bytes of canon records", bytes))) return rc;
	CanonPeriodLaunch l{};
	l.state = e->state;
	l.rules = e->rules;
	l.neighbourhood = e->neighbourhood;
	l.clustered = e->clustered;
	l.first = first; l.count = count;
	l.out = e->canon.at<ca3d_canon_period>();
	l.keys = keys ? e->canon.at<uint64_t>(rec_bytes) : nullptr;
	l.keys_stride = keys ? keys_stride : 0u;
	uint32_t *periods_dev = e->canon.at<uint32_t>(rec_bytes + key_bytes);
	l.periods = periods_dev;
	// (from pageable memory: the copy has left the caller's array when the call returns)
	HIP_TRY(hipMemcpyAsync(periods_dev, periods, period_bytes, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipEventRecord(e->canon_period_time.start, e->stream));
	HIP_TRY(launch_canon_period(l, e->stream));
	HIP_TRY(hipEventRecord(e->canon_period_time.stop, e->stream));
	HIP_TRY(hipMemcpyAsync(out, l.out, rec_bytes, hipMemcpyDeviceToHost, e->stream));
	if (keys) HIP_TRY(hipMemcpyAsync(keys, l.keys, key_bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, e->canon_period_time.start, e->canon_period_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_envelope(ca3d_ensemble_t *src, uint32_t first, uint32_t count, const uint32_t *periods, ca3d_ensemble_t *dst, uint32_t dst_first, uint32_t flags,
                           ca3d_envelope *out, float *gpu_ms) CA3D_API_TRY
{
	if (!src) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!periods) return fail(CA3D_ERR_INVALID_ARGUMENT, "periods is NULL");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	int rc = check_range(src, first, count);
	if (rc) return rc;
	for (uint32_t k = 0; k < count; k++)
		if (periods[k] == 0 || periods[k] > CA3D_CANON_MAX_PERIOD)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "periods[%u] is %u: a period is 1 .. %u", k, periods[k], (unsigned)CA3D_CANON_MAX_PERIOD);
	const uint32_t images = flags & (CA3D_ENVELOPE_IMAGE_ENVELOPE | CA3D_ENVELOPE_IMAGE_STATOR | CA3D_ENVELOPE_IMAGE_ROTOR);
	const bool copy_rules = (flags & CA3D_ENVELOPE_COPY_RULES) != 0u;
	if (flags & ~(images | CA3D_ENVELOPE_COPY_RULES)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in flags %#x", flags);
	if (images && !dst) return fail(CA3D_ERR_INVALID_ARGUMENT, "flags %#x ask for images, and dst is NULL", flags);
	if (!images && dst) return fail(CA3D_ERR_INVALID_ARGUMENT, "dst is given, and flags %#x ask for no image (CA3D_ENVELOPE_IMAGE_ENVELOPE = 1, _STATOR = 2, _ROTOR = 4)", flags);
	if (!images && copy_rules) return fail(CA3D_ERR_INVALID_ARGUMENT, "CA3D_ENVELOPE_COPY_RULES in flags %#x that ask for no image: there is no destination to copy a rule to", flags);
	// source k writes its images into destinations dst_first + k per + i (a count that does not fit a word is past every ensemble's end)
	const uint64_t wanted = (uint64_t)count * (uint32_t)__builtin_popcount(images);
	const uint32_t n_dst = wanted > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)wanted;
	if (dst)
	{
		if ((rc = check_destinations(dst, src, dst_first, n_dst, "images into"))) return rc;
		// the source range and the destinations are two intervals of the same ensemble: the first universe they share
		const uint32_t shared = first > dst_first ? first : dst_first;
		if (src == dst && shared - first < count && shared - dst_first < n_dst)
			return check_source(dst, src, dst_first, n_dst, "source", shared - first, shared, false);
		if ((rc = check_same_device_and_kind(dst, src, false, "CA3D_ENVELOPE_COPY_RULES"))) return rc; // the device
	}
	if ((rc = require_state(src, first, count))) return rc;
	for (uint32_t u = first; u < first + count; u++)
		if (!src->has_rules[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_set_rules has not been called for universe %u", u);
	if (dst && (rc = check_same_device_and_kind(dst, src, copy_rules, "CA3D_ENVELOPE_COPY_RULES"))) return rc; // the kind
	ca3d_ensemble *run = dst ? dst : src; // the handle whose stream takes the launch
	HIP_TRY(hipSetDevice(run->device));
	const size_t rec_bytes = (size_t)count * sizeof(ca3d_envelope), period_bytes = (size_t)count * sizeof(uint32_t), bytes = rec_bytes + period_bytes;
	if ((rc = reserve(run, run->envelope, bytes, &run->envelope_time, &run->envelope_src, "%zu bytes of envelope records", bytes))) return rc;
	EnvelopeLaunch l{};
	l.state = src->state;
	l.rules = src->rules;
	l.neighbourhood = src->neighbourhood;
	l.clustered = src->clustered;
	l.boundary = src->boundary;
	l.first = first; l.count = count;
	l.out = run->envelope.at<ca3d_envelope>();
	uint32_t *periods_dev = run->envelope.at<uint32_t>(rec_bytes);
	l.periods = periods_dev;
	l.images = images;
	if (dst)
	{
		l.dst_state = dst->state; l.dst_prev = dst->prev;
		l.dst_rules = dst->rules;
		l.dst_first = dst_first;
		l.rule_words = copy_rules ? rule_words(dst) : 0u;
	}
	if ((rc = wait_for_source(run, src, run->envelope_src))) return rc;
	// (from pageable memory: the copy has left the caller's array when the call returns)
	HIP_TRY(hipMemcpyAsync(periods_dev, periods, period_bytes, hipMemcpyHostToDevice, run->stream));
	HIP_TRY(hipEventRecord(run->envelope_time.start, run->stream));
	HIP_TRY(launch_envelope(l, run->stream));
	HIP_TRY(hipEventRecord(run->envelope_time.stop, run->stream));
	if (dst)
	{
		if ((rc = finish_destinations(dst, dst_first, n_dst, dst->envelope, dst->envelope_time, out, rec_bytes, gpu_ms))) return rc;
		if (copy_rules) mark_rules(dst, dst_first, n_dst);
		return CA3D_OK;
	}
	HIP_TRY(hipMemcpyAsync(out, l.out, rec_bytes, hipMemcpyDeviceToHost, src->stream));
	HIP_TRY(hipStreamSynchronize(src->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, src->envelope_time.start, src->envelope_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_damage(ca3d_ensemble_t *src, uint32_t first, uint32_t count, const uint32_t *steps, const uint32_t *twins, const uint32_t *flips, ca3d_ensemble_t *dst,
                         uint32_t dst_first, uint32_t flags, ca3d_damage *out, uint32_t *curve, uint32_t curve_stride, float *gpu_ms) CA3D_API_TRY
{
	if (!src) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!steps) return fail(CA3D_ERR_INVALID_ARGUMENT, "steps is NULL");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	int rc = check_range(src, first, count);
	if (rc) return rc;
	uint32_t longest = 0;
	for (uint32_t k = 0; k < count; k++)
	{
		if (steps[k] == 0 || steps[k] > CA3D_CANON_MAX_PERIOD)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "steps[%u] is %u (universe %u): a step count is 1 .. %u", k, steps[k], first + k, (unsigned)CA3D_CANON_MAX_PERIOD);
		if (steps[k] > longest) longest = steps[k];
	}
	for (uint32_t k = 0; twins && k < count; k++)
		if (twins[k] != CA3D_DAMAGE_SELF && twins[k] >= src->n)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "twins[%u] is %u (universe %u): a twin is CA3D_DAMAGE_SELF or one of the ensemble's %u universes", k, twins[k], first + k, src->n);
	for (uint32_t k = 0; flips && k < count; k++)
		for (uint32_t i = 0; i < CA3D_DAMAGE_FLIPS; i++)
		{
			const uint32_t f = flips[k * CA3D_DAMAGE_FLIPS + i];
			if (f != CA3D_DAMAGE_NO_FLIP && ((f & 0xFFu) >= 64u || ((f >> 8) & 0xFFu) >= 64u || ((f >> 16) & 0xFFu) >= 64u || f >> 24))
				return fail(CA3D_ERR_INVALID_ARGUMENT, "flips[%u][%u] is %#x (universe %u): a flip is x | y << 8 | z << 16 with x, y, z below 64, or CA3D_DAMAGE_NO_FLIP", k, i, f,
				            first + k);
		}
	if (curve && curve_stride < longest + 1u)
		return fail(CA3D_ERR_INVALID_ARGUMENT, "curve_stride is %u: a curve of %u steps holds %u samples", curve_stride, longest, longest + 1u);
	const uint32_t image = flags & CA3D_DAMAGE_IMAGE_DAMAGE;
	const bool copy_rules = (flags & CA3D_DAMAGE_COPY_RULES) != 0u;
	if (flags & ~(CA3D_DAMAGE_IMAGE_DAMAGE | CA3D_DAMAGE_COPY_RULES)) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown bits in flags %#x", flags);
	if (image && !dst) return fail(CA3D_ERR_INVALID_ARGUMENT, "flags %#x ask for the image, and dst is NULL", flags);
	if (!image && dst) return fail(CA3D_ERR_INVALID_ARGUMENT, "dst is given, and flags %#x ask for no image (CA3D_DAMAGE_IMAGE_DAMAGE = 1)", flags);
	if (!image && copy_rules) return fail(CA3D_ERR_INVALID_ARGUMENT, "CA3D_DAMAGE_COPY_RULES in flags %#x that ask for no image: there is no destination to copy a rule to", flags);
	if (dst)
	{
		if ((rc = check_destinations(dst, src, dst_first, count, "images into"))) return rc;
		// the source range and the destinations are two intervals of the same ensemble: the first universe they share
		const uint32_t shared = first > dst_first ? first : dst_first;
		if (src == dst && shared - first < count && shared - dst_first < count)
			return check_source(dst, src, dst_first, count, "source", shared - first, shared, false);
		for (uint32_t k = 0; src == dst && twins && k < count; k++)
			if (twins[k] != CA3D_DAMAGE_SELF && twins[k] >= dst_first && twins[k] - dst_first < count) return check_source(dst, src, dst_first, count, "twin", k, twins[k], false);
		if ((rc = check_same_device_and_kind(dst, src, false, "CA3D_DAMAGE_COPY_RULES"))) return rc; // the device
	}
	if ((rc = require_state(src, first, count))) return rc;
	for (uint32_t k = 0; twins && k < count; k++)
		if (twins[k] != CA3D_DAMAGE_SELF && !src->has_state[twins[k]])
			return fail(CA3D_ERR_NOT_CONFIGURED, "twins[%u]: ca3d_ensemble_upload_state has not been called for universe %u", k, twins[k]);
	for (uint32_t u = first; u < first + count; u++)
		if (!src->has_rules[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_set_rules has not been called for universe %u", u);
	if (dst && (rc = check_same_device_and_kind(dst, src, copy_rules, "CA3D_DAMAGE_COPY_RULES"))) return rc; // the kind
	ca3d_ensemble *run = dst ? dst : src; // the handle whose stream takes the launch
	HIP_TRY(hipSetDevice(run->device));
	constexpr uint32_t kItemWords = 2u + CA3D_DAMAGE_FLIPS; // a universe's step count, twin and flips
	const size_t rec_bytes = (size_t)count * sizeof(ca3d_damage), item_bytes = (size_t)count * kItemWords * sizeof(uint32_t);
	const size_t curve_bytes = curve ? (size_t)count * curve_stride * sizeof(uint32_t) : 0, bytes = rec_bytes + item_bytes + curve_bytes;
	if ((rc = reserve(run, run->damage, bytes, &run->damage_time, &run->damage_src, "%zu bytes of damage records", bytes))) return rc;
	// steps, twins and flips as the kernel reads them, every default written out
	std::vector<uint32_t> items((size_t)count * kItemWords, 0xFFFFFFFFu); // CA3D_DAMAGE_SELF, CA3D_DAMAGE_NO_FLIP
	memcpy(items.data(), steps, (size_t)count * sizeof(uint32_t));
	if (twins) memcpy(items.data() + count, twins, (size_t)count * sizeof(uint32_t));
	if (flips) memcpy(items.data() + 2u * (size_t)count, flips, (size_t)count * CA3D_DAMAGE_FLIPS * sizeof(uint32_t));
	DamageLaunch l{};
	l.state = src->state;
	l.rules = src->rules;
	l.neighbourhood = src->neighbourhood;
	l.clustered = src->clustered;
	l.boundary = src->boundary;
	l.first = first; l.count = count;
	l.out = run->damage.at<ca3d_damage>();
	uint32_t *items_dev = run->damage.at<uint32_t>(rec_bytes);
	l.steps = items_dev;
	l.twins = items_dev + count;
	l.flips = items_dev + 2u * (size_t)count;
	l.curve = curve ? run->damage.at<uint32_t>(rec_bytes + item_bytes) : nullptr;
	l.curve_stride = curve_stride;
	l.image = image;
	if (dst)
	{
		l.dst_state = dst->state; l.dst_prev = dst->prev;
		l.dst_rules = dst->rules;
		l.dst_first = dst_first;
		l.rule_words = copy_rules ? rule_words(dst) : 0u;
	}
	if ((rc = wait_for_source(run, src, run->damage_src))) return rc;
	// (from pageable memory: the copy has left `items` when the call returns)
	HIP_TRY(hipMemcpyAsync(items_dev, items.data(), item_bytes, hipMemcpyHostToDevice, run->stream));
	HIP_TRY(hipEventRecord(run->damage_time.start, run->stream));
	HIP_TRY(launch_damage(l, run->stream));
	HIP_TRY(hipEventRecord(run->damage_time.stop, run->stream));
	if (curve) HIP_TRY(hipMemcpyAsync(curve, l.curve, curve_bytes, hipMemcpyDeviceToHost, run->stream));
	if (dst)
	{
		if ((rc = finish_destinations(dst, dst_first, count, dst->damage, dst->damage_time, out, rec_bytes, gpu_ms))) return rc;
		if (copy_rules) mark_rules(dst, dst_first, count);
		return CA3D_OK;
	}
	HIP_TRY(hipMemcpyAsync(out, l.out, rec_bytes, hipMemcpyDeviceToHost, src->stream));
	HIP_TRY(hipStreamSynchronize(src->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, src->damage_time.start, src->damage_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_ensemble_usage(ca3d_ensemble_t *e, uint32_t first, uint32_t count, const uint32_t *steps, ca3d_usage *out, float *gpu_ms) CA3D_API_TRY
{
	if (!e) return fail(CA3D_ERR_INVALID_ARGUMENT, "NULL ensemble handle");
	if (!steps) return fail(CA3D_ERR_INVALID_ARGUMENT, "steps is NULL");
	if (!out) return fail(CA3D_ERR_INVALID_ARGUMENT, "out is NULL");
	int rc = check_range(e, first, count);
	if (rc) return rc;
	for (uint32_t k = 0; k < count; k++)
		if (steps[k] == 0 || steps[k] > CA3D_CANON_MAX_PERIOD)
			return fail(CA3D_ERR_INVALID_ARGUMENT, "steps[%u] is %u (universe %u): a step count is 1 .. %u", k, steps[k], first + k, (unsigned)CA3D_CANON_MAX_PERIOD);
	if ((rc = require_state(e, first, count))) return rc;
	for (uint32_t u = first; u < first + count; u++)
		if (!e->has_rules[u]) return fail(CA3D_ERR_NOT_CONFIGURED, "ca3d_ensemble_set_rules has not been called for universe %u", u);
	HIP_TRY(hipSetDevice(e->device));
	const size_t rec_bytes = (size_t)count * sizeof(ca3d_usage), step_bytes = (size_t)count * sizeof(uint32_t), bytes = rec_bytes + step_bytes;
	if ((rc = reserve(e, e->usage, bytes, &e->usage_time, nullptr, "%zu bytes of usage records", bytes))) return rc;
	UsageLaunch l{};
	l.state = e->state;
	l.rules = e->rules;
	l.neighbourhood = e->neighbourhood;
	l.clustered = e->clustered;
	l.boundary = e->boundary;
	l.first = first; l.count = count;
	l.out = e->usage.at<ca3d_usage>();
	uint32_t *steps_dev = e->usage.at<uint32_t>(rec_bytes);
	l.steps = steps_dev;
	// (from pageable memory: the copy has left the caller's array when the call returns)
	HIP_TRY(hipMemcpyAsync(steps_dev, steps, step_bytes, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipEventRecord(e->usage_time.start, e->stream));
	HIP_TRY(launch_usage(l, e->stream));
	HIP_TRY(hipEventRecord(e->usage_time.stop, e->stream));
	HIP_TRY(hipMemcpyAsync(out, l.out, rec_bytes, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, e->usage_time.start, e->usage_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_cut_windows(ca3d_t *src, ca3d_ensemble_t *dst, uint32_t n, const ca3d_window *w, float *gpu_ms) CA3D_API_TRY
{
	int rc = check_windows(src, dst, n, w, true);
	if (rc) return rc;
	if ((rc = settle_engine(src))) return rc;
	if ((rc = reserve(dst, dst->windows, (size_t)n * sizeof(ca3d_window), &dst->windows_time, &dst->windows_src, "%u windows", n))) return rc;
	if ((rc = stage_windows(dst, n, w, dst->stream, src->stream))) return rc;
	WindowLaunch l{};
	l.grid = src->buf[src->cur];
	l.G = src->G;
	l.state = dst->state; l.prev = dst->prev;
	l.windows = dst->windows.at<const ca3d_window>();
	l.n = n;
	l.op = kWindowCut;
	HIP_TRY(hipEventRecord(dst->windows_time.start, dst->stream));
	HIP_TRY(launch_windows(l, dst->stream));
	HIP_TRY(hipEventRecord(dst->windows_time.stop, dst->stream));
	// the records of the universes written, one launch for every run of consecutive ones (a tiling names one run)
	std::vector<uint32_t> written(n);
	for (uint32_t k = 0; k < n; k++) written[k] = w[k].universe;
	std::sort(written.begin(), written.end());
	for (uint32_t k = 0, run = 0; k < n; k = run)
	{
		for (run = k + 1u; run < n && written[run] == written[run - 1u] + 1u; run++) {}
		if ((rc = reset_records(dst, written[k], run - k))) return rc;
	}
	HIP_TRY(hipStreamSynchronize(dst->stream)); // the caller's windows are consumed, and the engine may go on
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, dst->windows_time.start, dst->windows_time.stop));
	for (uint32_t u : written) mark_state(dst, u, 1u);
	return CA3D_OK;
}
CA3D_API_CATCH

int ca3d_stamp_windows(ca3d_t *dst, ca3d_ensemble_t *src, uint32_t n, const ca3d_window *w, uint32_t mode, float *gpu_ms) CA3D_API_TRY
{
	if (mode > CA3D_STAMP_ERASE) return fail(CA3D_ERR_INVALID_ARGUMENT, "unknown mode %u (CA3D_STAMP_OR = 0, CA3D_STAMP_REPLACE = 1, CA3D_STAMP_ERASE = 2)", mode);
	int rc = check_windows(dst, src, n, w, false);
	if (rc) return rc;
	if ((rc = settle_engine(dst))) return rc;
	if ((rc = reserve(src, src->windows, (size_t)n * sizeof(ca3d_window), &src->windows_time, &src->windows_src, "%u windows", n))) return rc;
	if (!dst->has_state && (rc = engine_mark_state(dst))) return rc; // a world built from objects alone: all dead, step 0
	if ((rc = stage_windows(src, n, w, dst->stream, src->stream))) return rc;
	WindowLaunch l{};
	l.grid = dst->buf[dst->cur];
	l.G = dst->G;
	l.state = src->state;
	l.windows = src->windows.at<const ca3d_window>();
	l.n = n;
	HIP_TRY(hipEventRecord(src->windows_time.start, dst->stream));
	if (mode == CA3D_STAMP_REPLACE)
	{
		l.op = kWindowClear; // every box first: a window's cells must not outlive another window's clear
		HIP_TRY(launch_windows(l, dst->stream));
	}
	l.op = mode == CA3D_STAMP_ERASE ? kWindowErase : kWindowOr;
	HIP_TRY(launch_windows(l, dst->stream));
	HIP_TRY(hipEventRecord(src->windows_time.stop, dst->stream));
	engine_state_edited(dst);
	HIP_TRY(hipStreamSynchronize(dst->stream)); // the caller's windows are consumed, and the ensemble may go on
	if (gpu_ms) HIP_TRY(hipEventElapsedTime(gpu_ms, src->windows_time.start, src->windows_time.stop));
	return CA3D_OK;
}
CA3D_API_CATCH

} // extern "C"
