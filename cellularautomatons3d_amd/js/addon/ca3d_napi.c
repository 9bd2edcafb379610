/*
 * N-API addon: the JavaScript face of include/ca3d.h, 1:1, typed arrays in and out. This is the binding a
 * maintainer of main_pathtraced.js adds in place of the navigator.gpu calls. No logic lives
 * here: every function forwards to libca3d.so and throws a JS Error carrying ca3d_last_error() on failure.
 *
 * Built with plain gcc against /usr/include/node (N-API 8 headers; Node >= 12).
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ca3d.h"

#define NAPI_OK_OR_NULL(call)                                  \
	do {                                                       \
		if ((call) != napi_ok) {                               \
			napi_throw_error(env, NULL, "N-API call failed: " #call); \
			return NULL;                                       \
		}                                                      \
	} while (0)

static napi_value throw_ca3d(napi_env env, int rc)
{
	char msg[600];
	snprintf(msg, sizeof msg, "ca3d error %d: %s", rc, ca3d_last_error());
	napi_throw_error(env, NULL, msg);
	return NULL;
}

static napi_value undefined(napi_env env)
{
	napi_value u;
	napi_get_undefined(env, &u);
	return u;
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv)
{
	size_t argc = want;
	if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want)
	{
		napi_throw_type_error(env, NULL, "wrong number of arguments");
		return 0;
	}
	return 1;
}

/* What a handle external points at: the engine and the number of asynchronous jobs that still use it (main thread only). */
typedef struct
{
	ca3d_t *h; /* first member: a Slot * reads as a ca3d_t ** */
	int pending;
} Slot;

static ca3d_t *get_handle(napi_env env, napi_value v)
{
	void *p = NULL;
	if (napi_get_value_external(env, v, &p) != napi_ok || !p)
	{
		napi_throw_type_error(env, NULL, "expected an engine handle");
		return NULL;
	}
	return *(ca3d_t **)p;
}

static int get_u32(napi_env env, napi_value v, uint32_t *out)
{
	if (napi_get_value_uint32(env, v, out) != napi_ok)
	{
		napi_throw_type_error(env, NULL, "expected an unsigned integer");
		return 0;
	}
	return 1;
}

/* typed array of the given element type, or null/undefined when `nullable` */
static int get_typed(napi_env env, napi_value v, napi_typedarray_type want, int nullable, void **data, size_t *len)
{
	napi_valuetype t;
	napi_typeof(env, v, &t);
	if (nullable && (t == napi_null || t == napi_undefined))
	{
		*data = NULL;
		*len = 0;
		return 1;
	}
	bool is = false;
	napi_is_typedarray(env, v, &is);
	napi_typedarray_type type;
	napi_value ab;
	size_t off;
	if (!is || napi_get_typedarray_info(env, v, &type, len, data, &ab, &off) != napi_ok || type != want)
	{
		napi_throw_type_error(env, NULL, "expected a typed array of the documented element type");
		return 0;
	}
	return 1;
}

static void finalize_handle(napi_env env, void *data, void *hint)
{
	(void)env;
	(void)hint;
	Slot *slot = (Slot *)data; /* no job is pending: every job holds a reference to the external */
	if (slot->h) ca3d_destroy(slot->h);
	slot->h = NULL;
	free(slot);
}

static napi_value js_create(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	int32_t device = 0;
	napi_get_value_int32(env, argv[0], &device);
	ca3d_t *h = NULL;
	int rc = ca3d_create(device, &h);
	if (rc) return throw_ca3d(env, rc);
	Slot *slot = (Slot *)calloc(1, sizeof *slot);
	if (!slot) { ca3d_destroy(h); napi_throw_error(env, NULL, "out of memory"); return NULL; }
	slot->h = h;
	napi_value ext;
	NAPI_OK_OR_NULL(napi_create_external(env, slot, finalize_handle, NULL, &ext));
	return ext;
}

static napi_value js_destroy(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	void *p = NULL;
	if (napi_get_value_external(env, argv[0], &p) == napi_ok && p)
	{
		Slot *slot = (Slot *)p;
		if (slot->pending)
		{
			/* a libuv worker is inside ca3d_read_state / ca3d_render / ca3d_synchronize on this engine */
			napi_throw_error(env, NULL, "the engine has asynchronous work pending: await it before close()");
			return NULL;
		}
		if (slot->h) ca3d_destroy(slot->h);
		slot->h = NULL;
	}
	return undefined(env);
}

static napi_value js_device_count(napi_env env, napi_callback_info info)
{
	(void)info;
	int n = 0;
	int rc = ca3d_device_count(&n);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_int32(env, n, &v);
	return v;
}

static napi_value js_configure(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t g, layout;
	if (!h || !get_u32(env, argv[1], &g) || !get_u32(env, argv[2], &layout)) return NULL;
	int rc = ca3d_configure(h, g, g, g, (int)layout);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_configure_slab(napi_env env, napi_callback_info info)
{
	napi_value argv[6];
	if (!get_args(env, info, 6, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t g, layout, z0, nz, ghost;
	if (!h || !get_u32(env, argv[1], &g) || !get_u32(env, argv[2], &layout) || !get_u32(env, argv[3], &z0) ||
	    !get_u32(env, argv[4], &nz) || !get_u32(env, argv[5], &ghost))
		return NULL;
	int rc = ca3d_configure_slab(h, g, (int)layout, z0, nz, ghost);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_set_rules(napi_env env, napi_callback_info info)
{
	napi_value argv[6];
	if (!get_args(env, info, 6, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	void *m, *e, *c, *s, *b;
	size_t nm, ne, nc, ns, nb;
	if (!get_typed(env, argv[1], napi_int32_array, 0, &m, &nm) || !get_typed(env, argv[2], napi_int32_array, 0, &e, &ne) ||
	    !get_typed(env, argv[3], napi_int32_array, 0, &c, &nc) || !get_typed(env, argv[4], napi_uint32_array, 0, &s, &ns) ||
	    !get_typed(env, argv[5], napi_uint32_array, 0, &b, &nb))
		return NULL;
	if (ns != CA3D_LUT_LEN || nb != CA3D_LUT_LEN)
	{
		napi_throw_range_error(env, NULL, "survive/born must be Uint32Array(81)");
		return NULL;
	}
	int rc = ca3d_set_rules(h, (const int32_t *)m, (uint32_t)nm, (const int32_t *)e, (uint32_t)ne, (const int32_t *)c,
	                        (uint32_t)nc, (const uint32_t *)s, (const uint32_t *)b);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_upload_state(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	void *w;
	size_t n;
	if (!h || !get_typed(env, argv[1], napi_uint32_array, 0, &w, &n)) return NULL;
	int rc = ca3d_upload_state(h, (const uint32_t *)w, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_read_state(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	void *w;
	size_t n;
	if (!h || !get_typed(env, argv[1], napi_uint32_array, 0, &w, &n)) return NULL;
	int rc = ca3d_read_state(h, (uint32_t *)w, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_step(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t n;
	if (!h || !get_u32(env, argv[1], &n)) return NULL;
	int rc = ca3d_step(h, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_flush(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	int rc = ca3d_flush(h);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_slab_step(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t n;
	if (!h || !get_u32(env, argv[1], &n)) return NULL;
	int rc = ca3d_slab_step(h, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_slab_step_phase(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t n, phase;
	if (!h || !get_u32(env, argv[1], &n) || !get_u32(env, argv[2], &phase)) return NULL;
	int rc = ca3d_slab_step_phase(h, n, (int)phase);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_synchronize(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	int rc = ca3d_synchronize(h);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static void set_num(napi_env env, napi_value obj, const char *k, double v)
{
	napi_value n;
	napi_create_double(env, v, &n);
	napi_set_named_property(env, obj, k, n);
}

static napi_value js_info(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	ca3d_info i;
	int rc = ca3d_get_info(h, &i);
	if (rc) return throw_ca3d(env, rc);
	napi_value o, s;
	napi_create_object(env, &o);
	set_num(env, o, "gridSize", i.grid_size);
	set_num(env, o, "layout", i.layout);
	set_num(env, o, "z0", i.z0);
	set_num(env, o, "nz", i.nz);
	set_num(env, o, "ghost", i.ghost);
	set_num(env, o, "step", (double)i.step);
	set_num(env, o, "stateWords", (double)i.state_words);
	set_num(env, o, "currentBuffer", i.current_buffer);
	set_num(env, o, "device", i.device);
	set_num(env, o, "launchesTotal", (double)i.launches_total);
	napi_create_string_utf8(env, i.kernel_name, NAPI_AUTO_LENGTH, &s);
	napi_set_named_property(env, o, "kernelName", s);
	char variant[384];
	if (ca3d_get_kernel_variant(h, variant, sizeof variant, NULL) == CA3D_OK)
	{
		napi_create_string_utf8(env, variant, NAPI_AUTO_LENGTH, &s);
		napi_set_named_property(env, o, "kernelVariant", s);
	}
	return o;
}

static napi_value js_stats(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	ca3d_stats st;
	int rc = ca3d_get_stats(h, &st);
	if (rc) return throw_ca3d(env, rc);
	napi_value o;
	napi_create_object(env, &o);
	set_num(env, o, "steps", (double)st.steps);
	set_num(env, o, "kernelLaunches", (double)st.kernel_launches);
	set_num(env, o, "gpuMs", st.gpu_ms);
	set_num(env, o, "cellSteps", st.cell_steps);
	set_num(env, o, "algorithmicBytes", st.algorithmic_bytes);
	return o;
}

static napi_value js_render(napi_env env, napi_callback_info info)
{
	napi_value argv[8];
	if (!get_args(env, info, 8, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	void *u, *pres, *light, *depth;
	size_t nu, npres, nlight, ndepth;
	uint32_t w, hh, spp;
	if (!get_typed(env, argv[1], napi_float32_array, 0, &u, &nu) || !get_u32(env, argv[2], &w) || !get_u32(env, argv[3], &hh) ||
	    !get_u32(env, argv[4], &spp) || !get_typed(env, argv[5], napi_uint8_array, 1, &pres, &npres) ||
	    !get_typed(env, argv[6], napi_uint16_array, 1, &light, &nlight) || !get_typed(env, argv[7], napi_uint16_array, 1, &depth, &ndepth))
		return NULL;
	const size_t px = (size_t)w * hh;
	if (nu != 128 || (pres && npres != px * 4) || (light && nlight != px * 4) || (depth && ndepth != px * 2))
	{
		napi_throw_range_error(env, NULL, "uniforms must be Float32Array(128); targets must match width*height");
		return NULL;
	}
	int rc = ca3d_render(h, (const float *)u, w, hh, spp, (uint8_t *)pres, (uint16_t *)light, (uint16_t *)depth);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_render_stats(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	ca3d_render_stats st;
	int rc = ca3d_get_render_stats(h, &st);
	if (rc) return throw_ca3d(env, rc);
	napi_value o;
	napi_create_object(env, &o);
	set_num(env, o, "gpuMs", st.gpu_ms);
	set_num(env, o, "primaryRays", (double)st.primary_rays);
	set_num(env, o, "shadowRays", (double)st.shadow_rays);
	set_num(env, o, "primaryCellVisits", (double)st.primary_cell_visits);
	set_num(env, o, "shadowCellVisits", (double)st.shadow_cell_visits);
	return o;
}

static napi_value js_render_pipeline(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	int32_t n = 0;
	int rc = ca3d_get_render_pipeline(h, &n);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_int32(env, n, &v);
	return v;
}

static napi_value js_set_option(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	char name[64];
	size_t len = 0;
	int64_t v = 0;
	napi_get_value_string_utf8(env, argv[1], name, sizeof name, &len);
	napi_get_value_int64(env, argv[2], &v);
	int rc = ca3d_set_option(h, name, v);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* RCCL transport inside the engine (include/ca3d.h "Halo transport"): a Node.js host runs one process per GPU, creates the
 * id on rank 0, hands the 128 bytes to the other ranks over its own IPC, and calls slabRun — no Python involved. */
static napi_value js_comm_unique_id(napi_env env, napi_callback_info info)
{
	(void)info;
	void *data = NULL;
	napi_value ab, out;
	NAPI_OK_OR_NULL(napi_create_arraybuffer(env, CA3D_COMM_ID_BYTES, &data, &ab));
	int rc = ca3d_comm_unique_id(data);
	if (rc) return throw_ca3d(env, rc);
	NAPI_OK_OR_NULL(napi_create_typedarray(env, napi_uint8_array, CA3D_COMM_ID_BYTES, ab, 0, &out));
	return out;
}

static napi_value js_slab_comm_init(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	void *id;
	size_t n;
	uint32_t rank, world;
	if (!h || !get_typed(env, argv[1], napi_uint8_array, 0, &id, &n) || !get_u32(env, argv[2], &rank) || !get_u32(env, argv[3], &world)) return NULL;
	if (n != CA3D_COMM_ID_BYTES) { napi_throw_range_error(env, NULL, "the communicator id is a Uint8Array(128)"); return NULL; }
	int rc = ca3d_slab_comm_init(h, id, (int)rank, (int)world);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_slab_run(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t n, overlap;
	if (!h || !get_u32(env, argv[1], &n) || !get_u32(env, argv[2], &overlap)) return NULL;
	int rc = ca3d_slab_run(h, n, (int)overlap);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_slab_exchange(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	int rc = ca3d_slab_exchange(h);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_slab_gather(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]), *full = get_handle(env, argv[1]);
	if (!h || !full) return NULL;
	int rc = ca3d_slab_gather(h, full);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ca3d_summary as a JS object. uint64 fields: `digest` uses all 64 bits and crosses as a BigInt; step, population, births and
 * deaths stay below 2^53 on every grid the engine accepts (8192^3 = 2^39 cells) and cross as Numbers. */
static napi_value summary_object(napi_env env, const ca3d_summary *s, napi_value planes)
{
	napi_value o, v, lo, hi;
	napi_create_object(env, &o);
	set_num(env, o, "step", (double)s->step);
	set_num(env, o, "population", (double)s->population);
	set_num(env, o, "births", (double)s->births);
	set_num(env, o, "deaths", (double)s->deaths);
	napi_create_bigint_uint64(env, s->digest, &v);
	napi_set_named_property(env, o, "digest", v);
	napi_get_boolean(env, s->has_previous != 0, &v);
	napi_set_named_property(env, o, "hasPrevious", v);
	napi_create_array_with_length(env, 3, &lo);
	napi_create_array_with_length(env, 3, &hi);
	for (uint32_t i = 0; i < 3; i++)
	{
		napi_create_uint32(env, s->box_min[i], &v);
		napi_set_element(env, lo, i, v);
		napi_create_uint32(env, s->box_max[i], &v);
		napi_set_element(env, hi, i, v);
	}
	napi_set_named_property(env, o, "boxMin", lo);
	napi_set_named_property(env, o, "boxMax", hi);
	if (planes) napi_set_named_property(env, o, "planePopulation", planes);
	return o;
}

/* summary(handle, Uint32Array(nz) | null) */
static napi_value js_summary(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	void *pp;
	size_t n;
	if (!h || !get_typed(env, argv[1], napi_uint32_array, 1, &pp, &n)) return NULL;
	ca3d_info i;
	int rc = ca3d_get_info(h, &i);
	if (rc) return throw_ca3d(env, rc);
	if (pp && n != i.nz)
	{
		napi_throw_range_error(env, NULL, "planePopulation must hold one entry per owned plane (info().nz)");
		return NULL;
	}
	ca3d_summary s;
	rc = ca3d_summarize(h, &s, (uint32_t *)pp);
	if (rc) return throw_ca3d(env, rc);
	return summary_object(env, &s, pp ? argv[1] : NULL);
}

/*
 * Asynchronous forms of the calls that wait for the GPU ("optional napi_async_work wrappers"): the wait
 * runs on a libuv worker thread and the call returns a Promise, so a UI thread never blocks in a read-back. The engine
 * is not thread-safe: the JS wrapper (ca3d.js) queues everything else behind a pending job of the same engine.
 */
typedef struct
{
	napi_async_work work;
	napi_deferred deferred;
	ca3d_t *h;
	int kind; /* 0 readState, 1 render, 2 synchronize, 3 stepUntil, 4 stepUntilCycle */
	uint32_t max_steps, check_every, stop_mask, steps_done, reason, period;
	ca3d_summary summary;
	int rc;
	char err[512];
	uint32_t *words;
	size_t n_words;
	float uniforms[128];
	uint32_t w, hh, spp;
	uint8_t *pres;
	uint16_t *light, *depth;
	napi_ref refs[4]; /* the handle external and the typed arrays stay alive (and in place) until the job completes */
	int nrefs;
	Slot *slot;       /* its `pending` count keeps destroy() away while the worker runs */
} AsyncJob;

static void job_execute(napi_env env, void *data)
{
	(void)env;
	AsyncJob *j = (AsyncJob *)data;
	if (j->kind == 0) j->rc = ca3d_read_state(j->h, j->words, j->n_words);
	else if (j->kind == 1) j->rc = ca3d_render(j->h, j->uniforms, j->w, j->hh, j->spp, j->pres, j->light, j->depth);
	else if (j->kind == 3) j->rc = ca3d_step_until(j->h, j->max_steps, j->check_every, j->stop_mask, &j->summary, &j->steps_done, &j->reason);
	else if (j->kind == 4)
		j->rc = ca3d_step_until_cycle(j->h, j->max_steps, j->check_every, j->stop_mask, &j->summary, &j->steps_done, &j->reason, &j->period);
	else j->rc = ca3d_synchronize(j->h);
	if (j->rc) snprintf(j->err, sizeof j->err, "ca3d error %d: %s", j->rc, ca3d_last_error()); /* ca3d_last_error is per thread */
}

static void job_complete(napi_env env, napi_status status, void *data)
{
	AsyncJob *j = (AsyncJob *)data;
	napi_value v;
	if (status == napi_ok && j->rc == 0)
	{
		if (j->kind == 3 || j->kind == 4)
		{
			napi_create_object(env, &v);
			set_num(env, v, "stepsDone", j->steps_done);
			set_num(env, v, "reason", j->reason);
			if (j->kind == 4) set_num(env, v, "period", j->period);
			napi_set_named_property(env, v, "summary", summary_object(env, &j->summary, NULL));
		}
		else napi_get_undefined(env, &v);
		napi_resolve_deferred(env, j->deferred, v);
	}
	else
	{
		napi_value msg;
		napi_create_string_utf8(env, status == napi_ok ? j->err : "the asynchronous job was cancelled", NAPI_AUTO_LENGTH, &msg);
		napi_create_error(env, NULL, msg, &v);
		napi_reject_deferred(env, j->deferred, v);
	}
	if (j->slot) j->slot->pending--;
	for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
	napi_delete_async_work(env, j->work);
	free(j);
}

static napi_value job_start(napi_env env, AsyncJob *j, const char *name)
{
	napi_value promise, resource;
	if (napi_create_promise(env, &j->deferred, &promise) != napi_ok || napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &resource) != napi_ok ||
	    napi_create_async_work(env, NULL, resource, job_execute, job_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok)
	{
		for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
		free(j);
		napi_throw_error(env, NULL, "could not queue the asynchronous job");
		return NULL;
	}
	if (j->slot) j->slot->pending++;
	return promise;
}

static void job_keep(napi_env env, AsyncJob *j, napi_value v)
{
	napi_valuetype t;
	napi_typeof(env, v, &t);
	if (t == napi_null || t == napi_undefined) return;
	if (j->nrefs < (int)(sizeof j->refs / sizeof j->refs[0]) && napi_create_reference(env, v, 1, &j->refs[j->nrefs]) == napi_ok) j->nrefs++;
}

/* The job keeps the handle external alive (its finalizer destroys the engine) and counts itself on the slot. */
static void job_hold_engine(napi_env env, AsyncJob *j, napi_value handle)
{
	void *p = NULL;
	if (napi_get_value_external(env, handle, &p) == napi_ok) j->slot = (Slot *)p;
	job_keep(env, j, handle);
}

static napi_value js_read_state_async(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	void *w;
	size_t n;
	if (!h || !get_typed(env, argv[1], napi_uint32_array, 0, &w, &n)) return NULL;
	AsyncJob *j = (AsyncJob *)calloc(1, sizeof *j);
	if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
	j->h = h; j->kind = 0; j->words = (uint32_t *)w; j->n_words = n;
	job_hold_engine(env, j, argv[0]);
	job_keep(env, j, argv[1]);
	return job_start(env, j, "ca3d.readState");
}

static napi_value js_render_async(napi_env env, napi_callback_info info)
{
	napi_value argv[8];
	if (!get_args(env, info, 8, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	void *u, *pres, *light, *depth;
	size_t nu, npres, nlight, ndepth;
	uint32_t w, hh, spp;
	if (!get_typed(env, argv[1], napi_float32_array, 0, &u, &nu) || !get_u32(env, argv[2], &w) || !get_u32(env, argv[3], &hh) ||
	    !get_u32(env, argv[4], &spp) || !get_typed(env, argv[5], napi_uint8_array, 1, &pres, &npres) ||
	    !get_typed(env, argv[6], napi_uint16_array, 1, &light, &nlight) || !get_typed(env, argv[7], napi_uint16_array, 1, &depth, &ndepth))
		return NULL;
	const size_t px = (size_t)w * hh;
	if (nu != 128 || (pres && npres != px * 4) || (light && nlight != px * 4) || (depth && ndepth != px * 2))
	{
		napi_throw_range_error(env, NULL, "uniforms must be Float32Array(128); targets must match width*height");
		return NULL;
	}
	AsyncJob *j = (AsyncJob *)calloc(1, sizeof *j);
	if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
	j->h = h; j->kind = 1; j->w = w; j->hh = hh; j->spp = spp;
	memcpy(j->uniforms, u, sizeof j->uniforms); /* the block is consumed now, like the reference's writeBuffer */
	j->pres = (uint8_t *)pres; j->light = (uint16_t *)light; j->depth = (uint16_t *)depth;
	job_hold_engine(env, j, argv[0]);
	job_keep(env, j, argv[5]); job_keep(env, j, argv[6]); job_keep(env, j, argv[7]);
	return job_start(env, j, "ca3d.render");
}

static napi_value js_synchronize_async(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	AsyncJob *j = (AsyncJob *)calloc(1, sizeof *j);
	if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
	j->h = h; j->kind = 2;
	job_hold_engine(env, j, argv[0]);
	return job_start(env, j, "ca3d.synchronize");
}

/* stepUntilAsync(handle, maxSteps, checkEvery, stopMask) -> Promise<{stepsDone, reason, summary}>: many batches and a wait each */
static napi_value js_step_until_async(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t max_steps, every, mask;
	if (!h || !get_u32(env, argv[1], &max_steps) || !get_u32(env, argv[2], &every) || !get_u32(env, argv[3], &mask)) return NULL;
	AsyncJob *j = (AsyncJob *)calloc(1, sizeof *j);
	if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
	j->h = h; j->kind = 3; j->max_steps = max_steps; j->check_every = every; j->stop_mask = mask;
	job_hold_engine(env, j, argv[0]);
	return job_start(env, j, "ca3d.stepUntil");
}

/* stepUntilCycleAsync(handle, maxSteps, checkEvery, stopMask) -> Promise<{stepsDone, reason, period, summary}> */
static napi_value js_step_until_cycle_async(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	uint32_t max_steps, every, mask;
	if (!h || !get_u32(env, argv[1], &max_steps) || !get_u32(env, argv[2], &every) || !get_u32(env, argv[3], &mask)) return NULL;
	AsyncJob *j = (AsyncJob *)calloc(1, sizeof *j);
	if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
	j->h = h; j->kind = 4; j->max_steps = max_steps; j->check_every = every; j->stop_mask = mask;
	job_hold_engine(env, j, argv[0]);
	return job_start(env, j, "ca3d.stepUntilCycle");
}

/* ---- ca3d_group_*: one JS thread drives the Z-slab split over several GPUs (include/ca3d.h) ---------------------------- */
typedef struct
{
	ca3d_group_t *g;
} GroupSlot;

static void finalize_group(napi_env env, void *data, void *hint)
{
	(void)env;
	(void)hint;
	GroupSlot *slot = (GroupSlot *)data;
	if (slot->g) ca3d_group_destroy(slot->g);
	free(slot);
}

static ca3d_group_t *get_group(napi_env env, napi_value v)
{
	void *p = NULL;
	if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((GroupSlot *)p)->g)
	{
		napi_throw_type_error(env, NULL, "expected an engine-group handle");
		return NULL;
	}
	return ((GroupSlot *)p)->g;
}

static napi_value js_group_create(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	void *d;
	size_t n;
	if (!get_typed(env, argv[0], napi_int32_array, 0, &d, &n)) return NULL;
	ca3d_group_t *g = NULL;
	int rc = ca3d_group_create((const int *)d, (int)n, &g);
	if (rc) return throw_ca3d(env, rc);
	GroupSlot *slot = (GroupSlot *)calloc(1, sizeof *slot);
	if (!slot) { ca3d_group_destroy(g); napi_throw_error(env, NULL, "out of memory"); return NULL; }
	slot->g = g;
	napi_value ext;
	NAPI_OK_OR_NULL(napi_create_external(env, slot, finalize_group, NULL, &ext));
	return ext;
}

static napi_value js_group_destroy(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	void *p = NULL;
	if (napi_get_value_external(env, argv[0], &p) == napi_ok && p)
	{
		GroupSlot *slot = (GroupSlot *)p;
		if (slot->g) ca3d_group_destroy(slot->g);
		slot->g = NULL;
	}
	return undefined(env);
}

static napi_value js_group_configure(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	uint32_t grid, layout, ghost;
	if (!g || !get_u32(env, argv[1], &grid) || !get_u32(env, argv[2], &layout) || !get_u32(env, argv[3], &ghost)) return NULL;
	int rc = ca3d_group_configure(g, grid, (int)layout, ghost);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_group_set_rules(napi_env env, napi_callback_info info)
{
	napi_value argv[6];
	if (!get_args(env, info, 6, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	if (!g) return NULL;
	void *m, *e, *c, *s, *b;
	size_t nm, ne, nc, ns, nb;
	if (!get_typed(env, argv[1], napi_int32_array, 0, &m, &nm) || !get_typed(env, argv[2], napi_int32_array, 0, &e, &ne) ||
	    !get_typed(env, argv[3], napi_int32_array, 0, &c, &nc) || !get_typed(env, argv[4], napi_uint32_array, 0, &s, &ns) ||
	    !get_typed(env, argv[5], napi_uint32_array, 0, &b, &nb))
		return NULL;
	if (ns != CA3D_LUT_LEN || nb != CA3D_LUT_LEN)
	{
		napi_throw_range_error(env, NULL, "survive/born must be Uint32Array(81)");
		return NULL;
	}
	int rc = ca3d_group_set_rules(g, (const int32_t *)m, (uint32_t)nm, (const int32_t *)e, (uint32_t)ne, (const int32_t *)c, (uint32_t)nc,
	                              (const uint32_t *)s, (const uint32_t *)b);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_group_upload_state(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	void *w;
	size_t n;
	if (!g || !get_typed(env, argv[1], napi_uint32_array, 0, &w, &n)) return NULL;
	int rc = ca3d_group_upload_state(g, (const uint32_t *)w, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_group_read_state(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	void *w;
	size_t n;
	if (!g || !get_typed(env, argv[1], napi_uint32_array, 0, &w, &n)) return NULL;
	int rc = ca3d_group_read_state(g, (uint32_t *)w, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_group_step(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	uint32_t n;
	if (!g || !get_u32(env, argv[1], &n)) return NULL;
	int rc = ca3d_group_step(g, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_group_synchronize(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	if (!g) return NULL;
	int rc = ca3d_group_synchronize(g);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_group_set_option(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	if (!g) return NULL;
	char name[64];
	size_t len = 0;
	int64_t value = 0;
	if (napi_get_value_string_utf8(env, argv[1], name, sizeof name, &len) != napi_ok || napi_get_value_int64(env, argv[2], &value) != napi_ok)
	{
		napi_throw_type_error(env, NULL, "expected (group, name, integer)");
		return NULL;
	}
	int rc = ca3d_group_set_option(g, name, value);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* info of rank's slab engine (kernel name, planes, step ...) */
static napi_value js_group_info(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	uint32_t rank;
	if (!g || !get_u32(env, argv[1], &rank)) return NULL;
	ca3d_t *e = NULL;
	int rc = ca3d_group_engine(g, (int)rank, &e);
	ca3d_info i;
	if (rc == 0) rc = ca3d_get_info(e, &i);
	if (rc) return throw_ca3d(env, rc);
	int n = 0;
	ca3d_group_size(g, &n);
	napi_value o, s;
	napi_create_object(env, &o);
	set_num(env, o, "ranks", n);
	set_num(env, o, "gridSize", i.grid_size);
	set_num(env, o, "z0", i.z0);
	set_num(env, o, "nz", i.nz);
	set_num(env, o, "ghost", i.ghost);
	set_num(env, o, "step", (double)i.step);
	set_num(env, o, "device", i.device);
	set_num(env, o, "launchesTotal", (double)i.launches_total);
	napi_create_string_utf8(env, i.kernel_name, NAPI_AUTO_LENGTH, &s);
	napi_set_named_property(env, o, "kernelName", s);
	/* what the slab really runs on (ca3d_slab_comm_info): the PCI bus id tells two GPUs from one GPU listed twice */
	ca3d_comm_info ci;
	if (ca3d_slab_comm_info(e, &ci) == CA3D_OK)
	{
		napi_create_string_utf8(env, ci.pci_bus_id, NAPI_AUTO_LENGTH, &s);
		napi_set_named_property(env, o, "pciBusId", s);
		set_num(env, o, "commRanks", ci.comm_ranks);
	}
	return o;
}

/* groupSummary(group, Uint32Array(G) | null) */
static napi_value js_group_summary(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	void *pp;
	size_t n;
	if (!g || !get_typed(env, argv[1], napi_uint32_array, 1, &pp, &n)) return NULL;
	ca3d_t *e = NULL;
	ca3d_info i;
	int rc = ca3d_group_engine(g, 0, &e);
	if (rc == 0) rc = ca3d_get_info(e, &i);
	if (rc) return throw_ca3d(env, rc);
	if (pp && n != i.grid_size)
	{
		napi_throw_range_error(env, NULL, "planePopulation must hold one entry per plane of the grid");
		return NULL;
	}
	ca3d_summary s;
	rc = ca3d_group_summarize(g, &s, (uint32_t *)pp);
	if (rc) return throw_ca3d(env, rc);
	return summary_object(env, &s, pp ? argv[1] : NULL);
}

static napi_value js_group_render(napi_env env, napi_callback_info info)
{
	napi_value argv[8];
	if (!get_args(env, info, 8, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	if (!g) return NULL;
	void *u, *pres, *light, *depth;
	size_t nu, npres, nlight, ndepth;
	uint32_t w, hh, spp;
	if (!get_typed(env, argv[1], napi_float32_array, 0, &u, &nu) || !get_u32(env, argv[2], &w) || !get_u32(env, argv[3], &hh) ||
	    !get_u32(env, argv[4], &spp) || !get_typed(env, argv[5], napi_uint8_array, 1, &pres, &npres) ||
	    !get_typed(env, argv[6], napi_uint16_array, 1, &light, &nlight) || !get_typed(env, argv[7], napi_uint16_array, 1, &depth, &ndepth))
		return NULL;
	const size_t px = (size_t)w * hh;
	if (nu != 128 || (pres && npres != px * 4) || (light && nlight != px * 4) || (depth && ndepth != px * 2))
	{
		napi_throw_range_error(env, NULL, "uniforms must be Float32Array(128); targets must match width*height");
		return NULL;
	}
	int rc = ca3d_group_render(g, (const float *)u, w, hh, spp, (uint8_t *)pres, (uint16_t *)light, (uint16_t *)depth);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/*
 * ca3d_ensemble_*: many independent 64^3 universes in one launch (include/ca3d.h). Synchronous and 1:1, like the group calls.
 */
typedef struct
{
	ca3d_ensemble_t *e;
	uint32_t n; /* universes, as last configured: what the arrays of ensembleStepUntil must hold */
} EnsembleSlot;

static void finalize_ensemble(napi_env env, void *data, void *hint)
{
	(void)env;
	(void)hint;
	EnsembleSlot *slot = (EnsembleSlot *)data;
	if (slot->e) ca3d_ensemble_destroy(slot->e);
	free(slot);
}

static ca3d_ensemble_t *get_ensemble(napi_env env, napi_value v)
{
	void *p = NULL;
	if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((EnsembleSlot *)p)->e)
	{
		napi_throw_type_error(env, NULL, "expected an ensemble handle");
		return NULL;
	}
	return ((EnsembleSlot *)p)->e;
}

static napi_value js_ensemble_create(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	int32_t device = 0;
	napi_get_value_int32(env, argv[0], &device);
	ca3d_ensemble_t *e = NULL;
	int rc = ca3d_ensemble_create(device, &e);
	if (rc) return throw_ca3d(env, rc);
	EnsembleSlot *slot = (EnsembleSlot *)calloc(1, sizeof *slot);
	if (!slot) { ca3d_ensemble_destroy(e); napi_throw_error(env, NULL, "out of memory"); return NULL; }
	slot->e = e;
	napi_value ext;
	NAPI_OK_OR_NULL(napi_create_external(env, slot, finalize_ensemble, NULL, &ext));
	return ext;
}

static napi_value js_ensemble_destroy(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	void *p = NULL;
	if (napi_get_value_external(env, argv[0], &p) == napi_ok && p)
	{
		EnsembleSlot *slot = (EnsembleSlot *)p;
		if (slot->e) ca3d_ensemble_destroy(slot->e);
		slot->e = NULL;
	}
	return undefined(env);
}

static napi_value js_ensemble_configure(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t grid, n;
	if (!e || !get_u32(env, argv[1], &grid) || !get_u32(env, argv[2], &n)) return NULL;
	int rc = ca3d_ensemble_configure(e, grid, n);
	if (rc) return throw_ca3d(env, rc);
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	((EnsembleSlot *)p)->n = n;
	return undefined(env);
}

/* ensembleConfigureNeighbourhood(handle, gridSize, n, neighbourhood): 0 von Neumann, 1 Moore (enum ca3d_ensemble_neighbourhood) */
static napi_value js_ensemble_configure_neighbourhood(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t grid, n, nb;
	if (!e || !get_u32(env, argv[1], &grid) || !get_u32(env, argv[2], &n) || !get_u32(env, argv[3], &nb)) return NULL;
	int rc = ca3d_ensemble_configure_neighbourhood(e, grid, n, (int)nb);
	if (rc) return throw_ca3d(env, rc);
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	((EnsembleSlot *)p)->n = n;
	return undefined(env);
}

/* ensembleNeighbourhood(handle) -> 0 | 1 */
static napi_value js_ensemble_neighbourhood(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	int nb = 0;
	int rc = ca3d_ensemble_get_neighbourhood(e, &nb);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_int32(env, nb, &v);
	return v;
}

/* ensembleConfigureClustered(handle, gridSize, n): Moore main list, three table pairs a universe (ca3d_ensemble_configure_clustered) */
static napi_value js_ensemble_configure_clustered(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t grid, n;
	if (!e || !get_u32(env, argv[1], &grid) || !get_u32(env, argv[2], &n)) return NULL;
	int rc = ca3d_ensemble_configure_clustered(e, grid, n);
	if (rc) return throw_ca3d(env, rc);
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	((EnsembleSlot *)p)->n = n;
	return undefined(env);
}

/* ensembleClustered(handle) -> 0 | 1 */
static napi_value js_ensemble_clustered(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	int c = 0;
	int rc = ca3d_ensemble_get_clustered(e, &c);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_int32(env, c, &v);
	return v;
}

/* ensembleSetBoundary(handle, boundary): 0 reference, 1 torus, 2 closed (ca3d_ensemble_set_boundary) */
static napi_value js_ensemble_set_boundary(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	int32_t boundary = 0;
	if (!e) return NULL;
	if (napi_get_value_int32(env, argv[1], &boundary) != napi_ok)
	{
		napi_throw_type_error(env, NULL, "boundary: a number");
		return NULL;
	}
	int rc = ca3d_ensemble_set_boundary(e, (int)boundary);
	if (rc) return throw_ca3d(env, rc);
	return undefined(env);
}

/* ensembleBoundary(handle) -> 0 | 1 | 2 */
static napi_value js_ensemble_boundary(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	int b = 0;
	int rc = ca3d_ensemble_get_boundary(e, &b);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_int32(env, b, &v);
	return v;
}

/* ensembleSetClusteredTables(handle, first, count, Uint32Array born masks, Uint32Array survive masks) — 3 words (main, edges, corners) a
 * rule, 1 or count rules each */
static napi_value js_ensemble_set_clustered_tables(napi_env env, napi_callback_info info)
{
	napi_value argv[5];
	if (!get_args(env, info, 5, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count;
	void *b, *s;
	size_t nb, ns;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count) || !get_typed(env, argv[3], napi_uint32_array, 0, &b, &nb) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &s, &ns))
		return NULL;
	if (nb != ns || nb == 0 || nb % 3u)
	{
		napi_throw_range_error(env, NULL, "born and survive masks must hold the same number of rules, three words (main, edges, corners) each");
		return NULL;
	}
	int rc = ca3d_ensemble_set_rule_tables_clustered(e, first, count, (const uint32_t *)b, (const uint32_t *)s, (uint32_t)(nb / 3u));
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleSetRules(handle, universe | 0xFFFFFFFF, main, edges, corners, survive, born) */
static napi_value js_ensemble_set_rules(napi_env env, napi_callback_info info)
{
	napi_value argv[7];
	if (!get_args(env, info, 7, argv)) return NULL;
	ca3d_ensemble_t *en = get_ensemble(env, argv[0]);
	uint32_t u;
	if (!en || !get_u32(env, argv[1], &u)) return NULL;
	void *m, *e, *c, *s, *b;
	size_t nm, ne, nc, ns, nb;
	if (!get_typed(env, argv[2], napi_int32_array, 0, &m, &nm) || !get_typed(env, argv[3], napi_int32_array, 0, &e, &ne) ||
	    !get_typed(env, argv[4], napi_int32_array, 0, &c, &nc) || !get_typed(env, argv[5], napi_uint32_array, 0, &s, &ns) ||
	    !get_typed(env, argv[6], napi_uint32_array, 0, &b, &nb))
		return NULL;
	if (ns != CA3D_LUT_LEN || nb != CA3D_LUT_LEN)
	{
		napi_throw_range_error(env, NULL, "survive/born must be Uint32Array(81)");
		return NULL;
	}
	int rc = ca3d_ensemble_set_rules(en, u, (const int32_t *)m, (uint32_t)nm, (const int32_t *)e, (uint32_t)ne, (const int32_t *)c, (uint32_t)nc,
	                                 (const uint32_t *)s, (const uint32_t *)b);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleUploadState / ensembleReadState(handle, first, Uint32Array(count * 8192)) */
static napi_value ensemble_transfer(napi_env env, napi_callback_info info, int upload)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first;
	void *w;
	size_t n;
	if (!e || !get_u32(env, argv[1], &first) || !get_typed(env, argv[2], napi_uint32_array, 0, &w, &n)) return NULL;
	if (n == 0 || n % 8192u)
	{
		napi_throw_range_error(env, NULL, "a universe holds 8192 words");
		return NULL;
	}
	int rc = upload ? ca3d_ensemble_upload_state(e, first, (uint32_t)(n / 8192u), (const uint32_t *)w, n)
	                : ca3d_ensemble_read_state(e, first, (uint32_t)(n / 8192u), (uint32_t *)w, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}
static napi_value js_ensemble_upload_state(napi_env env, napi_callback_info info) { return ensemble_transfer(env, info, 1); }
static napi_value js_ensemble_read_state(napi_env env, napi_callback_info info) { return ensemble_transfer(env, info, 0); }

static napi_value js_ensemble_step(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t n;
	if (!e || !get_u32(env, argv[1], &n)) return NULL;
	int rc = ca3d_ensemble_step(e, n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleStepUntil(handle, maxSteps, checkEvery, stopMask, Uint32Array(n) stepsDone, Uint32Array(n) reason) */
static napi_value js_ensemble_step_until(napi_env env, napi_callback_info info)
{
	napi_value argv[6];
	if (!get_args(env, info, 6, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t max_steps, every, mask;
	void *done, *reason;
	size_t nd, nr;
	if (!e || !get_u32(env, argv[1], &max_steps) || !get_u32(env, argv[2], &every) || !get_u32(env, argv[3], &mask) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &done, &nd) || !get_typed(env, argv[5], napi_uint32_array, 0, &reason, &nr))
		return NULL;
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	if (nd != ((EnsembleSlot *)p)->n || nr != nd)
	{
		napi_throw_range_error(env, NULL, "stepsDone and reason must hold one entry per universe");
		return NULL;
	}
	int rc = ca3d_ensemble_step_until(e, max_steps, every, mask, (uint32_t *)done, (uint32_t *)reason);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleStepUntilCycle(handle, maxSteps, checkEvery, stopMask, Uint32Array(n) stepsDone, Uint32Array(n) reason, Uint32Array(n) period) */
static napi_value js_ensemble_step_until_cycle(napi_env env, napi_callback_info info)
{
	napi_value argv[7];
	if (!get_args(env, info, 7, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t max_steps, every, mask;
	void *done, *reason, *period;
	size_t nd, nr, np;
	if (!e || !get_u32(env, argv[1], &max_steps) || !get_u32(env, argv[2], &every) || !get_u32(env, argv[3], &mask) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &done, &nd) || !get_typed(env, argv[5], napi_uint32_array, 0, &reason, &nr) ||
	    !get_typed(env, argv[6], napi_uint32_array, 0, &period, &np))
		return NULL;
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	if (nd != ((EnsembleSlot *)p)->n || nr != nd || np != nd)
	{
		napi_throw_range_error(env, NULL, "stepsDone, reason and period must hold one entry per universe");
		return NULL;
	}
	int rc = ca3d_ensemble_step_until_cycle(e, max_steps, every, mask, (uint32_t *)done, (uint32_t *)reason, (uint32_t *)period);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleStepUntilMoving(handle, maxSteps, checkEvery, stopMask, Uint32Array(n) stepsDone, Uint32Array(n) reason, Uint32Array(n) period,
 *                         Int32Array(3 n) shift) */
static napi_value js_ensemble_step_until_moving(napi_env env, napi_callback_info info)
{
	napi_value argv[8];
	if (!get_args(env, info, 8, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t max_steps, every, mask;
	void *done, *reason, *period, *shift;
	size_t nd, nr, np, ns;
	if (!e || !get_u32(env, argv[1], &max_steps) || !get_u32(env, argv[2], &every) || !get_u32(env, argv[3], &mask) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &done, &nd) || !get_typed(env, argv[5], napi_uint32_array, 0, &reason, &nr) ||
	    !get_typed(env, argv[6], napi_uint32_array, 0, &period, &np) || !get_typed(env, argv[7], napi_int32_array, 0, &shift, &ns))
		return NULL;
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	if (nd != ((EnsembleSlot *)p)->n || nr != nd || np != nd || ns != 3u * nd)
	{
		napi_throw_range_error(env, NULL, "stepsDone, reason and period must hold one entry per universe, shift three");
		return NULL;
	}
	int rc = ca3d_ensemble_step_until_moving(e, max_steps, every, mask, (uint32_t *)done, (uint32_t *)reason, (uint32_t *)period, (int32_t *)shift);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleStepUntilTrace(handle, maxSteps, checkEvery, stopMask, Uint32Array(n) stepsDone, Uint32Array(n) reason,
 *                        Uint32Array(n * samplesPerUniverse * 3) samples, samplesPerUniverse, Uint32Array(n) nSamples) */
static napi_value js_ensemble_step_until_trace(napi_env env, napi_callback_info info)
{
	napi_value argv[9];
	if (!get_args(env, info, 9, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t max_steps, every, mask, per;
	void *done, *reason, *samples, *count;
	size_t nd, nr, ns, nc;
	if (!e || !get_u32(env, argv[1], &max_steps) || !get_u32(env, argv[2], &every) || !get_u32(env, argv[3], &mask) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &done, &nd) || !get_typed(env, argv[5], napi_uint32_array, 0, &reason, &nr) ||
	    !get_typed(env, argv[6], napi_uint32_array, 0, &samples, &ns) || !get_u32(env, argv[7], &per) ||
	    !get_typed(env, argv[8], napi_uint32_array, 0, &count, &nc))
		return NULL;
	void *p = NULL;
	napi_get_value_external(env, argv[0], &p);
	if (nd != ((EnsembleSlot *)p)->n || nr != nd || nc != nd || ns != nd * (size_t)per * 3u)
	{
		napi_throw_range_error(env, NULL, "stepsDone, reason and nSamples must hold one entry per universe, samples 3 x samplesPerUniverse words per universe");
		return NULL;
	}
	int rc = ca3d_ensemble_step_until_trace(e, max_steps, every, mask, (uint32_t *)done, (uint32_t *)reason, (uint32_t *)samples, per, (uint32_t *)count);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleSummaries(handle, first, count) -> [summary object, ...] */
static napi_value js_ensemble_summaries(napi_env env, napi_callback_info info)
{
	napi_value argv[3];
	if (!get_args(env, info, 3, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count)) return NULL;
	ca3d_summary *recs = (ca3d_summary *)calloc(count ? count : 1u, sizeof *recs);
	if (!recs) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
	int rc = ca3d_ensemble_summarize(e, first, count, recs);
	if (rc) { free(recs); return throw_ca3d(env, rc); }
	napi_value out;
	napi_create_array_with_length(env, count, &out);
	for (uint32_t i = 0; i < count; i++) napi_set_element(env, out, i, summary_object(env, &recs[i], NULL));
	free(recs);
	return out;
}

/* An optional trailing connectivity (CA3D_CONNECT_*): argv[at] when the call has it and it is not undefined, CA3D_CONNECT_CLOSED otherwise.
 * argv holds at + 1 values, the absent ones undefined (napi_get_cb_info). */
static int get_connectivity(napi_env env, napi_value *argv, size_t at, uint32_t *out)
{
	napi_valuetype t = napi_undefined;
	*out = CA3D_CONNECT_CLOSED;
	if (napi_typeof(env, argv[at], &t) != napi_ok) return 0;
	return t == napi_undefined ? 1 : get_u32(env, argv[at], out);
}

/* the first `want` of want + 1 arguments are required: argv holds want + 1 values, the last undefined when the call left it out */
static int get_args_and_one(napi_env env, napi_callback_info info, size_t want, napi_value *argv)
{
	size_t argc = want + 1u;
	if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want)
	{
		napi_throw_type_error(env, NULL, "wrong number of arguments");
		return 0;
	}
	return 1;
}

/* ensembleCensus(handle, first, count, maxComponents, Uint32Array(count * maxComponents * 8) records, Uint32Array(count) nComponents,
 *                Uint32Array(count) remaining[, connectivity]) -> gpuMs: the connected objects of universes [first, first + count)
 * (ca3d_ensemble_census_connected; without a connectivity CA3D_CONNECT_CLOSED, ca3d_ensemble_census);
 * a record is ca3d_component's eight words: population, firstCell, boxMin, boxMax, digest low, digest high, 0, 0 (js/ca3d.js opens them) */
static napi_value js_ensemble_census(napi_env env, napi_callback_info info)
{
	napi_value argv[8];
	if (!get_args_and_one(env, info, 7, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count, max_components, connectivity;
	void *recs, *n, *rest;
	size_t nrecs, nn, nrest;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count) || !get_u32(env, argv[3], &max_components) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &recs, &nrecs) || !get_typed(env, argv[5], napi_uint32_array, 0, &n, &nn) ||
	    !get_typed(env, argv[6], napi_uint32_array, 0, &rest, &nrest) || !get_connectivity(env, argv, 7, &connectivity))
		return NULL;
	/* sizes the library refuses anyway leave nothing to check the arrays against: it names the reason */
	const int sizable = count && max_components && max_components <= 1024u;
	if (sizable && (nrecs != (size_t)count * max_components * 8u || nn != count || nrest != count))
	{
		napi_throw_range_error(env, NULL, "records must hold count * maxComponents * 8 words, nComponents and remaining one entry per universe");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_component) == 32, "a record crosses as eight words");
	float ms = 0.f;
	int rc = ca3d_ensemble_census_connected(e, first, count, max_components, connectivity, (ca3d_component *)recs, (uint32_t *)n, (uint32_t *)rest, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* ensembleIsolate(dstHandle, dstFirst, srcHandle, Uint32Array(2 * nJobs) jobs (universe, cell pairs), flags, Int32Array(4 * nJobs) out
 *                 [, connectivity])
 * -> gpuMs: job k makes the object of src's universe jobs[2 k] that holds the cell jobs[2 k + 1] the only thing in dst's universe
 * dstFirst + k (ca3d_ensemble_isolate_connected; without a connectivity CA3D_CONNECT_CLOSED, ca3d_ensemble_isolate); out[4 k ..] is
 * ca3d_isolated's four words: population, dx, dy, dz */
static napi_value js_ensemble_isolate(napi_env env, napi_callback_info info)
{
	napi_value argv[7];
	if (!get_args_and_one(env, info, 6, argv)) return NULL;
	ca3d_ensemble_t *dst = get_ensemble(env, argv[0]);
	if (!dst) return NULL;
	ca3d_ensemble_t *src = get_ensemble(env, argv[2]);
	uint32_t dst_first, flags, connectivity;
	void *jobs, *out;
	size_t njobs, nout;
	if (!src || !get_u32(env, argv[1], &dst_first) || !get_typed(env, argv[3], napi_uint32_array, 0, &jobs, &njobs) || !get_u32(env, argv[4], &flags) ||
	    !get_typed(env, argv[5], napi_int32_array, 0, &out, &nout) || !get_connectivity(env, argv, 6, &connectivity))
		return NULL;
	if (njobs % 2u || nout != 2u * njobs || njobs / 2u > 0xFFFFFFFFu)
	{
		napi_throw_range_error(env, NULL, "jobs must hold a (universe, cell) pair and out four words a job");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_isolate_job) == 8 && sizeof(ca3d_isolated) == 16, "a job crosses as two words, a result as four");
	float ms = 0.f;
	/* (no job: the library refuses the call and names the reason; it reads neither array) */
	int rc = ca3d_ensemble_isolate_connected(dst, dst_first, src, (uint32_t)(njobs / 2u), (const ca3d_isolate_job *)jobs, flags, connectivity,
	                                         (ca3d_isolated *)out, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* cutWindows(engineHandle, ensembleHandle, Uint32Array(4 * n) windows (universe, x, y, z each)) -> gpuMs: universe windows[4 k] of the
 * ensemble becomes the 64^3 window of the engine's current state at origin windows[4 k + 1 ..] (ca3d_cut_windows);
 * stampWindows(engineHandle, ensembleHandle, windows, mode) -> gpuMs: those universes are stamped into the engine's state there
 * (ca3d_stamp_windows; mode CA3D_STAMP_OR / REPLACE / ERASE). `stamp`: which of the two */
static napi_value windows_call(napi_env env, napi_callback_info info, int stamp)
{
	napi_value argv[4];
	if (!get_args(env, info, stamp ? 4 : 3, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[1]);
	uint32_t mode = 0;
	void *w;
	size_t nw;
	if (!e || !get_typed(env, argv[2], napi_uint32_array, 0, &w, &nw) || (stamp && !get_u32(env, argv[3], &mode))) return NULL;
	if (nw % 4u || nw / 4u > 0xFFFFFFFFu)
	{
		napi_throw_range_error(env, NULL, "windows must hold (universe, x, y, z) a window");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_window) == 16, "a window crosses as four words");
	float ms = 0.f;
	/* (no window: the library refuses the call and names the reason; it does not read the array) */
	int rc = stamp ? ca3d_stamp_windows(h, e, (uint32_t)(nw / 4u), (const ca3d_window *)w, mode, &ms)
	               : ca3d_cut_windows(h, e, (uint32_t)(nw / 4u), (const ca3d_window *)w, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}
static napi_value js_cut_windows(napi_env env, napi_callback_info info) { return windows_call(env, info, 0); }
static napi_value js_stamp_windows(napi_env env, napi_callback_info info) { return windows_call(env, info, 1); }

/* ensembleCompose(dstHandle, dstFirst, srcHandle, Int32Array(6 * nParts) parts (universe, orientation, x, y, z, 0 each),
 * Uint32Array(nDst + 1) partBegin, flags, Uint32Array(4 * nDst) out) -> gpuMs: dst's universe dstFirst + k becomes the union of parts
 * partBegin[k] .. partBegin[k + 1] - 1, src's universes turned and shifted (ca3d_ensemble_compose); out[4 k ..] is ca3d_composed's four
 * words: population, placed, overlap, clipped */
static napi_value js_ensemble_compose(napi_env env, napi_callback_info info)
{
	napi_value argv[7];
	if (!get_args(env, info, 7, argv)) return NULL;
	ca3d_ensemble_t *dst = get_ensemble(env, argv[0]);
	if (!dst) return NULL;
	ca3d_ensemble_t *src = get_ensemble(env, argv[2]);
	uint32_t dst_first, flags;
	void *parts, *begin, *out;
	size_t nparts, nbegin, nout;
	if (!src || !get_u32(env, argv[1], &dst_first) || !get_typed(env, argv[3], napi_int32_array, 0, &parts, &nparts) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &begin, &nbegin) || !get_u32(env, argv[5], &flags) ||
	    !get_typed(env, argv[6], napi_uint32_array, 0, &out, &nout))
		return NULL;
	/* the library reads partBegin[0 .. nDst] and parts[0 .. partBegin[nDst]): both must lie inside the arrays given */
	if (nbegin < 1u || nbegin - 1u > 0xFFFFFFFFu || nout != 4u * (nbegin - 1u) || nparts % 6u ||
	    (nbegin > 1u && (size_t)((const uint32_t *)begin)[nbegin - 1u] > nparts / 6u))
	{
		napi_throw_range_error(env, NULL, "parts must hold six words a part, partBegin one entry a destination and one more, its last no more than the parts, out four words a destination");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_compose_part) == 24 && sizeof(ca3d_composed) == 16, "a part crosses as six words, a record as four");
	float ms = 0.f;
	/* (no destination: the library refuses the call and names the reason; it reads no array) */
	int rc = ca3d_ensemble_compose(dst, dst_first, (uint32_t)(nbegin - 1u), src, (const ca3d_compose_part *)parts, (const uint32_t *)begin, flags,
	                               (ca3d_composed *)out, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* ensembleCanon(handle, first, count, Uint32Array(count * 8) records, Uint32Array(count * 96) digests or null) -> gpuMs: the name of
 * universes [first, first + count) up to the 48 orientations and translation (ca3d_ensemble_canon); a record is ca3d_canon's eight
 * words: key low, key high, symmetry low, symmetry high, orientation, population, boxMin, boxMax; a digest crosses as low word, high
 * word (js/ca3d.js opens them) */
static napi_value js_ensemble_canon(napi_env env, napi_callback_info info)
{
	napi_value argv[5];
	if (!get_args(env, info, 5, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count;
	void *recs, *dig;
	size_t nrecs, ndig;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count) || !get_typed(env, argv[3], napi_uint32_array, 0, &recs, &nrecs) ||
	    !get_typed(env, argv[4], napi_uint32_array, 1, &dig, &ndig))
		return NULL;
	/* (count 0: the library refuses the call and names the reason; it writes neither array) */
	if (count && (nrecs != (size_t)count * 8u || (dig && ndig != (size_t)count * 96u)))
	{
		napi_throw_range_error(env, NULL, "records must hold eight words a universe, digests 96 words a universe or be null");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_canon) == 32, "a record crosses as eight words");
	float ms = 0.f;
	int rc = ca3d_ensemble_canon(e, first, count, (ca3d_canon *)recs, (uint64_t *)dig, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* ensembleCanonPeriod(handle, first, Uint32Array(count) periods, Uint32Array(count * 8) records, Uint32Array(count * keysStride * 2) keys
 * or null, keysStride) -> gpuMs: universes [first, first + count) named over periods[k] steps of their own, taken inside the kernel
 * (ca3d_ensemble_canon_period); a record is ca3d_canon_period's eight words: key low, key high, symmetry low, symmetry high,
 * orientation, phase, population, flagsShift; a key crosses as low word, high word (js/ca3d.js opens them) */
static napi_value js_ensemble_canon_period(napi_env env, napi_callback_info info)
{
	napi_value argv[6];
	if (!get_args(env, info, 6, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, stride;
	void *periods, *recs, *keys;
	size_t count, nrecs, nkeys;
	if (!e || !get_u32(env, argv[1], &first) || !get_typed(env, argv[2], napi_uint32_array, 0, &periods, &count) ||
	    !get_typed(env, argv[3], napi_uint32_array, 0, &recs, &nrecs) || !get_typed(env, argv[4], napi_uint32_array, 1, &keys, &nkeys) ||
	    !get_u32(env, argv[5], &stride))
		return NULL;
	if (count > 0xFFFFFFFFu || nrecs != count * 8u || (keys && nkeys != count * (size_t)stride * 2u))
	{
		napi_throw_range_error(env, NULL, "records must hold eight words a universe, keys two words a universe and slot of keysStride or be null");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_canon_period) == 32, "a record crosses as eight words");
	float ms = 0.f;
	/* (count 0: the library refuses the call and names the reason; it reads and writes no array, and an empty typed array may have no
	 * address at all) */
	uint32_t none[8];
	if (!count) periods = recs = none;
	int rc = ca3d_ensemble_canon_period(e, first, (uint32_t)count, (const uint32_t *)periods, (ca3d_canon_period *)recs, (uint64_t *)keys, stride, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* ensembleEnvelope(srcHandle, first, Uint32Array(count) periods, dstHandle or null, dstFirst, flags, Uint32Array(count * 12) records)
 * -> gpuMs: envelope, stator, rotor and heat of universes [first, first + count) over periods[k] steps of their own, taken inside the
 * kernel, the images flags selects written into dst's universes from dstFirst (ca3d_ensemble_envelope); a record is ca3d_envelope's
 * twelve words: period, flags, heat, populationSum, envelopePopulation, statorPopulation, envelopeMin, envelopeMax, rotorMin, rotorMax
 * (x | y << 8 | z << 16 each), 0, 0 (js/ca3d.js opens them) */
static napi_value js_ensemble_envelope(napi_env env, napi_callback_info info)
{
	napi_value argv[7];
	if (!get_args(env, info, 7, argv)) return NULL;
	ca3d_ensemble_t *src = get_ensemble(env, argv[0]);
	if (!src) return NULL;
	ca3d_ensemble_t *dst = NULL;
	napi_valuetype t;
	napi_typeof(env, argv[3], &t);
	if (t != napi_null && t != napi_undefined && !(dst = get_ensemble(env, argv[3]))) return NULL;
	uint32_t first, dst_first, flags;
	void *periods, *recs;
	size_t count, nrecs;
	if (!get_u32(env, argv[1], &first) || !get_typed(env, argv[2], napi_uint32_array, 0, &periods, &count) || !get_u32(env, argv[4], &dst_first) ||
	    !get_u32(env, argv[5], &flags) || !get_typed(env, argv[6], napi_uint32_array, 0, &recs, &nrecs))
		return NULL;
	if (count > 0xFFFFFFFFu || nrecs != count * 12u)
	{
		napi_throw_range_error(env, NULL, "records must hold twelve words a universe");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_envelope) == 48, "a record crosses as twelve words");
	float ms = 0.f;
	/* (count 0: the library refuses the call and names the reason; it reads and writes no array, and an empty typed array may have no
	 * address at all) */
	uint32_t none[12];
	if (!count) periods = recs = none;
	int rc = ca3d_ensemble_envelope(src, first, (uint32_t)count, (const uint32_t *)periods, dst, dst_first, flags, (ca3d_envelope *)recs, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* ensembleDamage(srcHandle, first, Uint32Array(count) steps, Uint32Array(count) twins or null, Uint32Array(count * 4) flips or null,
 *                dstHandle or null, dstFirst, flags, Uint32Array(count * 12) records, Uint32Array(count * curveStride) curve or null,
 *                curveStride) -> gpuMs: the Hamming distance between universes [first, first + count) and their perturbed twins over
 * steps[k] steps of their own, taken inside the kernel, the last difference written into dst's universes from dstFirst when flags asks
 * for it (ca3d_ensemble_damage); a record is ca3d_damage's twelve words: steps, flags, healedAt, finalDistance, initialDistance,
 * maxDistance, maxAt, distanceSum, damageMin, damageMax, touchedMin, touchedMax (x | y << 8 | z << 16 each) (js/ca3d.js opens them) */
static napi_value js_ensemble_damage(napi_env env, napi_callback_info info)
{
	napi_value argv[11];
	if (!get_args(env, info, 11, argv)) return NULL;
	ca3d_ensemble_t *src = get_ensemble(env, argv[0]);
	if (!src) return NULL;
	ca3d_ensemble_t *dst = NULL;
	napi_valuetype t;
	napi_typeof(env, argv[5], &t);
	if (t != napi_null && t != napi_undefined && !(dst = get_ensemble(env, argv[5]))) return NULL;
	uint32_t first, dst_first, flags, stride;
	void *steps, *twins, *flips, *recs, *curve;
	size_t count, ntwins, nflips, nrecs, ncurve;
	if (!get_u32(env, argv[1], &first) || !get_typed(env, argv[2], napi_uint32_array, 0, &steps, &count) ||
	    !get_typed(env, argv[3], napi_uint32_array, 1, &twins, &ntwins) || !get_typed(env, argv[4], napi_uint32_array, 1, &flips, &nflips) ||
	    !get_u32(env, argv[6], &dst_first) || !get_u32(env, argv[7], &flags) || !get_typed(env, argv[8], napi_uint32_array, 0, &recs, &nrecs) ||
	    !get_typed(env, argv[9], napi_uint32_array, 1, &curve, &ncurve) || !get_u32(env, argv[10], &stride))
		return NULL;
	if (count > 0xFFFFFFFFu || nrecs != count * 12u || (twins && ntwins != count) || (flips && nflips != count * CA3D_DAMAGE_FLIPS) ||
	    (curve && ncurve != count * (size_t)stride))
	{
		napi_throw_range_error(env, NULL, "records must hold twelve words a universe, twins one, flips four and the curve curveStride");
		return NULL;
	}
	_Static_assert(sizeof(ca3d_damage) == 48, "a record crosses as twelve words");
	float ms = 0.f;
	/* (count 0: the library refuses the call and names the reason; it reads and writes no array, and an empty typed array may have no
	 * address at all) */
	uint32_t none[12];
	if (!count)
	{
		steps = recs = none;
		twins = flips = curve = NULL;
	}
	int rc = ca3d_ensemble_damage(src, first, (uint32_t)count, (const uint32_t *)steps, (const uint32_t *)twins, (const uint32_t *)flips, dst, dst_first, flags,
	                              (ca3d_damage *)recs, (uint32_t *)curve, stride, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

/* ensembleUsage(handle, first, Uint32Array(count) steps, Uint32Array(count * 108) records) -> gpuMs: which entries of their rule tables
 * universes [first, first + count) read over steps[k] steps of their own, taken inside the kernel (ca3d_ensemble_usage); a record is
 * ca3d_usage's 108 words: steps, flags, usedBorn[3], usedSurvive[3], dead[49], alive[49], 0, 0 (js/ca3d.js opens them) */
static napi_value js_ensemble_usage(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	uint32_t first;
	void *steps, *recs;
	size_t count, nrecs;
	if (!get_u32(env, argv[1], &first) || !get_typed(env, argv[2], napi_uint32_array, 0, &steps, &count) ||
	    !get_typed(env, argv[3], napi_uint32_array, 0, &recs, &nrecs))
		return NULL;
	_Static_assert(sizeof(ca3d_usage) == 432, "a record crosses as 108 words");
	if (count > 0xFFFFFFFFu || nrecs != count * (sizeof(ca3d_usage) / 4u))
	{
		napi_throw_range_error(env, NULL, "records must hold 108 words a universe");
		return NULL;
	}
	float ms = 0.f;
	/* (count 0: the library refuses the call and names the reason; it reads and writes no array, and an empty typed array may have no
	 * address at all) */
	uint32_t none[1];
	if (!count) steps = recs = none;
	int rc = ca3d_ensemble_usage(e, first, (uint32_t)count, (const uint32_t *)steps, (ca3d_usage *)recs, &ms);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_double(env, (double)ms, &v);
	return v;
}

static napi_value js_ensemble_synchronize(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	int rc = ca3d_ensemble_synchronize(e);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_ensemble_stats(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	ca3d_stats st;
	int rc = ca3d_ensemble_get_stats(e, &st);
	if (rc) return throw_ca3d(env, rc);
	napi_value o;
	napi_create_object(env, &o);
	set_num(env, o, "steps", (double)st.steps);
	set_num(env, o, "kernelLaunches", (double)st.kernel_launches);
	set_num(env, o, "gpuMs", st.gpu_ms);
	set_num(env, o, "cellSteps", st.cell_steps);
	set_num(env, o, "algorithmicBytes", st.algorithmic_bytes);
	return o;
}

/* ensembleRenderSheet(handle, first, count, Float32Array(128) uniforms, tileW, tileH, columns, spp, Uint8Array(W * H * 4) presentation):
 * the contact sheet of universes [first, first + count), W = columns * tileW, H = ceil(count / columns) * tileH (ca3d_ensemble_render_sheet) */
static napi_value js_ensemble_render_sheet(napi_env env, napi_callback_info info)
{
	napi_value argv[9];
	if (!get_args(env, info, 9, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count, tw, th, columns, spp;
	void *u, *pres;
	size_t nu, npres;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count) || !get_typed(env, argv[3], napi_float32_array, 0, &u, &nu) ||
	    !get_u32(env, argv[4], &tw) || !get_u32(env, argv[5], &th) || !get_u32(env, argv[6], &columns) || !get_u32(env, argv[7], &spp) ||
	    !get_typed(env, argv[8], napi_uint8_array, 0, &pres, &npres))
		return NULL;
	/* sizes the library refuses anyway leave no sheet to check the array against: it names the reason */
	const int sizable = count && columns && tw && tw <= 1024u && th && th <= 1024u;
	const uint64_t px = sizable ? (uint64_t)columns * tw * (((uint64_t)count + columns - 1u) / columns) * th : 0u;
	if (nu != 128 || (sizable && px <= (1ull << 26) && npres != px * 4u))
	{
		napi_throw_range_error(env, NULL, "uniforms must be Float32Array(128); presentation must hold columns*tileW x ceil(count/columns)*tileH x 4 bytes");
		return NULL;
	}
	int rc = ca3d_ensemble_render_sheet(e, first, count, (const float *)u, tw, th, columns, spp, (uint8_t *)pres, NULL, NULL);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_ensemble_sheet_stats(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	if (!e) return NULL;
	ca3d_render_stats st;
	int rc = ca3d_ensemble_get_sheet_stats(e, &st);
	if (rc) return throw_ca3d(env, rc);
	napi_value o;
	napi_create_object(env, &o);
	set_num(env, o, "gpuMs", st.gpu_ms);
	set_num(env, o, "primaryRays", (double)st.primary_rays);
	set_num(env, o, "shadowRays", (double)st.shadow_rays);
	set_num(env, o, "primaryCellVisits", (double)st.primary_cell_visits);
	set_num(env, o, "shadowCellVisits", (double)st.shadow_cell_visits);
	return o;
}

/*
 * ca3d_seed_state and its kin: a spec crosses as eight u32 in ca3d_seed's own order — seed, andRounds, boxMin x y z, boxMax x y z
 * (js/ca3d.js builds them: seedSpec).
 */
static const ca3d_seed *get_specs(napi_env env, napi_value v, size_t *n_specs)
{
	void *w;
	size_t n;
	if (!get_typed(env, v, napi_uint32_array, 0, &w, &n)) return NULL;
	if (n == 0 || n % 8u)
	{
		napi_throw_range_error(env, NULL, "a seed spec holds 8 words: seed, andRounds, boxMin[3], boxMax[3]");
		return NULL;
	}
	*n_specs = n / 8u;
	return (const ca3d_seed *)w;
}

/* seedState(handle, Uint32Array(8)) */
static napi_value js_seed_state(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	size_t n;
	const ca3d_seed *spec = h ? get_specs(env, argv[1], &n) : NULL;
	if (!spec) return NULL;
	int rc = ca3d_seed_state(h, spec);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* groupSeedState(group, Uint32Array(8)) */
static napi_value js_group_seed_state(napi_env env, napi_callback_info info)
{
	napi_value argv[2];
	if (!get_args(env, info, 2, argv)) return NULL;
	ca3d_group_t *g = get_group(env, argv[0]);
	size_t n;
	const ca3d_seed *spec = g ? get_specs(env, argv[1], &n) : NULL;
	if (!spec) return NULL;
	int rc = ca3d_group_seed_state(g, spec);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleSeedState(handle, first, count, Uint32Array(8 * (1 | count))) */
static napi_value js_ensemble_seed_state(napi_env env, napi_callback_info info)
{
	napi_value argv[4];
	if (!get_args(env, info, 4, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count)) return NULL;
	size_t n;
	const ca3d_seed *specs = get_specs(env, argv[3], &n);
	if (!specs) return NULL;
	int rc = ca3d_ensemble_seed_state(e, first, count, specs, (uint32_t)n);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

/* ensembleSetRuleTables(handle, first, count, Uint32Array born masks, Uint32Array survive masks) — 1 or count entries each */
static napi_value js_ensemble_set_rule_tables(napi_env env, napi_callback_info info)
{
	napi_value argv[5];
	if (!get_args(env, info, 5, argv)) return NULL;
	ca3d_ensemble_t *e = get_ensemble(env, argv[0]);
	uint32_t first, count;
	void *b, *s;
	size_t nb, ns;
	if (!e || !get_u32(env, argv[1], &first) || !get_u32(env, argv[2], &count) || !get_typed(env, argv[3], napi_uint32_array, 0, &b, &nb) ||
	    !get_typed(env, argv[4], napi_uint32_array, 0, &s, &ns))
		return NULL;
	if (nb != ns || nb == 0)
	{
		napi_throw_range_error(env, NULL, "born and survive masks must hold the same number of entries");
		return NULL;
	}
	int rc = ca3d_ensemble_set_rule_tables(e, first, count, (const uint32_t *)b, (const uint32_t *)s, (uint32_t)nb);
	return rc ? throw_ca3d(env, rc) : undefined(env);
}

static napi_value js_recovered_launches(napi_env env, napi_callback_info info)
{
	napi_value argv[1];
	if (!get_args(env, info, 1, argv)) return NULL;
	ca3d_t *h = get_handle(env, argv[0]);
	if (!h) return NULL;
	uint32_t n = 0;
	int rc = ca3d_recovered_launches(h, &n);
	if (rc) return throw_ca3d(env, rc);
	napi_value v;
	napi_create_uint32(env, n, &v);
	return v;
}

static napi_value js_abi_version(napi_env env, napi_callback_info info)
{
	(void)info;
	napi_value v;
	napi_create_int32(env, ca3d_abi_version(), &v);
	return v;
}

/* ca3d_get_jit_stats: what the run-time compiler did in this process (compiled / read from the on-disk cache / already loaded) */
static napi_value js_jit_stats(napi_env env, napi_callback_info info)
{
	(void)info;
	ca3d_jit_stats st;
	int rc = ca3d_get_jit_stats(&st);
	if (rc != CA3D_OK) return throw_ca3d(env, rc);
	napi_value o, s;
	napi_create_object(env, &o);
	set_num(env, o, "programsCompiled", (double)st.programs_compiled);
	set_num(env, o, "programsFromDisk", (double)st.programs_from_disk);
	set_num(env, o, "programsFromMemory", (double)st.programs_from_memory);
	set_num(env, o, "compileMs", st.compile_ms);
	set_num(env, o, "diskReadMs", st.disk_read_ms);
	set_num(env, o, "loadMs", st.load_ms);
	napi_create_string_utf8(env, st.cache_dir, NAPI_AUTO_LENGTH, &s);
	napi_set_named_property(env, o, "cacheDir", s);
	return o;
}

static napi_value init(napi_env env, napi_value exports)
{
	static const struct { const char *name; napi_callback fn; } fns[] = {
	    {"abiVersion", js_abi_version}, {"jitStats", js_jit_stats}, {"deviceCount", js_device_count}, {"create", js_create}, {"destroy", js_destroy},
	    {"configure", js_configure}, {"configureSlab", js_configure_slab}, {"setRules", js_set_rules},
	    {"uploadState", js_upload_state}, {"readState", js_read_state}, {"step", js_step}, {"flush", js_flush}, {"slabStep", js_slab_step}, {"slabStepPhase", js_slab_step_phase},
	    {"synchronize", js_synchronize}, {"info", js_info}, {"stats", js_stats}, {"render", js_render},
	    {"renderStats", js_render_stats}, {"renderPipeline", js_render_pipeline}, {"setOption", js_set_option},
	    {"commUniqueId", js_comm_unique_id}, {"slabCommInit", js_slab_comm_init}, {"slabRun", js_slab_run}, {"slabExchange", js_slab_exchange},
	    {"slabGather", js_slab_gather},
	    {"recoveredLaunches", js_recovered_launches},
	    {"groupCreate", js_group_create}, {"groupDestroy", js_group_destroy}, {"groupConfigure", js_group_configure}, {"groupSetRules", js_group_set_rules},
	    {"groupUploadState", js_group_upload_state}, {"groupReadState", js_group_read_state}, {"groupStep", js_group_step},
	    {"groupSynchronize", js_group_synchronize}, {"groupSetOption", js_group_set_option}, {"groupInfo", js_group_info}, {"groupRender", js_group_render},
	    {"readStateAsync", js_read_state_async}, {"renderAsync", js_render_async}, {"synchronizeAsync", js_synchronize_async},
	    {"summary", js_summary}, {"groupSummary", js_group_summary}, {"stepUntilAsync", js_step_until_async}, {"stepUntilCycleAsync", js_step_until_cycle_async},
	    {"ensembleCreate", js_ensemble_create}, {"ensembleDestroy", js_ensemble_destroy}, {"ensembleConfigure", js_ensemble_configure},
	    {"ensembleSetRules", js_ensemble_set_rules}, {"ensembleUploadState", js_ensemble_upload_state}, {"ensembleReadState", js_ensemble_read_state},
	    {"ensembleStep", js_ensemble_step}, {"ensembleStepUntil", js_ensemble_step_until}, {"ensembleStepUntilCycle", js_ensemble_step_until_cycle}, {"ensembleStepUntilMoving", js_ensemble_step_until_moving}, {"ensembleStepUntilTrace", js_ensemble_step_until_trace}, {"ensembleSummaries", js_ensemble_summaries},
	    {"ensembleSynchronize", js_ensemble_synchronize}, {"ensembleStats", js_ensemble_stats},
	    {"seedState", js_seed_state}, {"groupSeedState", js_group_seed_state}, {"ensembleSeedState", js_ensemble_seed_state},
	    {"ensembleSetRuleTables", js_ensemble_set_rule_tables},
	    {"ensembleConfigureNeighbourhood", js_ensemble_configure_neighbourhood}, {"ensembleNeighbourhood", js_ensemble_neighbourhood},
	    {"ensembleConfigureClustered", js_ensemble_configure_clustered}, {"ensembleClustered", js_ensemble_clustered},
	    {"ensembleSetBoundary", js_ensemble_set_boundary}, {"ensembleBoundary", js_ensemble_boundary},
	    {"ensembleSetClusteredTables", js_ensemble_set_clustered_tables},
	    {"ensembleRenderSheet", js_ensemble_render_sheet}, {"ensembleSheetStats", js_ensemble_sheet_stats},
	    {"ensembleCensus", js_ensemble_census}, {"ensembleIsolate", js_ensemble_isolate}, {"ensembleCompose", js_ensemble_compose},
	    {"ensembleCanon", js_ensemble_canon},
	    {"ensembleCanonPeriod", js_ensemble_canon_period},
	    {"ensembleEnvelope", js_ensemble_envelope},
	    {"ensembleUsage", js_ensemble_usage},
	    {"cutWindows", js_cut_windows}, {"stampWindows", js_stamp_windows},
	    {"ensembleDamage", js_ensemble_damage}};
	for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++)
	{
		napi_value f;
		if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
		napi_set_named_property(env, exports, fns[i].name, f);
	}
	return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
