/*
 * JavaScript host of the MI355X engine: the rule / grid / step surface of the reference's MainModule
 * (main_pathtraced.js) over the N-API addon (addon/ca3d_napi.c -> include/ca3d.h). CommonJS, Node >= 12.
 *
 * Host-side helpers mirror the reference's own (same names without the underscore, same quirks): they are the
 * JS twin of cellularautomatons3d_amd/host.py and are checked against the same captured fixtures.
 * There is no CPU stepping here: without the addon and a GPU, `new Engine()` throws.
 */
"use strict";
const path = require("path");

const NEIGHBOURS_STORAGE_LEN = 27; // main_pathtraced.js:10
const WORK_GROUP_SIZE = 16; // main_pathtraced.js:5
const LAYOUT_PACKED32 = 0;
const LAYOUT_UNPACKED = 1;

// main_pathtraced.js:13-94
const vn = [1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1];
const vn2d = vn.slice(0, 12);
const moore2d = vn2d.concat([1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0]);
const layer = (z) => [1, 0, z, -1, 0, z, 0, 1, z, 0, -1, z, 1, 1, z, -1, 1, z, 1, -1, z, -1, -1, z, 0, 0, z];
const NEIGHBOURHOOD_MAP = {
	"moore": new Int32Array(moore2d.concat(layer(1), layer(-1))),
	"moore 2D": new Int32Array(moore2d),
	"von neumann": new Int32Array(vn),
	"von neumann 2D": new Int32Array(vn2d),
	"edges": new Int32Array([1, 1, 0, -1, 1, 0, 0, 1, 1, 0, 1, -1, 1, -1, 0, -1, -1, 0, 0, -1, 1, 0, -1, -1, 1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1]),
	"corners": new Int32Array([1, 1, 1, -1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1, 1, -1, -1, -1, -1, -1])
};

// _rulesComponentsToValues (main_pathtraced.js:554-581); NaN components are dropped where the reference lets its
// typed-array store ignore them.
function rulesComponentsToValues(rulesComponents)
{
	const result = [];
	const components = rulesComponents.split(" ").join("").split(",");
	for (let i = 0; i < components.length; i++)
	{
		if (components[i].indexOf("-") > -1)
		{
			const range = components[i].split("-");
			const start = parseInt(range[0], 10);
			const end = parseInt(range[1], 10);
			for (let j = start; j <= end; j++) { result.push(Math.min(j, 26)); }
		}
		else
		{
			const v = Math.min(parseInt(components[i], 10), 26);
			if (!Number.isNaN(v)) { result.push(v); }
		}
	}
	return result;
}

// _recalculateRulesValues (583-622) -> { born: Uint32Array(81), survive: Uint32Array(81) }
function recalculateRulesValues(r)
{
	const rulesets = [r.born, r.survive, r.bornEdges, r.surviveEdges, r.bornCorners, r.surviveCorners].map(rulesComponentsToValues);
	const born = new Uint32Array(NEIGHBOURS_STORAGE_LEN * 3);
	const survive = new Uint32Array(NEIGHBOURS_STORAGE_LEN * 3);
	let offset = 0;
	for (let i = 0; i < rulesets.length; i += 2)
	{
		for (const v of rulesets[i]) { born[v + offset] = 1; }
		for (const v of rulesets[i + 1]) { survive[v + offset] = 1; }
		offset += NEIGHBOURS_STORAGE_LEN;
	}
	return { born, survive };
}

const DEFAULT_RULES = { neighbourhood: "von neumann", born: "1,3", survive: "0-6", bornEdges: "27", surviveEdges: "27", bornCorners: "27", surviveCorners: "27" };

// _gridSizeUIFormatter (675-693)
function gridSizeUIFormatter(v)
{
	let out = v;
	const m = v % 32;
	if (m > 0) { out = m <= 16 ? v - m : v - m + 32; }
	return out;
}

// _getClusterIdxFromGridCoordinates (1170-1178)
function getClusterIdxFromGridCoordinates(gridSize, c)
{
	const cols = gridSize / 32;
	return (Math.floor(c.x / 32) % cols) + (c.y % gridSize) * cols + (c.z % gridSize) * cols * gridSize;
}

// initial state of _setupStorageBuffers (1241-1297); `random` replaces the unseeded Math.random
function initialState(gridSize, randomInitialState, random)
{
	if (!(gridSize > 0) || gridSize % 32) { throw new RangeError("grid size must be a positive multiple of 32"); }
	const data = new Uint32Array((gridSize / 32) * gridSize * gridSize);
	const center = Math.floor(gridSize * 0.5) - 1;
	if (randomInitialState)
	{
		const rnd = random || mulberry32(0xCA3D0001);
		for (let i = -2; i < 3; i++) for (let j = -2; j < 3; j++) for (let k = -2; k < 3; k++)
		{
			const idx = getClusterIdxFromGridCoordinates(gridSize, { x: center + i, y: center + j, z: center + k });
			if (rnd() > 0.5) { data[idx] = data[idx] | (1 << center + i); }
			else { data[idx] = data[idx] & ~(1 << center + i); }
		}
	}
	else
	{
		data[getClusterIdxFromGridCoordinates(gridSize, { x: center, y: center, z: center })] = 1 << (center % 32);
	}
	return data;
}

function mulberry32(a)
{
	return function () { a |= 0; a = a + 0x6D2B79F5 | 0; let t = Math.imul(a ^ a >>> 15, 1 | a); t = t + Math.imul(t ^ t >>> 7, 61 | t) ^ t; return ((t ^ t >>> 14) >>> 0) / 4294967296; };
}

function dispatchShape(gridSize)
{
	const wg = Math.ceil(gridSize / WORK_GROUP_SIZE);
	return [gridSize / 32, wg, wg]; // main_pathtraced.js:1805-1806
}

// K of ca3d_ensemble_step_until_trace (include/ca3d.h; host.trace_samples): the samples one universe can leave — one per check point at
// steps 0, checkEvery, 2 checkEvery ... of the call, and the last one at maxSteps
function traceSamples(maxSteps, checkEvery)
{
	if (!(checkEvery >= 1) || !(maxSteps >= 0)) { throw new RangeError("checkEvery must be at least 1 and maxSteps at least 0"); }
	return Math.ceil(maxSteps / checkEvery) + 1;
}

// counter-based synthetic fill shared with host.py / the oracle (SURVEY 8(d))
function randomFill(nWords, seed, andRounds)
{
	seed = seed === undefined ? 0xCA3D0001 : seed;
	const mix = (i, r) => { let x = (Math.imul(i, 0x9E3779B9) + seed + Math.imul(r, 0x85EBCA6B)) >>> 0; x ^= x >>> 16; x = Math.imul(x, 0x7FEB352D) >>> 0; x ^= x >>> 15; x = Math.imul(x, 0x846CA68B) >>> 0; x ^= x >>> 16; return x >>> 0; };
	const out = new Uint32Array(nWords);
	for (let i = 0; i < nWords; i++)
	{
		let w = mix(i, 0);
		for (let r = 1; r <= (andRounds || 0); r++) { w &= mix(i, r); }
		out[i] = w;
	}
	return out;
}

// The definition of ca3d_seed_state (include/ca3d.h) in executable form, twin of host.seeded_state: planes [z0, z0 + nz) of the state
// a device seed leaves. opts: {andRounds, box: {min: [x, y, z], max: [x, y, z]} (inclusive; default the whole grid), layout, z0, nz}.
// Packed: word (x >> 5) + y * cols + z * cols * G of the FULL grid is randomFill's word of that index, ANDed with the mask of its bits
// whose x lies in the box, 0 when y or z is outside; unpacked: one 0 / 1 word per cell, cut from the same packed words.
function seededState(gridSize, seed, opts)
{
	const o = opts || {};
	const G = gridSize, layout = o.layout || LAYOUT_PACKED32, rounds = o.andRounds || 0;
	if (layout === LAYOUT_PACKED32 ? (G <= 0 || G % 32) : (G <= 0 || G % 4)) { throw new RangeError("grid size " + G + " does not fit the layout"); }
	if (rounds < 0 || rounds > 31) { throw new RangeError("andRounds must be in [0, 31]"); }
	const z0 = o.z0 || 0, nz = o.nz === undefined ? G - z0 : o.nz;
	if (z0 < 0 || nz <= 0 || z0 + nz > G) { throw new RangeError("planes outside the grid"); }
	const lo = o.box ? o.box.min : [0, 0, 0], hi = o.box ? o.box.max : [G - 1, G - 1, G - 1];
	for (let i = 0; i < 3; i++) { if (lo[i] < 0 || lo[i] > hi[i] || hi[i] >= G) { throw new RangeError("the box does not lie in the grid"); } }
	seed = seed === undefined ? 0xCA3D0001 : seed;
	const mix = (i, r) => { let x = (Math.imul(i, 0x9E3779B9) + seed + Math.imul(r, 0x85EBCA6B)) >>> 0; x ^= x >>> 16; x = Math.imul(x, 0x7FEB352D) >>> 0; x ^= x >>> 15; x = Math.imul(x, 0x846CA68B) >>> 0; x ^= x >>> 16; return x >>> 0; };
	const cols = Math.ceil(G / 32);
	const packed = layout === LAYOUT_PACKED32;
	const out = new Uint32Array(packed ? cols * G * nz : G * G * nz);
	for (let z = z0; z < z0 + nz; z++)
	{
		if (z < lo[2] || z > hi[2]) { continue; }
		for (let y = lo[1]; y <= hi[1]; y++)
		{
			for (let xw = 0; xw < cols; xw++)
			{
				const a = Math.max(lo[0], 32 * xw), b = Math.min(hi[0], 32 * xw + 31);
				if (a > b) { continue; }
				const i = xw + y * cols + z * cols * G; // enters the hash modulo 2^32 (Math.imul)
				let w = mix(i, 0);
				for (let r = 1; r <= rounds; r++) { w &= mix(i, r); }
				w = (w & ((0xFFFFFFFF << (a & 31)) & (0xFFFFFFFF >>> (31 - (b & 31))))) >>> 0;
				if (packed) { out[xw + (y + (z - z0) * G) * cols] = w; }
				else { for (let x = a; x <= b; x++) { out[x + (y + (z - z0) * G) * G] = (w >>> (x & 31)) & 1; } }
			}
		}
	}
	return out;
}

// ca3d_seed as the addon takes it: seed, andRounds, boxMin x y z, boxMax x y z
function seedSpec(gridSize, spec)
{
	const s = spec || {};
	const lo = s.box ? s.box.min : [0, 0, 0], hi = s.box ? s.box.max : [gridSize - 1, gridSize - 1, gridSize - 1];
	return [(s.seed === undefined ? 0xCA3D0001 : s.seed) >>> 0, (s.andRounds || 0) >>> 0, lo[0] >>> 0, lo[1] >>> 0, lo[2] >>> 0, hi[0] >>> 0, hi[1] >>> 0, hi[2] >>> 0];
}

// Checkpoint file: 'CA3D' | u32 version | u32 grid | u32 layout | u64 step | u64 words | LE u32 words (host.py twin)
function saveCheckpoint(file, words, gridSize, step, layout)
{
	const fs = require("fs");
	const head = Buffer.alloc(32);
	head.write("CA3D", 0, "latin1");
	head.writeUInt32LE(1, 4); head.writeUInt32LE(gridSize, 8); head.writeUInt32LE(layout || 0, 12);
	head.writeBigUInt64LE(BigInt(step || 0), 16); head.writeBigUInt64LE(BigInt(words.length), 24);
	fs.writeFileSync(file, Buffer.concat([head, Buffer.from(words.buffer, words.byteOffset, words.byteLength)]));
}

function loadCheckpoint(file)
{
	const fs = require("fs");
	const b = fs.readFileSync(file);
	if (b.length < 32 || b.toString("latin1", 0, 4) !== "CA3D" || b.readUInt32LE(4) !== 1) { throw new Error("not a CA3D checkpoint"); }
	const gridSize = b.readUInt32LE(8), layout = b.readUInt32LE(12), step = Number(b.readBigUInt64LE(16)), n = Number(b.readBigUInt64LE(24));
	if (b.length !== 32 + 4 * n) { throw new Error("truncated checkpoint"); }
	const words = new Uint32Array(n);
	Buffer.from(words.buffer).set(b.subarray(32));
	return { words, gridSize, layout, step };
}

let addon = null;
function loadAddon()
{
	if (!addon)
	{
		try { addon = require(path.join(__dirname, "ca3d_napi.node")); }
		catch (e) { throw new Error("ca3d_napi.node is missing or unloadable (build: make -C cellularautomatons3d_amd/js/addon): " + e.message + " — this engine has no CPU fallback"); }
	}
	return addon;
}

const STOP_EXTINCT = 1, STOP_STILL = 2; // ca3d_step_until: bits of `reason`
const STOP_PERIODIC = 4; // ... and of ca3d_step_until_cycle / ca3d_ensemble_step_until_cycle, which alone take it
const STOP_MOVING = 8; // ... and of ca3d_ensemble_step_until_moving (Ensemble.stepUntilMoving), which alone takes it

const ISOLATE_PLACEMENTS = ["keep", "centre", "origin"]; // index = CA3D_ISOLATE_KEEP / CENTRE / ORIGIN (Ensemble.isolate)
const ISOLATE_COPY_RULES = 0x100;
const COMPOSE_OVER = 0x1, COMPOSE_COPY_RULES = 0x100; // CA3D_COMPOSE_OVER / CA3D_COMPOSE_COPY_RULES (Ensemble.compose)
const CANON_CLOSED = 0x1, CANON_MAX_PERIOD = 4096; // CA3D_CANON_CLOSED / CA3D_CANON_MAX_PERIOD (Ensemble.canonPeriod)
// CA3D_ENVELOPE_RETURNS, the image bits in the order the images are written, CA3D_ENVELOPE_COPY_RULES (Ensemble.envelope)
const ENVELOPE_RETURNS = 0x1, ENVELOPE_IMAGES = { envelope: 1, stator: 2, rotor: 4 }, ENVELOPE_COPY_RULES = 0x100;
// CA3D_DAMAGE_HEALED, CA3D_DAMAGE_FLIPS, CA3D_DAMAGE_SELF = CA3D_DAMAGE_NO_FLIP, CA3D_DAMAGE_IMAGE_DAMAGE, CA3D_DAMAGE_COPY_RULES (Ensemble.damage)
const DAMAGE_HEALED = 0x1, DAMAGE_FLIPS = 4, DAMAGE_NONE = 0xFFFFFFFF, DAMAGE_IMAGE_DAMAGE = 0x1, DAMAGE_COPY_RULES = 0x100;

const STAMP_MODES = ["or", "replace", "erase"]; // index = CA3D_STAMP_OR / REPLACE / ERASE (Engine.stampWindows)

// [[universe, [x, y, z]], ...] (or the flat Uint32Array itself) as ca3d_window records: universe, x, y, z a window
function flatWindows(windows)
{
	if (windows instanceof Uint32Array) return windows;
	return Uint32Array.from(windows.flatMap(([universe, origin]) =>
	{
		if (!origin || origin.length !== 3) throw new RangeError("windows: [universe, [x, y, z]] each");
		return [universe, origin[0], origin[1], origin[2]];
	}));
}

// the origins [x, y, z] of ceil(G / 64)^3 windows that tile a grid of G, x fastest (every cell exactly once when 64 divides G)
function windowTiling(gridSize)
{
	if (gridSize < 64) throw new RangeError("a window is 64^3 cells: the grid must be 64 or more a side");
	const n = Math.ceil(gridSize / 64), out = [];
	for (let z = 0; z < n; z++) for (let y = 0; y < n; y++) for (let x = 0; x < n; x++) out.push([64 * x, 64 * y, 64 * z]);
	return out;
}

class Engine
{
	constructor(device)
	{
		this._a = loadAddon();
		this._h = this._a.create(device || 0);
		this.gridSize = 0;
	}

	// An asynchronous job holds the engine on a worker thread until its promise settles: nothing else may enter the engine
	// meanwhile (it is not thread-safe), and it must not be destroyed under the worker.
	_idle(what)
	{
		if (this._inflight) { throw new Error("ca3d: " + what + "() while an asynchronous call is pending on this engine — await it first"); }
	}
	close() { this._idle("close"); if (this._h) { this._a.destroy(this._h); this._h = null; } }
	/** close() once every asynchronous call issued so far has settled. */
	closeAsync() { return (this._pending || Promise.resolve()).then(() => this.close()); }

	configure(gridSize, layout) { this._idle("configure"); this._a.configure(this._h, gridSize, layout || LAYOUT_PACKED32); this.gridSize = gridSize; }

	setRules(mainOffsets, edgesOffsets, cornersOffsets, survive, born) { this._idle("setRules"); this._a.setRules(this._h, mainOffsets, edgesOffsets, cornersOffsets, survive, born); }

	setRuleStrings(rules)
	{
		const r = Object.assign({}, DEFAULT_RULES, rules || {});
		const lut = recalculateRulesValues(r);
		this.setRules(NEIGHBOURHOOD_MAP[r.neighbourhood], NEIGHBOURHOOD_MAP["edges"], NEIGHBOURHOOD_MAP["corners"], lut.survive, lut.born);
	}

	// _restartSim (624-637)
	restartSim(gridSize, rules, randomInitialState, random)
	{
		this.configure(gridSize);
		this.setRuleStrings(rules);
		this.uploadState(initialState(gridSize, randomInitialState, random));
	}

	uploadState(words) { this._idle("uploadState"); this._a.uploadState(this._h, words); }

	// ca3d_seed_state: the state seededState(gridSize, seed, {andRounds, box, layout}) written on the device into both buffers — nothing is
	// uploaded. Replaces the state as uploadState does; only enqueues. spec: {seed, andRounds, box: {min: [x, y, z], max: [x, y, z]}}
	seedState(spec) { this._idle("seedState"); this._a.seedState(this._h, Uint32Array.from(seedSpec(this.gridSize, spec))); }

	readState()
	{
		this._idle("readState");
		const out = new Uint32Array(this.info().stateWords);
		this._a.readState(this._h, out);
		return out;
	}

	// _computePass (1796-1809), n times
	step(n) { this._idle("step"); this._a.step(this._h, n === undefined ? 1 : n); }
	/** device.queue.submit: submits the steps encoded under setOption("queue", n). */
	flush() { this._idle("flush"); this._a.flush(this._h); }

	/** Windows (ca3d_cut_windows): universe u of the Ensemble `ens` becomes the 64^3 window of this engine's current state whose cell
	 *  (0, 0, 0) is grid cell (x, y, z), for every [u, [x, y, z]] of `windows` (or a Uint32Array of u, x, y, z a window) — the grid is
	 *  a torus, a window may wrap. On the device, one launch behind every step asked for so far; the universes are at step 0
	 *  afterwards, rules untouched, and must be distinct. windowTiling(gridSize) gives the origins that cover the grid -> gpuMs. */
	cutWindows(ens, windows) { this._idle("cutWindows"); return this._a.cutWindows(this._h, ens._e, flatWindows(windows)); }
	/** ca3d_stamp_windows: universe u of `ens` is stamped into this engine's state with its cell (0, 0, 0) at (x, y, z). mode: "or" (the
	 *  default) sets the universe's live cells, "erase" clears them, "replace" first clears every window's 64^3 box and then sets;
	 *  windows may overlap and their order does not matter. The step counter stays, the next summary has no previous state, the next
	 *  frame rebuilds what it derives from the state; an engine that was only configured counts as empty -> gpuMs. */
	stampWindows(ens, windows, mode)
	{
		this._idle("stampWindows");
		const m = STAMP_MODES.indexOf(mode === undefined ? "or" : mode);
		if (m < 0) throw new Error(`unknown mode ${JSON.stringify(mode)}: "or", "replace" or "erase"`);
		return this._a.stampWindows(this._h, ens._e, flatWindows(windows), m);
	}

	// Z-slab mode (multi-GPU hosts; SURVEY 8(e)): see include/ca3d.h. phase: 0 whole batch, 1 edge zones, 2 interior.
	configureSlab(gridSize, z0, nz, ghost, layout) { this._a.configureSlab(this._h, gridSize, layout === undefined ? LAYOUT_PACKED32 : layout, z0, nz, ghost); this.gridSize = gridSize; }
	slabStep(n) { this._a.slabStep(this._h, n); }
	slabStepPhase(n, phase) { this._a.slabStepPhase(this._h, n, phase); }
	// RCCL transport inside the engine: one process per GPU; rank 0 creates the id (Engine.commUniqueId()) and hands it to
	// the other ranks by the host's own IPC; slabRun(n, overlap) = n steps with the ghost planes exchanged between batches
	static commUniqueId() { return loadAddon().commUniqueId(); }
	slabCommInit(id, rank, world) { this._a.slabCommInit(this._h, id, rank, world); }
	slabRun(n, overlap) { this._a.slabRun(this._h, n, overlap ? 1 : 0); }
	slabExchange() { this._a.slabExchange(this._h); }
	slabGather(full) { this._a.slabGather(this._h, full._h); }

	synchronize() { this._idle("synchronize"); this._a.synchronize(this._h); }

	// _renderPass (1775-1794) with the reference's 128-float block (MemoryManager.bufferf32)
	render(uniforms, width, height, spp, targets)
	{
		const t = targets || {};
		this._idle("render");
		this._a.render(this._h, uniforms, width, height, spp || 1, t.presentation || null, t.light || null, t.depth || null);
	}

	// Asynchronous forms (napi_async_work): the wait for the GPU runs on a worker thread and the call returns a Promise, so
	// a UI thread never blocks in a read-back. The engine takes one call at a time: do not call anything else on it until
	// the promise has settled (asynchronous calls issued meanwhile queue up behind it by themselves).
	_queue(start)
	{
		this._inflight = (this._inflight || 0) + 1;
		const done = () => { this._inflight--; };
		const run = () => { const inflight = this._inflight; this._inflight = 0; try { return start(); } finally { this._inflight = inflight; } };
		const p = (this._pending || Promise.resolve()).then(run, run);
		this._pending = p.then(done, done);
		return p;
	}
	readStateAsync()
	{
		return this._queue(() => {
			const out = new Uint32Array(this.info().stateWords);
			return this._a.readStateAsync(this._h, out).then(() => out);
		});
	}
	renderAsync(uniforms, width, height, spp, targets)
	{
		const t = targets || {};
		return this._queue(() => this._a.renderAsync(this._h, uniforms, width, height, spp || 1, t.presentation || null, t.light || null, t.depth || null).then(() => t));
	}
	synchronizeAsync() { return this._queue(() => this._a.synchronizeAsync(this._h)); }

	// ca3d_summarize (no reference counterpart): population, births / deaths against the state one step earlier, bounding box and
	// digest of the current state, computed on the device. -> {step, population, births, deaths, digest (BigInt), hasPrevious,
	// boxMin [x, y, z], boxMax, planePopulation? (Uint32Array, one entry per owned z plane, with {planes: true})}
	summary(opts)
	{
		this._idle("summary");
		const planes = opts && opts.planes ? new Uint32Array(this._a.info(this._h).nz) : null;
		return this._a.summary(this._h, planes);
	}
	// ca3d_step_until: steps in batches of checkEvery (default 8) until the grid is empty (extinct, default true) or a fixed point
	// (still, default true), at most maxSteps steps; the batches and their waits run on a worker thread.
	// -> Promise<{stepsDone, reason (STOP_EXTINCT | STOP_STILL bits; 0: maxSteps reached), summary}>
	stepUntil(maxSteps, opts)
	{
		const o = Object.assign({ checkEvery: 8, extinct: true, still: true }, opts || {});
		const mask = (o.extinct ? STOP_EXTINCT : 0) | (o.still ? STOP_STILL : 0);
		return this._queue(() => this._a.stepUntilAsync(this._h, maxSteps, o.checkEvery, mask));
	}
	// ca3d_step_until_cycle: stepUntil with a third condition (periodic, default true) — the state at a check point equals, bit for bit,
	// the state at an earlier check point of this call. period: the steps between the two (a multiple of the true period, the least
	// period itself with checkEvery 1), 0 unless STOP_PERIODIC is in reason.
	// -> Promise<{stepsDone, reason (STOP_EXTINCT | STOP_STILL | STOP_PERIODIC bits; 0: maxSteps reached), period, summary}>
	stepUntilCycle(maxSteps, opts)
	{
		const o = Object.assign({ checkEvery: 8, extinct: true, still: true, periodic: true }, opts || {});
		const mask = (o.extinct ? STOP_EXTINCT : 0) | (o.still ? STOP_STILL : 0) | (o.periodic ? STOP_PERIODIC : 0);
		return this._queue(() => this._a.stepUntilCycleAsync(this._h, maxSteps, o.checkEvery, mask));
	}

	info() { this._idle("info"); return this._a.info(this._h); }
	stats() { this._idle("stats"); return this._a.stats(this._h); }
	renderStats() { this._idle("renderStats"); return this._a.renderStats(this._h); }
	renderPipeline() { this._idle("renderPipeline"); return this._a.renderPipeline(this._h); } // converged frames in flight (option render_pipeline)
	setOption(name, value) { this._idle("setOption"); this._a.setOption(this._h, name, value); }
	/** resident launches that timed out and were re-run through the per-step kernels (include/ca3d.h) */
	recoveredLaunches() { this._idle("recoveredLaunches"); return this._a.recoveredLaunches(this._h); }
}

// ca3d_group_*: the Z-slab split of a grid over the GPUs of a node, driven by this one JavaScript thread (the reference's host
// is one thread that enqueues everything, main_pathtraced.js:1821-1854). `devices`: one GPU index per slab, in z order; the
// same index may repeat (several slabs on one GPU). Same rule / state / step / render surface as Engine, on the FULL grid.
class EngineGroup
{
	constructor(devices)
	{
		this._a = loadAddon();
		this.devices = Int32Array.from(devices);
		this._g = this._a.groupCreate(this.devices);
		this.gridSize = 0;
	}
	close() { if (this._g) { this._a.groupDestroy(this._g); this._g = null; } }
	/** ghost = planes kept of each neighbour = steps between two exchanges */
	configure(gridSize, ghost, layout) { this._a.groupConfigure(this._g, gridSize, layout || LAYOUT_PACKED32, ghost); this.gridSize = gridSize; this.layout = layout || LAYOUT_PACKED32; }
	setRules(mainOffsets, edgesOffsets, cornersOffsets, survive, born) { this._a.groupSetRules(this._g, mainOffsets, edgesOffsets, cornersOffsets, survive, born); }
	setRuleStrings(rules)
	{
		const r = Object.assign({}, DEFAULT_RULES, rules || {});
		const lut = recalculateRulesValues(r);
		this.setRules(NEIGHBOURHOOD_MAP[r.neighbourhood], NEIGHBOURHOOD_MAP["edges"], NEIGHBOURHOOD_MAP["corners"], lut.survive, lut.born);
	}
	uploadState(words) { this._a.groupUploadState(this._g, words); this._words = words.length; }
	/** ca3d_group_seed_state: every rank seeds its own planes on its own device (spec as Engine.seedState) */
	seedState(spec)
	{
		this._a.groupSeedState(this._g, Uint32Array.from(seedSpec(this.gridSize, spec)));
		this._words = this.layout === LAYOUT_PACKED32 ? this.gridSize / 32 * this.gridSize * this.gridSize : this.gridSize ** 3;
	}
	readState() { const out = new Uint32Array(this._words); this._a.groupReadState(this._g, out); return out; }
	step(n) { this._a.groupStep(this._g, n === undefined ? 1 : n); }
	synchronize() { this._a.groupSynchronize(this._g); }
	/** "transport": 0 peer copies (default), 1 RCCL; any other option goes to every slab engine */
	setOption(name, value) { this._a.groupSetOption(this._g, name, value); }
	info(rank) { return this._a.groupInfo(this._g, rank || 0); }
	/** ca3d_group_summarize: Engine.summary() of the whole grid (every rank summarises its slab on its own device) */
	summary(opts) { return this._a.groupSummary(this._g, opts && opts.planes ? new Uint32Array(this.gridSize) : null); }
	render(uniforms, width, height, spp, targets)
	{
		const t = targets || {};
		this._a.groupRender(this._g, uniforms, width, height, spp || 1, t.presentation || null, t.light || null, t.depth || null);
	}
}

// ca3d_ensemble_*: `n` independent 64^3 universes (8192 packed words each) stepped side by side by one kernel launch, each with its
// own rule (a table pair of the ensemble's neighbourhood, von Neumann or Moore — or, clustered, three pairs), step counter, summary record and — in stepUntil — its
// own moment to stop (include/ca3d.h). Synchronous.
const ENSEMBLE_ALL = 0xFFFFFFFF, ENSEMBLE_WORDS = 8192;
const ENSEMBLE_NEIGHBOURHOODS = ["von neumann", "moore"]; // index = enum ca3d_ensemble_neighbourhood
const ENSEMBLE_BOUNDARIES = ["reference", "torus", "closed"]; // index = enum ca3d_ensemble_boundary
const CONNECTIVITIES = ["closed", "torus"]; // index = CA3D_CONNECT_CLOSED / TORUS (Ensemble.census, Ensemble.isolate)
// "closed", "torus", or "boundary": torus when `ensemble`'s boundary is "torus", closed otherwise -> CA3D_CONNECT_*
function connectivityOf(ensemble, name)
{
	if (name === undefined || name === null) return 0;
	if (name === "boundary") name = ensemble.boundary === "torus" ? "torus" : "closed";
	const c = CONNECTIVITIES.indexOf(name);
	if (c < 0) throw new Error(`unknown connectivity ${JSON.stringify(name)}: one of ${CONNECTIVITIES.join(", ")}, boundary`);
	return c;
}
class Ensemble
{
	constructor(device)
	{
		this._a = loadAddon();
		this._e = this._a.ensembleCreate(device || 0);
		this.n = 0;
	}
	close() { if (this._e) { this._a.ensembleDestroy(this._e); this._e = null; } }
	/** neighbourhood: "von neumann" (default) or "moore" — of every universe; the rules set afterwards must be of that kind.
	 *  clustered (Moore only): every universe carries edges and corners table pairs beside its main one
	 *  options.boundary: what setBoundary takes; a configure without it goes back to "reference" */
	configure(n, gridSize, neighbourhood, clustered = false, options = {})
	{
		const boundary = options.boundary === undefined ? "reference" : options.boundary;
		if (ENSEMBLE_BOUNDARIES.indexOf(boundary) < 0) throw new Error(`unknown ensemble boundary ${JSON.stringify(boundary)}: one of ${ENSEMBLE_BOUNDARIES.join(", ")}`);
		const nb = ENSEMBLE_NEIGHBOURHOODS.indexOf(neighbourhood === undefined ? "von neumann" : neighbourhood);
		if (nb < 0) throw new Error(`unknown ensemble neighbourhood ${JSON.stringify(neighbourhood)}: "von neumann" or "moore"`);
		if (clustered && ENSEMBLE_NEIGHBOURHOODS[nb] !== "moore") throw new Error(`a clustered ensemble's main list is Moore (got neighbourhood ${JSON.stringify(neighbourhood)})`);
		if (clustered) this._a.ensembleConfigureClustered(this._e, gridSize === undefined ? 64 : gridSize, n);
		else this._a.ensembleConfigureNeighbourhood(this._e, gridSize === undefined ? 64 : gridSize, n, nb);
		this.n = n;
		if (boundary !== "reference") this.setBoundary(boundary);
	}
	/** ca3d_ensemble_set_boundary: what the steps queued from now on see behind a universe's six faces — "reference" (- faces dead, + faces
	 *  wrap: the default), "torus" (all wrap) or "closed" (all dead). Moves nothing; canonPeriod is refused while it is not "reference" */
	setBoundary(name)
	{
		const b = ENSEMBLE_BOUNDARIES.indexOf(name);
		if (b < 0) throw new Error(`unknown ensemble boundary ${JSON.stringify(name)}: one of ${ENSEMBLE_BOUNDARIES.join(", ")}`);
		this._a.ensembleSetBoundary(this._e, b);
	}
	/** the boundary the next step runs under, as its string (throws before configure) */
	get boundary() { return ENSEMBLE_BOUNDARIES[this._a.ensembleBoundary(this._e)]; }
	/** the configured neighbourhood as its string (throws before configure) */
	get neighbourhood() { return ENSEMBLE_NEIGHBOURHOODS[this._a.ensembleNeighbourhood(this._e)]; }
	/** whether the ensemble was configured clustered (throws before configure) */
	get clustered() { return this._a.ensembleClustered(this._e) !== 0; }
	/** universe: an index, or ENSEMBLE_ALL */
	setRules(universe, mainOffsets, edgesOffsets, cornersOffsets, survive, born) { this._a.ensembleSetRules(this._e, universe, mainOffsets, edgesOffsets, cornersOffsets, survive, born); }
	setRuleStrings(universe, rules)
	{
		const r = Object.assign({}, DEFAULT_RULES, rules || {});
		const lut = recalculateRulesValues(r);
		this.setRules(universe, NEIGHBOURHOOD_MAP[r.neighbourhood], NEIGHBOURHOOD_MAP["edges"], NEIGHBOURHOOD_MAP["corners"], lut.survive, lut.born);
	}
	/** words: Uint32Array(count * 8192), the states of universes first .. first + count - 1 */
	uploadState(first, words) { this._a.ensembleUploadState(this._e, first, words); }
	/** ca3d_ensemble_seed_state: `specs` — ONE spec object ({seed, andRounds, box}) for `count` universes from `first` (default: all of
	 *  them), or an array with one spec per universe */
	seedStates(first, specs, count)
	{
		const list = Array.isArray(specs) ? specs : [specs];
		count = Array.isArray(specs) ? list.length : (count === undefined ? this.n - first : count);
		const words = new Uint32Array(8 * list.length);
		list.forEach((s, k) => words.set(seedSpec(64, s), 8 * k));
		this._a.ensembleSeedState(this._e, first, count, words);
	}
	/** ca3d_ensemble_set_rule_tables: rules as masks (bit c = born / survive at count c; c in 0..6, Moore ensembles 0..26), one pair per universe
	 *  from `first` (arrays), or one pair (numbers) for `count` universes (default: all from `first`) — one call, one copy */
	setRuleTables(first, bornMasks, surviveMasks, count)
	{
		const scalar = typeof bornMasks === "number";
		const b = Uint32Array.from(scalar ? [bornMasks] : bornMasks), s = Uint32Array.from(scalar ? [surviveMasks] : surviveMasks);
		this._a.ensembleSetRuleTables(this._e, first, scalar ? (count === undefined ? this.n - first : count) : b.length, b, s);
	}
	/** ca3d_ensemble_set_rule_tables_clustered: a rule is three masks [main (bits 0..26), edges (0..12), corners (0..8)]; arrays of such
	 *  triples: one rule per universe from `first`; two plain triples: that rule for `count` universes (default: all from `first`) */
	setClusteredTables(first, bornMasks, surviveMasks, count)
	{
		const one = typeof bornMasks[0] === "number";
		const flat = (m) => Uint32Array.from(one ? m : [].concat(...m.map((r) => Array.from(r))));
		const b = flat(bornMasks), s = flat(surviveMasks);
		this._a.ensembleSetClusteredTables(this._e, first, one ? (count === undefined ? this.n - first : count) : b.length / 3, b, s);
	}
	readState(first, count)
	{
		first = first || 0;
		const out = new Uint32Array((count === undefined ? this.n - first : count) * ENSEMBLE_WORDS);
		this._a.ensembleReadState(this._e, first, out);
		return out;
	}
	step(n) { this._a.ensembleStep(this._e, n === undefined ? 1 : n); }
	/** -> {stepsDone: Uint32Array(n), reason: Uint32Array(n)} (STOP_EXTINCT | STOP_STILL bits; 0: maxSteps reached) */
	stepUntil(maxSteps, opts)
	{
		const o = Object.assign({ checkEvery: 8, stopMask: STOP_EXTINCT | STOP_STILL }, opts || {});
		const stepsDone = new Uint32Array(this.n), reason = new Uint32Array(this.n);
		this._a.ensembleStepUntil(this._e, maxSteps, o.checkEvery, o.stopMask, stepsDone, reason);
		return { stepsDone, reason };
	}
	/** -> {stepsDone, reason, period: Uint32Array(n) each} (reason: + STOP_PERIODIC; period[u]: 0 unless STOP_PERIODIC is in reason[u]) */
	stepUntilCycle(maxSteps, opts)
	{
		const o = Object.assign({ checkEvery: 8, stopMask: STOP_EXTINCT | STOP_STILL | STOP_PERIODIC }, opts || {});
		const stepsDone = new Uint32Array(this.n), reason = new Uint32Array(this.n), period = new Uint32Array(this.n);
		this._a.ensembleStepUntilCycle(this._e, maxSteps, o.checkEvery, o.stopMask, stepsDone, reason, period);
		return { stepsDone, reason, period };
	}
	/** stepUntilCycle that also stops a universe whose state at a check point is its anchor state translated by a vector d != 0, both clear
	 *  of the faces (ca3d_ensemble_step_until_moving): a glider or spaceship, decided inside the kernel and exact
	 *  -> {stepsDone, reason, period: Uint32Array(n) each, shift: Int32Array(3 n)} (reason: + STOP_MOVING; shift[3 u ..]: dx, dy, dz over
	 *  period[u], zero unless STOP_MOVING is in reason[u]) */
	stepUntilMoving(maxSteps, opts)
	{
		const o = Object.assign({ checkEvery: 8, stopMask: STOP_EXTINCT | STOP_STILL | STOP_PERIODIC | STOP_MOVING }, opts || {});
		const stepsDone = new Uint32Array(this.n), reason = new Uint32Array(this.n), period = new Uint32Array(this.n), shift = new Int32Array(3 * this.n);
		this._a.ensembleStepUntilMoving(this._e, maxSteps, o.checkEvery, o.stopMask, stepsDone, reason, period, shift);
		return { stepsDone, reason, period, shift };
	}
	/** stepUntil that records every universe's population curve inside the kernel: one sample (population, births, deaths) per check
	 *  point -> {samples: Uint32Array(n * samplesPerUniverse * 3), samplesPerUniverse, nSamples, stepsDone, reason}; sample j of universe u
	 *  starts at samples[(u * samplesPerUniverse + j) * 3], slots past nSamples[u] are zero. stopMask: STOP_EXTINCT | STOP_STILL bits;
	 *  0 (the default): nothing stops and every universe has samplesPerUniverse samples. */
	stepTrace(maxSteps, checkEvery, stopMask)
	{
		checkEvery = checkEvery === undefined ? 8 : checkEvery;
		// (checkEvery 0: no K to size the array with — the library names the error)
		const samplesPerUniverse = checkEvery >= 1 ? traceSamples(maxSteps, checkEvery) : 1;
		const samples = new Uint32Array(this.n * samplesPerUniverse * 3);
		const nSamples = new Uint32Array(this.n), stepsDone = new Uint32Array(this.n), reason = new Uint32Array(this.n);
		this._a.ensembleStepUntilTrace(this._e, maxSteps, checkEvery, stopMask || 0, stepsDone, reason, samples, samplesPerUniverse, nSamples);
		return { samples, samplesPerUniverse, nSamples, stepsDone, reason };
	}
	/** the universes' records, as Engine.summary() objects without planePopulation */
	summaries(first, count) { first = first || 0; return this._a.ensembleSummaries(this._e, first, count === undefined ? this.n - first : count); }
	/** The census (ca3d_ensemble_census): the connected objects — 26-neighbourhood inside the closed cube, no face wraps — of universes
	 *  first .. first + count - 1 (default: all from `first`), found on the device in one launch behind the queued steps
	 *  -> {components, nComponents: Uint32Array(count), remaining: Uint32Array(count), gpuMs}. components[k] lists universe first + k's
	 *  first min(C, maxComponents) objects in the order of their first cells, each {population, firstCell (x + 64 y + 4096 z), boxMin
	 *  [x, y, z], boxMax, digest (BigInt: the state digest of the object translated to the origin)}; remaining[k]: live cells in no
	 *  listed object, 0 when the list is complete. maxComponents: 1 .. 1024, default 64. The call only reads.
	 *  opts.connectivity (ca3d_ensemble_census_connected): "closed" (the default), "torus" — cells are adjacent modulo 64, an object on a
	 *  face is one object, boxMin starts its cyclic box and boxMax = boxMin + extent - 1 is not reduced (>= 64 through a seam) — or
	 *  "boundary": torus when this ensemble's boundary is "torus", closed otherwise. */
	census(first, count, maxComponents, opts)
	{
		const connectivity = connectivityOf(this, (opts || {}).connectivity);
		first = first || 0;
		count = count === undefined ? this.n - first : count;
		maxComponents = maxComponents === undefined ? 64 : maxComponents;
		// (a size the library refuses gets no arrays: it names the reason)
		const sizable = count > 0 && maxComponents >= 1 && maxComponents <= 1024;
		const words = new Uint32Array(sizable ? count * maxComponents * 8 : 0);
		const nComponents = new Uint32Array(sizable ? count : 0), remaining = new Uint32Array(sizable ? count : 0);
		const gpuMs = this._a.ensembleCensus(this._e, first, count, maxComponents, words, nComponents, remaining, connectivity);
		const box = (w) => [w & 0xFF, (w >>> 8) & 0xFF, (w >>> 16) & 0xFF];
		const components = [];
		for (let k = 0; k < count; k++)
		{
			const list = [];
			for (let i = 0; i < nComponents[k]; i++)
			{
				const r = words.subarray((k * maxComponents + i) * 8, (k * maxComponents + i) * 8 + 8);
				list.push({ population: r[0], firstCell: r[1], boxMin: box(r[2]), boxMax: box(r[3]), digest: BigInt(r[5]) << 32n | BigInt(r[4]) });
			}
			components.push(list);
		}
		return { components, nComponents, remaining, gpuMs };
	}
	/** Isolate (ca3d_ensemble_isolate): universe dstFirst + k of THIS ensemble becomes the connected object of universe jobs[k][0] of
	 *  opts.src (default: this ensemble) that holds the cell jobs[k][1] (x + 64 y + 4096 z, any cell of the object — a census' firstCell
	 *  will do), alone, translated as opts.placement says ("keep", "centre" — the default —, "origin"), at step 0, found and written on
	 *  the device in one launch -> {population: Uint32Array(n), shift: Int32Array(3 n) (dx, dy, dz a job), gpuMs}. opts.copyRules
	 *  (default true): the destination universe takes its source universe's rule (both ensembles of one kind). opts.dstFirst: 0.
	 *  jobs: an array of [universe, cell] pairs, or a Uint32Array of such pairs. opts.connectivity (ca3d_ensemble_isolate_connected):
	 *  "closed" (the default), "torus" — the object is the torus census', moved modulo 64 so that it arrives in one piece — or
	 *  "boundary": torus when the source ensemble's boundary is "torus", closed otherwise. */
	isolate(jobs, opts)
	{
		const o = Object.assign({ dstFirst: 0, src: null, placement: "centre", copyRules: true, connectivity: "closed" }, opts || {});
		const connectivity = connectivityOf(o.src || this, o.connectivity);
		const placement = ISOLATE_PLACEMENTS.indexOf(o.placement);
		if (placement < 0) throw new Error(`unknown placement ${JSON.stringify(o.placement)}: "keep", "centre" or "origin"`);
		const flat = jobs instanceof Uint32Array ? jobs : Uint32Array.from(jobs.flat());
		if (flat.length % 2) throw new RangeError("jobs: [universe, cell] pairs");
		const n = flat.length / 2;
		const out = new Int32Array(4 * n);
		const gpuMs = this._a.ensembleIsolate(this._e, o.dstFirst, (o.src || this)._e, flat, placement | (o.copyRules ? ISOLATE_COPY_RULES : 0), out, connectivity);
		const population = new Uint32Array(n), shift = new Int32Array(3 * n);
		for (let k = 0; k < n; k++)
		{
			population[k] = out[4 * k];
			shift.set(out.subarray(4 * k + 1, 4 * k + 4), 3 * k);
		}
		return { population, shift, gpuMs };
	}
	/** Compose (ca3d_ensemble_compose), the inverse of isolate: universe dstFirst + k of THIS ensemble becomes the union of the pieces
	 *  layouts[k], an array of [universe, orientation, [x, y, z]]: the WHOLE state of that universe of opts.src (default: this ensemble),
	 *  turned by orientation 0 .. 47 (perm = PERMS[o % 6], bit i of floor(o / 6) mirrors output axis i) with the turned piece's boxMin
	 *  put at [x, y, z], -64 .. 64 each; cells that leave the cube are clipped. opts.over (default false): on top of the destination's
	 *  current state; opts.copyRules (default true): a destination takes the rule of its first piece's universe (both ensembles of one
	 *  kind); opts.dstFirst: 0. One launch for all destinations, at step 0
	 *  -> {population, placed, overlap, clipped: Uint32Array(n) each, gpuMs}. */
	compose(layouts, opts)
	{
		const o = Object.assign({ dstFirst: 0, src: null, over: false, copyRules: true }, opts || {});
		const n = layouts.length;
		const begin = new Uint32Array(n + 1);
		const flat = [];
		layouts.forEach((layout, k) =>
		{
			for (const part of layout)
			{
				if (!Array.isArray(part) || part.length !== 3 || part[2].length !== 3) throw new RangeError("a part is [universe, orientation, [x, y, z]]");
				flat.push(part[0], part[1], part[2][0], part[2][1], part[2][2], 0);
			}
			begin[k + 1] = flat.length / 6;
		});
		const out = new Uint32Array(4 * n);
		const gpuMs = this._a.ensembleCompose(this._e, o.dstFirst, (o.src || this)._e, Int32Array.from(flat), begin,
			(o.over ? COMPOSE_OVER : 0) | (o.copyRules ? COMPOSE_COPY_RULES : 0), out);
		const r = { population: new Uint32Array(n), placed: new Uint32Array(n), overlap: new Uint32Array(n), clipped: new Uint32Array(n), gpuMs };
		for (let k = 0; k < n; k++) { r.population[k] = out[4 * k]; r.placed[k] = out[4 * k + 1]; r.overlap[k] = out[4 * k + 2]; r.clipped[k] = out[4 * k + 3]; }
		return r;
	}
	/** Canon (ca3d_ensemble_canon): the name of universes opts.first .. opts.first + opts.count - 1 (default: all from `first`) up to the
	 *  48 orientations of compose and any translation, found on the device in one launch behind the queued steps
	 *  -> {records, gpuMs}, records[k] = {key (BigInt: equal for all turned and shifted copies of a state), symmetry (BigInt: bit o set
	 *  when turning by o leaves the state as it is), orientation (which turns the state into the one whose digest is the key),
	 *  population, boxMin [x, y, z], boxMax}; with opts.digests also digests[k], an array of 48 BigInt, the digest of every
	 *  orientation. The WHOLE state of a universe is named: isolate objects first. The call only reads. */
	canon(opts)
	{
		const o = Object.assign({ first: 0, digests: false }, opts || {});
		const count = o.count === undefined ? this.n - o.first : o.count;
		// (a count the library refuses gets no arrays: it names the reason)
		const words = new Uint32Array(count > 0 ? count * 8 : 0);
		const dwords = o.digests ? new Uint32Array(count > 0 ? count * 96 : 0) : null;
		const gpuMs = this._a.ensembleCanon(this._e, o.first, count, words, dwords);
		const box = (w) => [w & 0xFF, (w >>> 8) & 0xFF, (w >>> 16) & 0xFF];
		const big = (a, i) => BigInt(a[i + 1]) << 32n | BigInt(a[i]);
		const records = [], digests = [];
		for (let k = 0; k < count; k++)
		{
			const r = words.subarray(8 * k, 8 * k + 8);
			records.push({ key: big(r, 0), symmetry: big(r, 2), orientation: r[4], population: r[5], boxMin: box(r[6]), boxMax: box(r[7]) });
			if (dwords) digests.push(Array.from({ length: 48 }, (_, i) => big(dwords, 96 * k + 2 * i)));
		}
		return dwords ? { records, digests, gpuMs } : { records, gpuMs };
	}
	/** Canon over a period (ca3d_ensemble_canon_period): universe opts.first + k named over opts.periods[k] steps of its own, taken INSIDE
	 *  one launch behind the queued steps; the ensemble is left exactly as it is. opts.periods: one number for universes opts.first ..
	 *  opts.first + opts.count - 1 (default: all from `first`), or an array with one period per universe of the range, each 1 .. 4096
	 *  -> {records, gpuMs}, records[k] = {key (BigInt: the smallest canon key over the phases t = 0 .. period - 1; all phases of all
	 *  48 turned copies of a glider share it), symmetry (BigInt), orientation, phase (the smallest t that reaches the key),
	 *  population (of that phase), closed (after `period` steps the state is back up to a translation, compared word for word: the
	 *  period is a multiple of the true one), shift [dx, dy, dz] (that translation: all 0 for an oscillator or a still life)}; with
	 *  opts.keys also keys[k], an array of periods[k] BigInt, the key of every phase. Every universe of the range needs a rule. */
	canonPeriod(opts)
	{
		const o = Object.assign({ first: 0, keys: false }, opts || {});
		const scalar = typeof o.periods === "number";
		const count = scalar ? (o.count === undefined ? this.n - o.first : o.count) : o.periods.length;
		const periods = scalar ? new Uint32Array(count > 0 ? count : 0).fill(o.periods) : Uint32Array.from(o.periods);
		// (a period the library refuses sizes no array: it names the reason)
		const longest = periods.reduce((m, p) => Math.max(m, p), 0), stride = longest <= CANON_MAX_PERIOD ? longest : 0;
		const words = new Uint32Array(periods.length * 8);
		const kwords = o.keys ? new Uint32Array(periods.length * stride * 2) : null;
		const gpuMs = this._a.ensembleCanonPeriod(this._e, o.first, periods, words, kwords, stride);
		const big = (a, i) => BigInt(a[i + 1]) << 32n | BigInt(a[i]);
		const byte = (w, s) => ((w >>> s & 0xFF) ^ 0x80) - 0x80;
		const records = [], keys = [];
		for (let k = 0; k < periods.length; k++)
		{
			const r = words.subarray(8 * k, 8 * k + 8);
			records.push({ key: big(r, 0), symmetry: big(r, 2), orientation: r[4], phase: r[5], population: r[6], closed: (r[7] & CANON_CLOSED) !== 0,
				shift: [byte(r[7], 8), byte(r[7], 16), byte(r[7], 24)] });
			if (kwords) keys.push(Array.from({ length: periods[k] }, (_, t) => big(kwords, 2 * (stride * k + t))));
		}
		return kwords ? { records, keys, gpuMs } : { records, gpuMs };
	}
	/** Envelope over a period (ca3d_ensemble_envelope): HOW universe opts.first + k oscillates over periods[k] steps of its own, taken
	 *  INSIDE one launch behind the queued steps under this ensemble's rule and boundary; this ensemble is left exactly as it is.
	 *  periods: one number for every universe from opts.first on, or an array with one period per universe, each 1 .. 4096
	 *  -> {records, gpuMs}, records[k] = {period, returns (after `period` steps the state is back word for word), heat (cells changed,
	 *  summed over the steps), populationSum, envelopePopulation (cells that ever live), statorPopulation (cells that always live),
	 *  rotorPopulation, envelopeMin, envelopeMax, rotorMin, rotorMax ([x, y, z], inclusive; zeros for an empty set)}.
	 *  opts.images: any of "envelope", "stator", "rotor"; with n of them universe opts.dstFirst + k n + i of opts.dst (this ensemble
	 *  or another one on the same device; required with images) becomes the i-th of them, in that order, at step 0. opts.copyRules
	 *  (default false): each destination takes its source universe's rule (both ensembles of one kind). */
	envelope(periods, opts)
	{
		const o = Object.assign({ first: 0, dst: null, dstFirst: 0, images: [], copyRules: false }, opts || {});
		const count = Math.max(this.n - o.first, 0);
		const p = typeof periods === "number" ? new Uint32Array(count).fill(periods) : Uint32Array.from(periods);
		let flags = o.copyRules ? ENVELOPE_COPY_RULES : 0;
		for (const name of o.images)
		{
			if (!(name in ENVELOPE_IMAGES)) throw new Error(`unknown image ${JSON.stringify(name)}: "envelope", "stator" or "rotor"`);
			flags |= ENVELOPE_IMAGES[name];
		}
		const words = new Uint32Array(p.length * 12);
		const gpuMs = this._a.ensembleEnvelope(this._e, o.first, p, o.dst ? o.dst._e : null, o.dstFirst, flags, words);
		const box = (w) => [w & 0xFF, (w >>> 8) & 0xFF, (w >>> 16) & 0xFF];
		const records = [];
		for (let k = 0; k < p.length; k++)
		{
			const r = words.subarray(12 * k, 12 * k + 12);
			records.push({ period: r[0], returns: (r[1] & ENVELOPE_RETURNS) !== 0, heat: r[2], populationSum: r[3], envelopePopulation: r[4],
				statorPopulation: r[5], rotorPopulation: r[4] - r[5], envelopeMin: box(r[6]), envelopeMax: box(r[7]), rotorMin: box(r[8]), rotorMax: box(r[9]) });
		}
		return { records, gpuMs };
	}
	/** Damage spreading (ca3d_ensemble_damage): how a perturbation of universe opts.first + k spreads over steps[k] steps — the universe
	 *  and a perturbed twin stepped side by side INSIDE one launch behind the queued steps, under the universe's rule and this ensemble's
	 *  boundary, their Hamming distance d_t taken at every t = 0 .. steps[k]; this ensemble is left exactly as it is.
	 *  steps: one number for every universe from opts.first on, or an array with one step count per universe, each 1 .. 4096
	 *  -> {records, gpuMs} and, with opts.curve, curve: records[k] = {steps, healed, healedAt (the first t with d_t = 0, null if none),
	 *  finalDistance, initialDistance, maxDistance, maxAt, distanceSum, damageMin, damageMax (the box of the last difference),
	 *  touchedMin, touchedMax (the box of every difference; [x, y, z], inclusive; zeros for an empty set)}; curve[k] = Uint32Array of
	 *  d_0 .. d_steps[k].
	 *  opts.twins: per universe the universe of this ensemble the twin starts from, null for the universe itself (the default for all);
	 *  opts.flips: per universe up to four cells [x, y, z] flipped in the twin, a cell listed twice cancels. opts.image: universe
	 *  opts.dstFirst + k of opts.dst (this ensemble or another one on the same device; required with the image) becomes the last
	 *  difference, at step 0. opts.copyRules (default false): each destination takes its source universe's rule (both ensembles of
	 *  one kind). */
	damage(steps, opts)
	{
		const o = Object.assign({ first: 0, twins: null, flips: null, dst: null, dstFirst: 0, image: false, copyRules: false, curve: false }, opts || {});
		const count = Math.max(this.n - o.first, 0);
		const p = typeof steps === "number" ? new Uint32Array(count).fill(steps) : Uint32Array.from(steps);
		const twins = o.twins ? Uint32Array.from(o.twins, (u) => (u === null || u === undefined ? DAMAGE_NONE : u)) : null;
		let flips = null;
		if (o.flips)
		{
			if (o.flips.length !== p.length) throw new Error(`flips for ${o.flips.length} universes, steps for ${p.length}`);
			flips = new Uint32Array(p.length * DAMAGE_FLIPS).fill(DAMAGE_NONE);
			o.flips.forEach((cells, k) =>
			{
				if (cells.length > DAMAGE_FLIPS) throw new Error(`universe ${o.first + k}: ${cells.length} flips, at most ${DAMAGE_FLIPS}`);
				cells.forEach(([x, y, z], i) =>
				{
					if (![x, y, z].every((v) => Number.isInteger(v) && v >= 0 && v < 64)) throw new Error(`a flipped cell lies inside the 64^3 universe, not at ${[x, y, z]}`);
					flips[k * DAMAGE_FLIPS + i] = (x | y << 8 | z << 16) >>> 0;
				});
			});
		}
		const flags = (o.image ? DAMAGE_IMAGE_DAMAGE : 0) | (o.copyRules ? DAMAGE_COPY_RULES : 0);
		const stride = o.curve && p.length ? p.reduce((a, b) => Math.max(a, b), 0) + 1 : 0;
		const samples = o.curve ? new Uint32Array(p.length * stride) : null;
		const words = new Uint32Array(p.length * 12);
		const gpuMs = this._a.ensembleDamage(this._e, o.first, p, twins, flips, o.dst ? o.dst._e : null, o.dstFirst, flags, words, samples, stride);
		const box = (w) => [w & 0xFF, (w >>> 8) & 0xFF, (w >>> 16) & 0xFF];
		const records = [];
		for (let k = 0; k < p.length; k++)
		{
			const r = words.subarray(12 * k, 12 * k + 12);
			records.push({ steps: r[0], healed: (r[1] & DAMAGE_HEALED) !== 0, healedAt: r[1] & DAMAGE_HEALED ? r[2] : null, finalDistance: r[3], initialDistance: r[4],
				maxDistance: r[5], maxAt: r[6], distanceSum: r[7], damageMin: box(r[8]), damageMax: box(r[9]), touchedMin: box(r[10]), touchedMax: box(r[11]) });
		}
		if (!o.curve) return { records, gpuMs };
		const curve = [];
		for (let k = 0; k < p.length; k++) curve.push(samples.slice(k * stride, k * stride + p[k] + 1));
		return { records, curve, gpuMs };
	}
	/** Rule usage (ca3d_ensemble_usage): WHICH entries of its rule tables universe opts.first + k reads over steps[k] steps of its own,
	 *  taken INSIDE one launch behind the queued steps under this ensemble's rule and boundary; this ensemble is left exactly as it is.
	 *  steps: one number for every universe from opts.first on, or an array with one step count per universe, each 1 .. 4096
	 *  -> {records, gpuMs}, records[k] = {steps, usedBorn, usedSurvive ([main, edges, corners]: bit c set where a dead / live cell with
	 *  count c occurred, that is, where born_c / survive_c was read), dead, alive (Uint32Array(49): the cells dead / alive with count c,
	 *  summed over the steps, at bin base + c; main from bin 0, edges from 27, corners from 40; von Neumann and Moore fill main only)}. */
	usage(steps, opts)
	{
		const o = Object.assign({ first: 0 }, opts || {});
		const count = Math.max(this.n - o.first, 0);
		const p = typeof steps === "number" ? new Uint32Array(count).fill(steps) : Uint32Array.from(steps);
		const words = new Uint32Array(p.length * 108);
		const gpuMs = this._a.ensembleUsage(this._e, o.first, p, words);
		const records = [];
		for (let k = 0; k < p.length; k++)
		{
			const r = words.subarray(108 * k, 108 * k + 108);
			records.push({ steps: r[0], usedBorn: Array.from(r.subarray(2, 5)), usedSurvive: Array.from(r.subarray(5, 8)), dead: r.slice(8, 57), alive: r.slice(57, 106) });
		}
		return { records, gpuMs };
	}
	/** The contact sheet (ca3d_ensemble_render_sheet): universes first .. first + count - 1 (default: all from `first`) as tiles of one
	 *  image, one launch; tile k — column k % columns, row floor(k / columns) — is the frame Engine.render draws of universe first + k at
	 *  64^3 with "render_skip" 0, bit for bit. `uniforms`: Float32Array(128) filled for a tileW x tileH window, one block for every tile;
	 *  columns: tiles per row (default ceil(sqrt(count))); spp 1 or 4 -> {width, height, presentation: Uint8Array(width * height * 4)} */
	renderSheet(opts)
	{
		const o = Object.assign({ spp: 1, first: 0 }, opts || {});
		const count = o.count === undefined ? this.n - o.first : o.count;
		const columns = o.columns === undefined ? Math.max(1, Math.ceil(Math.sqrt(count))) : o.columns;
		const width = columns * o.tileW, height = columns ? Math.ceil(count / columns) * o.tileH : 0;
		// (a size the library refuses — nothing to draw, more than 2^26 pixels — gets no array: it names the reason)
		const bytes = width * height * 4;
		const presentation = new Uint8Array(bytes > 0 && bytes <= 4 * 2 ** 26 ? bytes : 0);
		this._a.ensembleRenderSheet(this._e, o.first, count, o.uniforms, o.tileW, o.tileH, columns, o.spp, presentation);
		return { width, height, presentation };
	}
	/** the last sheet: {gpuMs, primaryRays, shadowRays, primaryCellVisits, shadowCellVisits}; waits for it */
	sheetStats() { return this._a.ensembleSheetStats(this._e); }
	synchronize() { this._a.ensembleSynchronize(this._e); }
	stats() { return this._a.ensembleStats(this._e); }
}

module.exports = {
	Engine, EngineGroup, Ensemble, ENSEMBLE_ALL, ENSEMBLE_WORDS, ENSEMBLE_BOUNDARIES, CONNECTIVITIES, STOP_EXTINCT, STOP_STILL, STOP_PERIODIC, STOP_MOVING, NEIGHBOURHOOD_MAP, DEFAULT_RULES, LAYOUT_PACKED32, LAYOUT_UNPACKED, NEIGHBOURS_STORAGE_LEN,
	rulesComponentsToValues, recalculateRulesValues, gridSizeUIFormatter, getClusterIdxFromGridCoordinates,
	initialState, dispatchShape, traceSamples, randomFill, seededState, loadAddon, saveCheckpoint, loadCheckpoint, STAMP_MODES, windowTiling
};
