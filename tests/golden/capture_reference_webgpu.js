#!/usr/bin/env node
/*
 * Fixture generator: runs the REFERENCE's own host JavaScript (main_pathtraced.js + MemoryManager.js + ui.js +
 * libs/wgpu-matrix.module.js), unmodified, under Node with DOM shims and the navigator.gpu façade
 * (cellularautomatons3d_amd/js/webgpu_facade.js) over a do-nothing engine, through init and four more frames, and records
 * every call the host makes on the WebGPU objects: tests/golden/reference_webgpu_calls.json. tests/js/facade_reference_mock.js
 * replays that sequence against the façade, so the test needs no reference sources.
 *
 * Only DATA is written into the repo: call names, descriptor fields, the bytes the host uploads (as sparse 32-bit words) and
 * object handles. Shader code and labels are dropped; the façade recognises the pipelines by their entry-point names. The
 * reference sources are copied to a throw-away directory under os.tmpdir() for the duration of the run and deleted afterwards.
 *
 * Usage: node tests/golden/capture_reference_webgpu.js <reference checkout>
 */
"use strict";
const fs = require("fs");
const os = require("os");
const path = require("path");

const REF = process.argv[2];
const OUT = path.join(__dirname, "reference_webgpu_calls.json");
const root = path.join(__dirname, "..", "..");
const { installFacade } = require(path.join(root, "cellularautomatons3d_amd", "js", "webgpu_facade.js"));

const W = 640, H = 360;
const calls = [];
const idOf = new WeakMap(), proxyOf = new WeakMap(), rawOf = new WeakMap();
let nextId = 0;

function words(bytes)
{
	// the bytes as little-endian 32-bit words, zero words left out: [[index, word], ...]
	const n = bytes.byteLength;
	const padded = new Uint8Array((n + 3) & ~3);
	padded.set(bytes);
	const w = new Uint32Array(padded.buffer);
	const out = [];
	for (let i = 0; i < w.length; i++) { if (w[i] !== 0) { out.push([i, w[i]]); } }
	return out;
}

function ser(v)
{
	if (v === null || v === undefined || typeof v !== "object") { return typeof v === "function" ? undefined : v; }
	if (rawOf.has(v)) { return { $ref: idOf.get(rawOf.get(v)) }; }
	if (v instanceof ArrayBuffer) { return { $ab: v.byteLength, w: words(new Uint8Array(v)) }; }
	if (ArrayBuffer.isView(v)) { return { $ta: v.constructor.name, bytes: v.byteLength, w: words(new Uint8Array(v.buffer, v.byteOffset, v.byteLength)) }; }
	if (Array.isArray(v)) { return v.map(ser); }
	const o = {};
	for (const k of Object.keys(v)) { if (k !== "label" && k !== "code") { o[k] = ser(v[k]); } }
	return o;
}

function wrap(obj, id)
{
	if (obj === null || typeof obj !== "object" || ArrayBuffer.isView(obj) || obj instanceof ArrayBuffer) { return obj; }
	if (proxyOf.has(obj)) { return proxyOf.get(obj); }
	idOf.set(obj, id || "o" + nextId++);
	const p = new Proxy(obj, {
		get(t, k)
		{
			const v = t[k];
			if (typeof v === "function") { return (...args) => call(t, k, v, args); }
			if (k === "queue" && v && typeof v === "object" && !proxyOf.has(v))
			{
				// a sub-object the host calls methods on: recorded as a property read
				const w = wrap(v);
				calls.push({ o: idOf.get(t), p: k, r: idOf.get(v) });
				return w;
			}
			return k === "queue" ? proxyOf.get(v) : v;
		}
	});
	proxyOf.set(obj, p);
	rawOf.set(p, obj);
	return p;
}

function call(t, k, fn, args)
{
	const entry = { o: idOf.get(t), m: k, a: args.map(ser) };
	calls.push(entry);
	const r = fn.apply(t, args);
	const keep = (x) => { if (x && typeof x === "object" && !ArrayBuffer.isView(x)) { const w = wrap(x); entry.r = idOf.get(x); return w; } return x; };
	if (r && typeof r.then === "function") { entry.async = true; return r.then(keep); }
	return keep(r);
}

async function main()
{
	if (!REF) { throw new Error("usage: capture_reference_webgpu.js <reference checkout>"); }
	const tmp = fs.mkdtempSync(path.join(os.tmpdir(), "ca3d-capture-"));
	const log = console.log;
	try
	{
		fs.mkdirSync(path.join(tmp, "libs"));
		for (const f of ["main_pathtraced.js", "MemoryManager.js", "ui.js", "libs/wgpu-matrix.module.js"]) { fs.copyFileSync(path.join(REF, f), path.join(tmp, f)); }
		fs.writeFileSync(path.join(tmp, "package.json"), JSON.stringify({ type: "module" }));
		let now = 1000;
		global.performance = { now: () => now };
		let raf = null;
		global.requestAnimationFrame = (cb) => { raf = cb; };
		global.window = { innerWidth: W, innerHeight: H, devicePixelRatio: 1, addEventListener() {} };
		const stubEl = { addEventListener() {}, removeEventListener() {}, querySelectorAll() { return []; }, classList: { add() {}, remove() {} } };
		const engine = { configure() {}, setRules() {}, setRuleStrings() {}, uploadState() {}, step() {}, render() {} };
		const facade = installFacade(global, { engine, width: W, height: H });
		global.navigator.gpu = wrap(facade.gpu, "gpu");
		const ctx = wrap(facade.canvasContext, "ctx");
		const canvas = { width: 0, height: 0, getContext: () => ctx, addEventListener() {}, requestPointerLock() {} };
		global.document = { querySelector: (q) => (q === ".main-canvas" ? canvas : stubEl), body: { insertAdjacentHTML() {} }, pointerLockElement: null, addEventListener() {} };
		global.fetch = async (url) => ({ text: async () => fs.readFileSync(path.join(REF, url), "utf8") });
		if (!String.prototype.replaceAll) { String.prototype.replaceAll = function (a, b) { return this.split(a).join(b); }; } // Node 12
		console.log = () => {};
		await import(path.join(tmp, "main_pathtraced.js"));
		global.window.onload();
		for (let i = 0; i < 200 && !raf; i++) { await new Promise((r) => setTimeout(r, 10)); }
		console.log = log;
		if (!raf) { throw new Error("init() did not reach the frame loop"); }
		// init() already ran one _updateLoop; run 4 more frames 50 ms apart (each crosses the 48 ms step gate)
		for (let f = 0; f < 4; f++) { now += 50; const cb = raf; raf = null; cb(); }
		const doc = { generator: "tests/golden/capture_reference_webgpu.js", node: process.version, window: [W, H],
			frames: 5, simulation_step: global.window.mm._simulationStep, calls };
		fs.writeFileSync(OUT, JSON.stringify(doc) + "\n");
		console.log(`${calls.length} calls -> ${path.relative(root, OUT)}`);
	}
	finally
	{
		console.log = log;
		fs.rmdirSync(tmp, { recursive: true });
	}
}
main().catch((e) => { console.error(e); process.exit(1); });
