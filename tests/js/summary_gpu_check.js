// GPU check of engine.summary() / engine.stepUntil() / EngineGroup.summary() from Node.js: the numbers of the device against a
// few lines of straightforward JavaScript over the JS CPU stepper's states (oracle/js_stepper.js).
"use strict";
const assert = require("assert");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));
const js = require(path.join(root, "oracle", "js_stepper.js"));

const M64 = (1n << 64n) - 1n;
function mix(i, w)
{
	let z = ((((BigInt(i) << 32n) & M64) | BigInt(w)) + 0x9E3779B97F4A7C15n) & M64;
	z = ((z ^ (z >> 30n)) * 0xBF58476D1CE4E5B9n) & M64;
	z = ((z ^ (z >> 27n)) * 0x94D049BB133111EBn) & M64;
	return z ^ (z >> 31n);
}
// the definition of include/ca3d.h, cell by cell
function summarize(G, cur, prev)
{
	const cols = G / 32;
	const s = { population: 0, births: 0, deaths: 0, digest: 0n, boxMin: [G, G, G], boxMax: [0, 0, 0], planePopulation: new Uint32Array(G) };
	for (let i = 0; i < cur.length; i++)
	{
		const w = cur[i], q = prev ? prev[i] : 0;
		if (w !== 0) s.digest = (s.digest + mix(i, w)) & M64;
		if (w === 0 && q === 0) continue;
		const z = Math.floor(i / (cols * G)), y = Math.floor(i / cols) % G, xc = i % cols;
		for (let b = 0; b < 32; b++)
		{
			const now = (w >>> b) & 1, was = (q >>> b) & 1;
			if (prev && now && !was) s.births++;
			if (prev && was && !now) s.deaths++;
			if (!now) continue;
			s.population++;
			s.planePopulation[z]++;
			const p = [xc * 32 + b, y, z];
			for (let k = 0; k < 3; k++) { s.boxMin[k] = Math.min(s.boxMin[k], p[k]); s.boxMax[k] = Math.max(s.boxMax[k], p[k]); }
		}
	}
	if (s.population === 0) { s.boxMin = [G, G, G]; s.boxMax = [0, 0, 0]; }
	return s;
}
function same(got, want, step, hasPrevious, where)
{
	assert.strictEqual(got.step, step, where);
	assert.strictEqual(got.hasPrevious, hasPrevious, where);
	for (const k of ["population", "births", "deaths", "digest"]) assert.strictEqual(got[k], want[k], where + " " + k);
	assert.strictEqual(typeof got.digest, "bigint");
	assert.deepStrictEqual(got.boxMin, want.boxMin, where);
	assert.deepStrictEqual(got.boxMax, want.boxMax, where);
	if (got.planePopulation) assert.deepStrictEqual(Buffer.from(got.planePopulation.buffer), Buffer.from(want.planePopulation.buffer), where);
}
function stepper(G, rules)
{
	const r = Object.assign({}, c.DEFAULT_RULES, rules);
	const lut = c.recalculateRulesValues(r);
	return js.makeStepper(G, [c.NEIGHBOURHOOD_MAP[r.neighbourhood], c.NEIGHBOURHOOD_MAP["edges"], c.NEIGHBOURHOOD_MAP["corners"]], lut.survive, lut.born);
}

async function main()
{
	const eng = new c.Engine(0);
	for (const G of [64, 128])
	{
		// summary after an upload, one step and four more, on a rule that keeps changing
		const rules = { neighbourhood: "von neumann", born: "2,4", survive: "1,3,5" };
		const st = c.randomFill((G / 32) * G * G, 21, 0);
		const step = stepper(G, rules);
		eng.configure(G);
		eng.setRuleStrings(rules);
		eng.uploadState(st);
		same(eng.summary({ planes: true }), summarize(G, st, null), 0, false, G + " upload");
		let a = st.slice(), b = new Uint32Array(a.length), done = 0;
		for (const n of [1, 4])
		{
			eng.step(n);
			for (let i = 0; i < n; i++) { step(a, b); const t = a; a = b; b = t; }
			done += n;
			same(eng.summary({ planes: true }), summarize(G, a, b), done, true, G + " step " + done);
			assert.strictEqual(eng.summary().planePopulation, undefined);
		}

		// stepUntil on the default rule: the first step at which nothing changes, found with the JS stepper
		const dstep = stepper(G, {});
		const states = [st.slice()];
		let still = 0;
		for (let s = 1; s < 64 && !still; s++)
		{
			const next = new Uint32Array(st.length);
			dstep(states[s - 1], next);
			states.push(next);
			if (Buffer.compare(Buffer.from(next.buffer), Buffer.from(states[s - 1].buffer)) === 0) still = s;
		}
		assert.ok(still > 0);
		while (states.length <= 16) { const next = new Uint32Array(st.length); dstep(states[states.length - 1], next); states.push(next); }
		for (const every of [1, 8])
		{
			eng.setRuleStrings({});
			eng.uploadState(st);
			const p = eng.stepUntil(1000, { checkEvery: every });
			assert.throws(() => eng.step(1), /asynchronous call is pending/); // the engine is on a worker thread meanwhile
			const r = await p;
			const want = every === 1 ? still : Math.ceil(still / every) * every;
			assert.strictEqual(r.stepsDone, want);
			assert.strictEqual(r.reason, c.STOP_STILL);
			assert.strictEqual(eng.info().step, want);
			assert.deepStrictEqual(Buffer.from(eng.readState().buffer), Buffer.from(states[want].buffer));
			same(r.summary, summarize(G, states[want], states[want - 1]), want, true, G + " stepUntil " + every);
			assert.strictEqual(r.summary.births + r.summary.deaths, 0);
		}
		const none = await eng.stepUntil(0, { still: false, extinct: false });
		assert.strictEqual(none.stepsDone, 0);
		assert.strictEqual(none.reason, 0);

		// the slab split of the same run: EngineGroup.summary equals the single engine's
		eng.setRuleStrings(rules);
		eng.uploadState(st);
		eng.step(6);
		const g = new c.EngineGroup([0, 0]);
		g.configure(G, 2);
		g.setRuleStrings(rules);
		g.uploadState(st);
		g.step(6);
		const one = eng.summary({ planes: true }), all = g.summary({ planes: true });
		same(all, one, 6, true, G + " group");
		g.close();
	}
	eng.close();
	console.log("ok");
}
main().catch((e) => { console.error(e); process.exit(1); });
