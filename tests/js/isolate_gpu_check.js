// GPU check of the ensemble's isolate from Node.js. argv[2]: a directory with expected.json — {universes, glider: {born, survive,
// universe, jobs: [[universe, cell]], population, shift, moving: per job {stepsDone, reason, period, shift}}, crafted: {jobs, placement,
// population, shift}} — states.bin (the source, [universe][8192] u32), glider.bin and crafted.bin (the isolated states, one per job).
// The expectations are host.isolate of those states and the definition of step_until_moving on oracle trajectories, written by
// tests/test_js_isolate.py.
"use strict";
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

function typed(Type, buf) { return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length)); }

function main()
{
	const dir = process.argv[2];
	const want = JSON.parse(fs.readFileSync(path.join(dir, "expected.json"), "utf8"));
	const states = typed(Uint32Array, fs.readFileSync(path.join(dir, "states.bin")));
	const B = want.universes;
	assert.strictEqual(states.length, B * c.ENSEMBLE_WORDS);

	const ens = new c.Ensemble(0), nursery = new c.Ensemble(0);
	assert.throws(() => nursery.isolate([[0, 0]], { src: ens }), /ca3d error -2.*destination/); // not configured
	nursery.configure(2, 64, "moore");
	assert.throws(() => nursery.isolate([[0, 0]], { src: ens }), /ca3d error -2.*source/);
	ens.configure(B, 64, "moore");
	assert.throws(() => nursery.isolate([[0, 0]], { src: ens, copyRules: false }), /ca3d error -2.*job 0.*universe 0/); // no states yet
	ens.uploadState(0, states);
	assert.throws(() => nursery.isolate([[0, 0]], { src: ens }), /ca3d error -2.*job 0.*set_rules/); // no rules to copy
	const g = want.glider;
	ens.setRuleStrings(c.ENSEMBLE_ALL, { neighbourhood: "moore", born: g.born, survive: g.survive });

	// what it is for: the glider beside a block — one census, two jobs, and step_until_moving tells them apart
	const census = ens.census(g.universe, 1, 8);
	const jobs = census.components[0].map((o) => [g.universe, o.firstCell]);
	assert.deepStrictEqual(jobs, g.jobs);
	const got = nursery.isolate(jobs, { src: ens });
	assert.deepStrictEqual([Array.from(got.population), Array.from(got.shift)], [g.population, g.shift.flat()]);
	assert.ok(got.gpuMs > 0);
	assert.deepStrictEqual(nursery.readState(), typed(Uint32Array, fs.readFileSync(path.join(dir, "glider.bin"))));
	nursery.summaries().forEach((s, k) => assert.deepStrictEqual([s.step, s.population, s.hasPrevious], [0, g.population[k], false]));
	assert.deepStrictEqual(ens.readState(), states); // the source is only read
	const r = nursery.stepUntilMoving(64, { checkEvery: 4 });
	g.moving.forEach((m, k) => assert.deepStrictEqual(
		{ stepsDone: r.stepsDone[k], reason: r.reason[k], period: r.period[k], shift: Array.from(r.shift.subarray(3 * k, 3 * k + 3)) }, m, "job " + k));
	assert.strictEqual(r.reason[0], c.STOP_MOVING);

	// one crafted shape: every component of `shapes`, to the origin, into a nursery of another kind, without the rules
	const k = want.crafted;
	nursery.configure(k.jobs.length + 1, 64, "von neumann");
	const moved = nursery.isolate(Uint32Array.from(k.jobs.flat()), { src: ens, dstFirst: 1, placement: k.placement, copyRules: false });
	assert.deepStrictEqual([Array.from(moved.population), Array.from(moved.shift)], [k.population, k.shift.flat()]);
	assert.deepStrictEqual(nursery.readState(1, k.jobs.length), typed(Uint32Array, fs.readFileSync(path.join(dir, "crafted.bin"))));
	assert.throws(() => nursery.readState(0, 1), /ca3d error -2/); // universe 0 was no destination
	assert.throws(() => nursery.isolate(k.jobs, { src: ens, placement: k.placement }), /ca3d error -5/); // rules of another kind
	assert.throws(() => nursery.isolate(k.jobs, { src: ens, dstFirst: 2, copyRules: false }), /ca3d error -1/); // one job too many
	assert.throws(() => nursery.isolate([], { src: ens, copyRules: false }), /ca3d error -1/);
	assert.throws(() => nursery.isolate([[B, 0]], { src: ens, copyRules: false }), /ca3d error -1.*job 0/);
	assert.throws(() => nursery.isolate([[0, 1 << 18]], { src: ens, copyRules: false }), /ca3d error -1.*job 0/);
	assert.throws(() => nursery.isolate([[0, 0]], { src: ens, placement: "middle" }), /unknown placement/);
	assert.throws(() => ens.isolate([[1, 0]], { dstFirst: 1 }), /ca3d error -1.*destinations/); // one handle: a source among the destinations
	ens.close();
	nursery.close();
	console.log("ok");
}

main();
