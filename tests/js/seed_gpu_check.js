// GPU check of device seeding from Node.js: Engine.seedState on a 64^3 engine, Ensemble.seedStates + setRuleTables on eight universes,
// stepUntil; states against the JS definition (seededState), records against Engine.summary() of lone engines given the same universes.
"use strict";
const assert = require("assert");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

const RULES = [["1,3", "0-6"], ["2,4", "1,3,5"], ["", ""], ["", "0-6"], ["3", "2,3"], ["1", ""], ["5,6", "4-6"], ["2", "1-3"]];
const B = RULES.length, W = c.ENSEMBLE_WORDS;
const maskOf = (text) => c.rulesComponentsToValues(text).reduce((m, v) => m | (1 << v), 0);
const same = (a, b, what) => assert.deepStrictEqual(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength), what);

function main()
{
	assert.strictEqual(maskOf("2,4"), 0x14);
	assert.strictEqual(maskOf("1,3,5"), 0x2A);
	const box = { min: [5, 0, 60], max: [40, 63, 63] };

	// one engine
	const eng = new c.Engine(0);
	assert.throws(() => eng.seedState({ seed: 1 }), /ca3d error -2/);
	eng.configure(64);
	assert.throws(() => eng.seedState({ seed: 1, andRounds: 32 }), /ca3d error -1/);
	assert.throws(() => eng.seedState({ seed: 1, box: { min: [0, 0, 0], max: [64, 63, 63] } }), /ca3d error -1/);
	eng.seedState({ seed: 3, andRounds: 1, box }); // rules need not be set
	same(eng.readState(), c.seededState(64, 3, { andRounds: 1, box }), "boxed seed");
	let s = eng.summary();
	assert.strictEqual(s.population, 2325);
	assert.deepStrictEqual([s.step, s.hasPrevious, s.boxMin, s.boxMax], [0, false, box.min, box.max]);
	eng.seedState({ seed: 9, andRounds: 2 });
	same(eng.readState(), c.randomFill(W, 9, 2), "whole-grid seed equals randomFill");
	eng.setRuleStrings({ born: "2,4", survive: "1,3,5" });
	eng.setOption("queue", 16);
	eng.step(5);
	eng.seedState({ seed: 9, andRounds: 2 }); // drops the queued steps
	eng.setOption("queue", 0);
	assert.strictEqual(eng.info().step, 0);
	eng.step(24);
	const twin = new c.Engine(0);
	twin.configure(64);
	twin.setRuleStrings({ born: "2,4", survive: "1,3,5" });
	twin.uploadState(c.randomFill(W, 9, 2));
	twin.step(24);
	same(eng.readState(), twin.readState(), "24 steps from a seed and from an upload");
	assert.deepStrictEqual(eng.summary(), twin.summary());
	assert.strictEqual(eng.recoveredLaunches(), 0);
	twin.close();

	// eight universes: rules as masks in one call, seeds in one call
	const ens = new c.Ensemble(0);
	ens.configure(B);
	assert.throws(() => ens.setRuleTables(0, RULES.map((r, u) => maskOf(r[0]) | (u === 6 ? 0x80 : 0)), RULES.map((r) => maskOf(r[1]))), /ca3d error -1.*universe 6/);
	ens.setRuleTables(0, RULES.map((r) => maskOf(r[0])), RULES.map((r) => maskOf(r[1])));
	const specs = RULES.map((_, u) => ({ seed: 1 + u, andRounds: [0, 2, 5][u % 3], box: u % 2 ? box : undefined }));
	assert.throws(() => ens.seedStates(4, specs), /ca3d error -1/); // past the end
	ens.seedStates(0, specs);
	const first = ens.readState();
	for (let u = 0; u < B; u++)
	{
		same(first.subarray(u * W, (u + 1) * W), c.seededState(64, specs[u].seed, specs[u]), "universe " + u);
	}
	for (const r of ens.summaries()) { assert.strictEqual(r.step, 0); assert.strictEqual(r.hasPrevious, false); }

	const r = ens.stepUntil(40, { checkEvery: 4 });
	const recs = ens.summaries(), states = ens.readState();
	for (let u = 0; u < B; u++)
	{
		const done = r.stepsDone[u];
		assert.ok(done === 40 || (done % 4 === 0 && r.reason[u] !== 0), "universe " + u);
		eng.setRuleStrings({ born: RULES[u][0], survive: RULES[u][1] });
		eng.uploadState(c.seededState(64, specs[u].seed, specs[u]));
		eng.step(done);
		const one = eng.summary();
		assert.deepStrictEqual(recs[u], one, "universe " + u + " after " + done + " steps");
		same(states.subarray(u * W, (u + 1) * W), eng.readState(), "universe " + u);
		const want = (one.population === 0 ? c.STOP_EXTINCT : 0) | (one.hasPrevious && one.births + one.deaths === 0 ? c.STOP_STILL : 0);
		assert.strictEqual(r.reason[u], want, "universe " + u);
	}
	// one spec for a sub-range leaves the others alone
	ens.seedStates(2, { seed: 77, andRounds: 1 }, 3);
	const after = ens.readState(), now = ens.summaries();
	for (let u = 0; u < B; u++)
	{
		if (u >= 2 && u < 5) { same(after.subarray(u * W, (u + 1) * W), c.randomFill(W, 77, 1), "universe " + u); assert.strictEqual(now[u].step, 0); }
		else { same(after.subarray(u * W, (u + 1) * W), states.subarray(u * W, (u + 1) * W), "universe " + u); assert.deepStrictEqual(now[u], recs[u]); }
	}
	ens.setRuleTables(0, 0x0A, 0x7F); // the start-up rule for every universe
	ens.step(2);
	eng.setRuleStrings({});
	eng.uploadState(c.randomFill(W, 77, 1));
	eng.step(2);
	same(ens.readState(3, 1), eng.readState(), "universe 3 under the start-up rule");

	// the group, two slabs on one device
	const grp = new c.EngineGroup([0, 0]);
	grp.configure(64, 2);
	grp.setRuleStrings({});
	grp.seedState({ seed: 3, andRounds: 1, box });
	same(grp.readState(), c.seededState(64, 3, { andRounds: 1, box }), "group seed");
	grp.step(5);
	eng.uploadState(c.seededState(64, 3, { andRounds: 1, box }));
	eng.step(5);
	same(grp.readState(), eng.readState(), "group, five steps on");
	grp.close();
	eng.close();
	ens.close();
	console.log("ok");
}
main();
