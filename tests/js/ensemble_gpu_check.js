// GPU check of the Ensemble class from Node.js: eight universes with different rules run until each one's own end; every record is
// compared with Engine.summary() of a lone engine given the same universe and stepped as often.
"use strict";
const assert = require("assert");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

const RULES = [["1,3", "0-6"], ["2,4", "1,3,5"], ["", ""], ["", "0-6"], ["3", "2,3"], ["1", ""], ["5,6", "4-6"], ["2", "1-3"]];
const B = RULES.length, W = c.ENSEMBLE_WORDS;

function main()
{
	const ens = new c.Ensemble(0);
	assert.throws(() => ens.configure(B, 128), /ca3d error -5/);
	ens.configure(B);
	assert.throws(() => ens.step(1), /ca3d error -2/);
	const words = new Uint32Array(B * W);
	for (let u = 0; u < B; u++)
	{
		ens.setRuleStrings(u, { born: RULES[u][0], survive: RULES[u][1] });
		words.set(c.randomFill(W, 1 + u, [0, 2, 5][u % 3]), u * W);
	}
	assert.throws(() => ens.setRuleStrings(0, { neighbourhood: "moore", born: "4", survive: "4" }), /ca3d error -5.*universe 0/);
	ens.uploadState(0, words);
	for (const s of ens.summaries()) { assert.strictEqual(s.step, 0); assert.strictEqual(s.hasPrevious, false); }

	const r = ens.stepUntil(40, { checkEvery: 4 });
	assert.strictEqual(r.stepsDone.length, B);
	const recs = ens.summaries(), states = ens.readState();
	const outcomes = new Set();
	const eng = new c.Engine(0);
	eng.configure(64);
	for (let u = 0; u < B; u++)
	{
		const done = r.stepsDone[u];
		outcomes.add(r.reason[u]);
		assert.ok(done === 40 || (done % 4 === 0 && r.reason[u] !== 0), "universe " + u);
		eng.setRuleStrings({ born: RULES[u][0], survive: RULES[u][1] });
		eng.uploadState(words.subarray(u * W, (u + 1) * W));
		eng.step(done);
		const one = eng.summary();
		assert.strictEqual(typeof recs[u].digest, "bigint");
		assert.deepStrictEqual(recs[u], one, "universe " + u + " after " + done + " steps");
		assert.deepStrictEqual(Buffer.from(states.buffer, u * W * 4, W * 4), Buffer.from(eng.readState().buffer), "universe " + u);
		// the reason is what the record says
		const want = (one.population === 0 ? c.STOP_EXTINCT : 0) | (one.hasPrevious && one.births + one.deaths === 0 ? c.STOP_STILL : 0);
		assert.strictEqual(r.reason[u], want, "universe " + u);
	}
	// died out (seen a check late, an empty grid is still as well), froze alive, still changing
	assert.ok(outcomes.has(0) && outcomes.has(c.STOP_EXTINCT | c.STOP_STILL) && outcomes.has(c.STOP_STILL), [...outcomes].join());
	ens.step(3);
	assert.deepStrictEqual(ens.summaries(1, 1)[0].step, r.stepsDone[1] + 3);
	assert.strictEqual(ens.stats().cellSteps, 3 * B * 64 * 64 * 64);
	eng.close();
	ens.close();
	console.log("ok");
}
main();
