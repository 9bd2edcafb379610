// GPU check of the ensemble's rule usage from Node.js. argv[2]: a directory with expected.json — {boundary, steps, cases: per ensemble
// kind {kind, born, survive (masks; clustered: three each), record: what Ensemble.usage returns of universe 0}} — and states.bin
// ([2][8192] u32: universe 0's state, and an empty universe). The expectations are host.usage of that state, written by
// tests/test_js_usage.py.
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
	assert.strictEqual(states.length, 2 * c.ENSEMBLE_WORDS);

	for (const k of want.cases)
	{
		const ens = new c.Ensemble(0);
		assert.throws(() => ens.usage(want.steps), /ca3d error -2.*configure/); // not configured
		const clustered = k.kind === "clustered";
		ens.configure(2, 64, k.kind === "von neumann" ? "von neumann" : "moore", clustered, { boundary: want.boundary });
		assert.throws(() => ens.usage(want.steps), /ca3d error -2.*universe 0/); // no states yet
		ens.uploadState(0, states);
		assert.throws(() => ens.usage(want.steps), /ca3d error -2.*set_rules.*universe 0/); // no rules yet
		if (clustered) ens.setClusteredTables(0, k.born, k.survive);
		else ens.setRuleTables(0, k.born, k.survive);

		const got = ens.usage(want.steps);
		assert.ok(got.gpuMs > 0);
		assert.strictEqual(got.records.length, 2);
		const r = got.records[0];
		assert.ok(r.dead instanceof Uint32Array && r.alive instanceof Uint32Array && r.dead.length === 49 && r.alive.length === 49);
		assert.deepStrictEqual({ steps: r.steps, usedBorn: r.usedBorn, usedSurvive: r.usedSurvive, dead: Array.from(r.dead), alive: Array.from(r.alive) }, k.record, k.kind);
		// the empty universe: every cell dead, and what becomes of it depends on born at 0 alone
		const e = got.records[1];
		assert.strictEqual(e.dead[0] + e.alive[0], 262144 * want.steps, k.kind);
		assert.strictEqual(e.dead[0] >= 262144, true);
		// over a range, and with one step count per universe
		assert.deepStrictEqual(ens.usage([want.steps], { first: 0 }).records[0], r);
		assert.strictEqual(ens.usage(1, { first: 1 }).records.length, 1);
		assert.deepStrictEqual(ens.readState(), states); // the call only reads
		assert.strictEqual(ens.summaries()[0].step, 0);

		assert.throws(() => ens.usage(want.steps, { first: 2 }), /ca3d error -1.*universes/); // a range past n
		assert.throws(() => ens.usage([]), /ca3d error -1.*universes/);
		assert.throws(() => ens.usage([0, 1]), /ca3d error -1.*steps\[0\]/);
		assert.throws(() => ens.usage(4097), /ca3d error -1.*steps\[0\]/);
		ens.close();
	}
	console.log("ok");
}

main();
