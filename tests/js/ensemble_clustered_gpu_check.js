// GPU check of a clustered Ensemble from Node.js. argv[2]: a directory with expected.json (rules as strings and as masks, seeds and the
// records the Python side computed from the oracle) and states.bin (the oracle's states, [universe][check point][8192] u32).
"use strict";
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

function main()
{
	const dir = process.argv[2];
	const want = JSON.parse(fs.readFileSync(path.join(dir, "expected.json"), "utf8"));
	const bin = fs.readFileSync(path.join(dir, "states.bin"));
	const B = want.cases.length, W = c.ENSEMBLE_WORDS, P = want.steps.length;
	assert.strictEqual(bin.length, B * P * W * 4);

	const ens = new c.Ensemble(0);
	assert.throws(() => ens.clustered, /ca3d error -2/);
	assert.throws(() => ens.configure(B, 64, "von neumann", true), /clustered/);
	assert.throws(() => ens.configure(B, 64, undefined, true), /clustered/);
	ens.configure(B, 64, "moore");
	assert.strictEqual(ens.clustered, false);
	assert.throws(() => ens.setClusteredTables(0, [1, 1, 1], [1, 1, 1]), /ca3d error -5/);
	ens.configure(B, 64, "moore", true);
	assert.strictEqual(ens.clustered, true);
	assert.strictEqual(ens.neighbourhood, "moore");
	assert.throws(() => ens.setRuleStrings(1, { born: "1,3", survive: "0-6" }), /ca3d error -5.*universe 1/);
	assert.throws(() => ens.setClusteredTables(0, [[1, 1, 1], [1, 2 ** 13, 1]], [[0, 0, 0], [0, 0, 0]]), /ca3d error -1.*universe 1/);
	assert.throws(() => ens.setClusteredTables(0, [1, 1, 2 ** 9], [0, 0, 0]), /ca3d error -1.*universe 0/);
	const words = new Uint32Array(B * W);
	// the first half by strings, the second half by masks, in one call
	const half = B >> 1;
	want.cases.forEach((k, u) => {
		if (u < half) ens.setRuleStrings(u, k.rules);
		words.set(c.randomFill(W, k.seed, k.andRounds), u * W);
	});
	ens.setClusteredTables(half, want.cases.slice(half).map((k) => k.bornMasks), want.cases.slice(half).map((k) => k.surviveMasks));
	ens.uploadState(0, words);
	for (const s of ens.summaries()) { assert.strictEqual(s.step, 0); assert.strictEqual(s.hasPrevious, false); }
	want.steps.forEach((n, p) => {
		ens.step(n);
		const recs = ens.summaries(), states = ens.readState();
		for (let u = 0; u < B; u++)
		{
			const where = "universe " + u + " at check point " + p;
			const e = Object.assign({}, want.cases[u].records[p]);
			e.digest = BigInt(e.digest);
			assert.deepStrictEqual(recs[u], e, where);
			assert.ok(Buffer.from(states.buffer, u * W * 4, W * 4).equals(bin.subarray((u * P + p) * W * 4, (u * P + p + 1) * W * 4)), where);
		}
	});
	ens.close();
	console.log("ok");
}
main();
