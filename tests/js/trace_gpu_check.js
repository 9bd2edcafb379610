// GPU check of the ensemble trace from Node.js. argv[2]: a directory with expected.json (rules, seeds and, per stop mask, the samples,
// counts, stepsDone and reason the Python side computed from the oracle) and states.bin (the oracle's state each universe ends in,
// [mask][universe][8192] u32).
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
	const B = want.universes, W = c.ENSEMBLE_WORDS, K = c.traceSamples(want.maxSteps, want.checkEvery);
	assert.strictEqual(bin.length, want.cases.length * W * 4);

	const ens = new c.Ensemble(0);
	ens.configure(B);
	assert.throws(() => ens.stepTrace(4, 1, 0), /ca3d error -2/); // no rules yet
	for (let round = 0; round * B < want.cases.length; round++)
	{
		const cases = want.cases.slice(round * B, (round + 1) * B);
		const words = new Uint32Array(B * W);
		cases.forEach((k, u) => {
			ens.setRuleStrings(u, { born: k.born, survive: k.survive });
			words.set(c.randomFill(W, k.seed, k.andRounds), u * W);
		});
		ens.uploadState(0, words);
		assert.throws(() => ens.stepTrace(4, 1, c.STOP_PERIODIC), /ca3d error -1/);
		assert.throws(() => ens.stepTrace(4, 0, 0), /ca3d error -1/);
		const got = ens.stepTrace(want.maxSteps, want.checkEvery, cases[0].stopMask);
		assert.strictEqual(got.samplesPerUniverse, K);
		assert.strictEqual(got.samples.length, B * K * 3);
		const states = ens.readState();
		for (let u = 0; u < B; u++)
		{
			const k = cases[u], where = "mask " + k.stopMask + " universe " + u;
			assert.deepStrictEqual([got.nSamples[u], got.stepsDone[u], got.reason[u]], [k.nSamples, k.stepsDone, k.reason], where);
			assert.deepStrictEqual(Array.from(got.samples.subarray(u * K * 3, (u + 1) * K * 3)), k.samples, where);
			const at = (round * B + u) * W * 4;
			assert.ok(Buffer.from(states.buffer, u * W * 4, W * 4).equals(bin.subarray(at, at + W * 4)), where);
		}
	}
	ens.close();
	console.log("ok");
}
main();
