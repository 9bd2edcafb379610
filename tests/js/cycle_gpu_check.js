// GPU check of cycle detection from Node.js. argv[2]: a directory with expected.json (rules, seeds and the (stepsDone, reason, period) the
// Python side computed from the oracle) and states.bin (the oracle's state each universe stops in, [universe][8192] u32).
"use strict";
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

async function main()
{
	const dir = process.argv[2];
	const want = JSON.parse(fs.readFileSync(path.join(dir, "expected.json"), "utf8"));
	const bin = fs.readFileSync(path.join(dir, "states.bin"));
	const B = want.cases.length, W = c.ENSEMBLE_WORDS;
	assert.strictEqual(bin.length, B * W * 4);
	assert.strictEqual(c.STOP_PERIODIC, 4);
	const opts = { checkEvery: want.checkEvery };

	const ens = new c.Ensemble(0);
	ens.configure(B);
	const words = new Uint32Array(B * W);
	want.cases.forEach((k, u) => {
		ens.setRuleStrings(u, { born: k.born, survive: k.survive });
		words.set(c.randomFill(W, k.seed, k.andRounds), u * W);
	});
	ens.uploadState(0, words);
	assert.throws(() => ens.stepUntilCycle(4, { stopMask: 8 }), /ca3d error -1/);
	assert.throws(() => ens.stepUntil(4, { stopMask: c.STOP_PERIODIC }), /ca3d error -1/);
	const got = ens.stepUntilCycle(want.maxSteps, opts);
	const states = ens.readState();
	for (let u = 0; u < B; u++)
	{
		const k = want.cases[u], where = "universe " + u;
		assert.deepStrictEqual([got.stepsDone[u], got.reason[u], got.period[u]], [k.stepsDone, k.reason, k.period], where);
		assert.ok(Buffer.from(states.buffer, u * W * 4, W * 4).equals(bin.subarray(u * W * 4, (u + 1) * W * 4)), where);
	}
	ens.close();

	// the first universe again, in a lone engine
	const k = want.cases[0];
	const eng = new c.Engine(0);
	eng.configure(64);
	eng.setRuleStrings({ born: k.born, survive: k.survive });
	eng.uploadState(c.randomFill(W, k.seed, k.andRounds));
	const one = await eng.stepUntilCycle(want.maxSteps, opts);
	assert.deepStrictEqual([one.stepsDone, one.reason, one.period], [k.stepsDone, k.reason, k.period]);
	assert.strictEqual(one.summary.step, k.stepsDone);
	const st = await eng.readState();
	assert.ok(Buffer.from(st.buffer, st.byteOffset, W * 4).equals(bin.subarray(0, W * 4)));
	const plain = await eng.stepUntilCycle(4, { checkEvery: 1, periodic: false, extinct: false, still: false });
	assert.deepStrictEqual([plain.stepsDone, plain.reason, plain.period], [4, 0, 0]);
	eng.close();
	console.log("ok");
}
main().catch((e) => { console.error(e); process.exit(1); });
