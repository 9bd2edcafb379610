// GPU check of Ensemble.stepUntilMoving from Node.js. argv[2]: a directory with expected.json (the rule and, per run, the call and what the
// Python side expects of it from the oracle), first.bin (the start states, [universe][8192] u32) and states.bin (the oracle's states
// after each run, [run][universe][8192] u32).
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
	const first = fs.readFileSync(path.join(dir, "first.bin")), bin = fs.readFileSync(path.join(dir, "states.bin"));
	const W = c.ENSEMBLE_WORDS, B = first.length / (W * 4);
	assert.strictEqual(bin.length, want.runs.length * B * W * 4);
	assert.strictEqual(c.STOP_MOVING, 8);

	const ens = new c.Ensemble(0);
	assert.throws(() => ens.stepUntilMoving(4), /ca3d error -2/);
	want.runs.forEach((run, r) => {
		ens.configure(B, 64, "moore");
		ens.setRuleStrings(c.ENSEMBLE_ALL, { neighbourhood: "moore", born: want.born, survive: want.survive });
		ens.uploadState(0, new Uint32Array(first.buffer.slice(first.byteOffset, first.byteOffset + first.length)));
		assert.throws(() => ens.stepUntilMoving(4, { stopMask: 16 }), /ca3d error -1/);
		assert.throws(() => ens.stepUntilCycle(4, { stopMask: c.STOP_MOVING }), /ca3d error -1/);
		const got = ens.stepUntilMoving(run.maxSteps, { checkEvery: run.checkEvery, stopMask: run.stopMask });
		assert.ok(got.shift instanceof Int32Array && got.shift.length === 3 * B);
		assert.deepStrictEqual(Array.from(got.stepsDone), run.stepsDone);
		assert.deepStrictEqual(Array.from(got.reason), run.reason);
		assert.deepStrictEqual(Array.from(got.period), run.period);
		assert.deepStrictEqual(Array.from(got.shift), run.shift);
		const states = ens.readState();
		for (let u = 0; u < B; u++)
			assert.ok(Buffer.from(states.buffer, u * W * 4, W * 4).equals(bin.subarray((r * B + u) * W * 4, (r * B + u + 1) * W * 4)), "run " + r + " universe " + u);
	});
	// the default mask holds STOP_MOVING
	const again = ens.stepUntilMoving(48, { checkEvery: 4 });
	assert.ok(Array.from(again.reason).every((v) => v === c.STOP_MOVING));
	ens.close();
	console.log("ok");
}
main();
