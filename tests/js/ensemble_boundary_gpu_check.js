// GPU check of the ensemble boundaries from Node.js. argv[2]: a directory with expected.json (per case: kind, boundary, masks, steps) and
// first.bin / states.bin (the uploaded states and the states Python's Ensemble read back after the same steps, [case][universe][8192] u32).
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
	const W = c.ENSEMBLE_WORDS, B = want.universes;
	assert.deepStrictEqual(c.ENSEMBLE_BOUNDARIES, ["reference", "torus", "closed"]);
	assert.strictEqual(bin.length, want.cases.length * B * W * 4);

	const ens = new c.Ensemble(0);
	assert.throws(() => ens.boundary, /ca3d error -2/);
	assert.throws(() => ens.setBoundary("torus"), /ca3d error -2/);
	assert.throws(() => ens.configure(B, 64, "moore", false, { boundary: "mirror" }), /unknown ensemble boundary/);
	const words = new Uint32Array(first.buffer.slice(first.byteOffset, first.byteOffset + B * W * 4));
	want.cases.forEach((k, i) => {
		// the first case names its boundary when it configures, the others set it afterwards
		if (i === 0) ens.configure(B, 64, k.kind === "von neumann" ? "von neumann" : "moore", k.kind === "clustered", { boundary: k.boundary });
		else
		{
			ens.configure(B, 64, k.kind === "von neumann" ? "von neumann" : "moore", k.kind === "clustered");
			assert.strictEqual(ens.boundary, "reference"); // every configure goes back to the reference
			assert.throws(() => ens.setBoundary("mirror"), /unknown ensemble boundary/);
			ens.setBoundary(k.boundary);
		}
		assert.strictEqual(ens.boundary, k.boundary);
		if (k.kind === "clustered") ens.setClusteredTables(0, k.born, k.survive);
		else ens.setRuleTables(0, k.born, k.survive);
		ens.uploadState(0, words);
		ens.step(k.steps);
		const states = ens.readState();
		for (let u = 0; u < B; u++)
			assert.ok(Buffer.from(states.buffer, u * W * 4, W * 4).equals(bin.subarray((i * B + u) * W * 4, (i * B + u + 1) * W * 4)),
				k.kind + ", " + k.boundary + ": universe " + u);
	});
	ens.close();
	console.log("ok");
}
main();
