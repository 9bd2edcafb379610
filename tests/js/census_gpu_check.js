// GPU check of the ensemble's census from Node.js. argv[2]: a directory with expected.json — {universes, maxComponents, lists: per
// universe [{population, firstCell, boxMin, boxMax, digest (decimal string)}], glider: {born, survive, universe, every, lists: the
// same per census}} — and states.bin ([universe][8192] u32). The expectations are host.census of those states (and of the oracle's
// states of the glider universe), written by tests/test_js_census.py.
"use strict";
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

function typed(Type, buf) { return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length)); }
function plain(list) { return list.map((o) => ({ population: o.population, firstCell: o.firstCell, boxMin: o.boxMin, boxMax: o.boxMax, digest: o.digest.toString() })); }

function main()
{
	const dir = process.argv[2];
	const want = JSON.parse(fs.readFileSync(path.join(dir, "expected.json"), "utf8"));
	const states = typed(Uint32Array, fs.readFileSync(path.join(dir, "states.bin")));
	const B = want.universes, M = want.maxComponents;
	assert.strictEqual(states.length, B * c.ENSEMBLE_WORDS);

	const ens = new c.Ensemble(0);
	assert.throws(() => ens.census(0, 1, M), /ca3d error -2/); // not configured
	ens.configure(B, 64, "moore");
	assert.throws(() => ens.census(), /ca3d error -2.*universe 0/); // no states yet
	ens.uploadState(0, states); // no rules: a census needs none
	const got = ens.census(0, B, M);
	assert.deepStrictEqual([got.components.length, got.nComponents.length, got.remaining.length], [B, B, B]);
	for (let u = 0; u < B; u++)
	{
		assert.deepStrictEqual(plain(got.components[u]), want.lists[u], "universe " + u);
		assert.deepStrictEqual([got.nComponents[u], got.remaining[u]], [want.lists[u].length, 0], "universe " + u);
	}
	assert.ok(got.gpuMs > 0);
	// a sub-range and a truncated list: the corners universe holds eight components
	const sub = ens.census(want.corners, 1, 3);
	assert.deepStrictEqual(plain(sub.components[0]), want.lists[want.corners].slice(0, 3));
	assert.deepStrictEqual([sub.nComponents[0], sub.remaining[0]], [3, 5]);
	assert.strictEqual(ens.census().components.length, B); // defaults: every universe, 64 components
	assert.throws(() => ens.census(0, 0, M), /ca3d error -1/);
	assert.throws(() => ens.census(1, B, M), /ca3d error -1/);
	assert.throws(() => ens.census(0, B, 0), /ca3d error -1/);
	assert.throws(() => ens.census(0, B, 1025), /ca3d error -1/);

	// what it is for: the glider beside a block, census after census
	const g = want.glider;
	ens.setRuleStrings(c.ENSEMBLE_ALL, { neighbourhood: "moore", born: g.born, survive: g.survive });
	for (let k = 0; k < g.lists.length; k++)
	{
		if (k) ens.step(g.every);
		const r = ens.census(g.universe, 1, M);
		assert.deepStrictEqual(plain(r.components[0]), g.lists[k], "glider, census " + k);
		assert.strictEqual(r.remaining[0], 0);
	}
	ens.close();
	console.log("ok");
}

main();
