// GPU check of the torus census and isolate from Node.js. argv[2]: a directory with expected.json — {universes, maxComponents, torus:
// per universe [{population, firstCell, boxMin, boxMax, digest (decimal string)}], closed: the same under the closed cube, job:
// {universe, cell, placements: {name: {population, shift}}}} — states.bin ([universe][8192] u32) and isolated.bin ([placement][8192]
// u32, in the order of job.order). The expectations are host.census and host.isolate of those states, written by
// tests/test_js_census_torus.py.
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
	const isolated = typed(Uint32Array, fs.readFileSync(path.join(dir, "isolated.bin")));
	const B = want.universes, M = want.maxComponents;
	assert.deepStrictEqual(c.CONNECTIVITIES, ["closed", "torus"]);

	const ens = new c.Ensemble(0);
	ens.configure(B, 64, "moore");
	ens.uploadState(0, states);
	const lists = (r) => r.components.map(plain);
	assert.deepStrictEqual(lists(ens.census(0, B, M, { connectivity: "torus" })), want.torus);
	assert.deepStrictEqual(lists(ens.census(0, B, M, { connectivity: "closed" })), want.closed);
	assert.deepStrictEqual(lists(ens.census(0, B, M)), want.closed); // the default is the census as it was
	assert.deepStrictEqual(lists(ens.census(0, B, M, { connectivity: "boundary" })), want.closed);
	ens.setBoundary("torus");
	assert.deepStrictEqual(lists(ens.census(0, B, M, { connectivity: "boundary" })), want.torus);
	assert.deepStrictEqual(lists(ens.census(0, B, M)), want.closed); // whatever the boundary
	assert.throws(() => ens.census(0, B, M, { connectivity: "open" }), /unknown connectivity/);
	assert.throws(() => ens._a.ensembleCensus(ens._e, 0, 1, 1, new Uint32Array(8), new Uint32Array(1), new Uint32Array(1), 2), /ca3d error -1.*connectivity 2/);

	// isolate: the seam-crossing object arrives in one piece
	const nursery = new c.Ensemble(0);
	nursery.configure(1, 64, "moore");
	const job = want.job;
	job.order.forEach((placement, i) =>
	{
		const r = nursery.isolate([[job.universe, job.cell]], { src: ens, placement, copyRules: false, connectivity: "torus" });
		assert.deepStrictEqual([r.population[0], Array.from(r.shift)], [job.placements[placement].population, job.placements[placement].shift], placement);
		assert.deepStrictEqual(nursery.readState(0, 1), isolated.subarray(i * c.ENSEMBLE_WORDS, (i + 1) * c.ENSEMBLE_WORDS), placement);
	});
	const viaBoundary = nursery.isolate([[job.universe, job.cell]], { src: ens, placement: "centre", copyRules: false, connectivity: "boundary" });
	assert.strictEqual(viaBoundary.population[0], job.placements.centre.population);
	const fragment = nursery.isolate([[job.universe, job.cell]], { src: ens, placement: "centre", copyRules: false });
	assert.ok(fragment.population[0] < job.placements.centre.population); // the closed cube cuts it at the face
	assert.throws(() => nursery.isolate([[0, 0]], { src: ens, connectivity: "open" }), /unknown connectivity/);
	nursery.close();
	ens.close();
	console.log("ok");
}

main();
