// GPU check of the ensemble's damage spreading from Node.js. argv[2]: a directory with expected.json — {neighbourhood, rules: per
// universe {born, survive}, steps, twins (a universe or null) and flips (cells [x, y, z]) per SOURCE universe, the first steps.length
// universes, records and curves: per source what Ensemble.damage returns} —, states.bin ([universe][8192] u32) and images.bin
// ([source][8192] u32, the last differences). The expectations are host.damage of those states, written by tests/test_js_damage.py.
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
	const images = typed(Uint32Array, fs.readFileSync(path.join(dir, "images.bin")));
	const B = want.rules.length, n = want.steps.length;
	assert.strictEqual(states.length, B * c.ENSEMBLE_WORDS);
	assert.strictEqual(images.length, n * c.ENSEMBLE_WORDS);
	const how = { twins: want.twins, flips: want.flips };

	const ens = new c.Ensemble(0), nursery = new c.Ensemble(0);
	assert.throws(() => ens.damage(want.steps, how), /ca3d error -2.*configure/); // not configured
	ens.configure(B, 64, want.neighbourhood);
	assert.throws(() => ens.damage(want.steps, how), /ca3d error -2.*universe 0/); // no states yet
	ens.uploadState(0, states);
	assert.throws(() => ens.damage(want.steps, how), /ca3d error -2.*set_rules.*universe 0/); // no rules yet
	want.rules.forEach((r, u) => ens.setRuleStrings(u, { neighbourhood: want.neighbourhood, born: r.born, survive: r.survive }));

	const got = ens.damage(want.steps, Object.assign({ curve: true }, how));
	assert.ok(got.gpuMs > 0);
	assert.deepStrictEqual(got.records, want.records);
	assert.deepStrictEqual(got.curve.map((row) => Array.from(row)), want.curves);
	assert.strictEqual(ens.damage(want.steps, how).curve, undefined);
	// over a range, and with one step count for all from `first` on
	const tail = { first: 1, twins: want.twins.slice(1), flips: want.flips.slice(1) };
	assert.deepStrictEqual(ens.damage(want.steps.slice(1), tail).records, want.records.slice(1));
	assert.deepStrictEqual(ens.damage(want.steps[n - 1], { first: B - 1 }).records.length, 1);

	// the images, into a second ensemble, with the rules
	nursery.configure(1 + n, 64, want.neighbourhood);
	const withImage = ens.damage(want.steps, Object.assign({ dst: nursery, dstFirst: 1, image: true, copyRules: true }, how));
	assert.deepStrictEqual(withImage.records, want.records);
	assert.deepStrictEqual(nursery.readState(1, n), images);
	assert.strictEqual(nursery.summaries(1, 1)[0].step, 0);
	assert.deepStrictEqual(ens.readState(), states); // the call only reads
	assert.strictEqual(ens.summaries()[0].step, 0);

	assert.throws(() => ens.damage(want.steps, { first: B - 1 }), /ca3d error -1.*universes/); // a range past n
	assert.throws(() => ens.damage([]), /ca3d error -1.*universes/);
	assert.throws(() => ens.damage(want.steps.map(() => 0)), /ca3d error -1.*steps\[0\]/);
	assert.throws(() => ens.damage(4097), /ca3d error -1.*steps\[0\]/);
	assert.throws(() => ens.damage(want.steps, { twins: want.steps.map(() => B) }), /ca3d error -1.*twins\[0\]/);
	assert.throws(() => ens.damage(want.steps, { image: true }), /ca3d error -1.*dst is NULL/);
	assert.throws(() => ens.damage(want.steps, { dst: nursery }), /ca3d error -1.*no image/);
	assert.throws(() => ens.damage(want.steps, { flips: want.steps.map(() => [[64, 0, 0]]) }), /inside the 64\^3 universe/);
	nursery.close();
	ens.close();
	console.log("ok");
}

main();
