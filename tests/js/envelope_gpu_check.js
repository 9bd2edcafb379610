// GPU check of the ensemble's envelope over a period from Node.js. argv[2]: a directory with expected.json — {neighbourhood, rules: per
// universe {born, survive}, periods, records: per universe what Ensemble.envelope returns, images: the names asked for} —, states.bin
// ([universe][8192] u32) and images.bin ([universe][image][8192] u32, in the documented order). The expectations are host.envelope of
// those states, written by tests/test_js_envelope.py.
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
	const B = want.periods.length, n = want.images.length;
	assert.strictEqual(states.length, B * c.ENSEMBLE_WORDS);
	assert.strictEqual(images.length, B * n * c.ENSEMBLE_WORDS);

	const ens = new c.Ensemble(0), nursery = new c.Ensemble(0);
	assert.throws(() => ens.envelope(want.periods), /ca3d error -2.*configure/); // not configured
	ens.configure(B, 64, want.neighbourhood);
	assert.throws(() => ens.envelope(want.periods), /ca3d error -2.*universe 0/); // no states yet
	ens.uploadState(0, states);
	assert.throws(() => ens.envelope(want.periods), /ca3d error -2.*set_rules.*universe 0/); // no rules yet
	want.rules.forEach((r, u) => ens.setRuleStrings(u, { neighbourhood: want.neighbourhood, born: r.born, survive: r.survive }));

	const got = ens.envelope(want.periods);
	assert.ok(got.gpuMs > 0);
	assert.deepStrictEqual(got.records, want.records);
	// over a range, and with one period for all from `first` on
	assert.deepStrictEqual(ens.envelope(want.periods.slice(1), { first: 1 }).records, want.records.slice(1));
	assert.deepStrictEqual(ens.envelope(want.periods[B - 1], { first: B - 1 }).records, want.records.slice(B - 1));

	// the images, into a second ensemble, with the rules
	nursery.configure(1 + B * n, 64, want.neighbourhood);
	const withImages = ens.envelope(want.periods, { dst: nursery, dstFirst: 1, images: want.images, copyRules: true });
	assert.deepStrictEqual(withImages.records, want.records);
	assert.deepStrictEqual(nursery.readState(1, B * n), images);
	assert.strictEqual(nursery.summaries(1, 1)[0].step, 0);
	assert.deepStrictEqual(ens.readState(), states); // the call only reads
	assert.strictEqual(ens.summaries()[0].step, 0);

	assert.throws(() => ens.envelope(want.periods, { first: 1 }), /ca3d error -1.*universes/); // a range past n
	assert.throws(() => ens.envelope([]), /ca3d error -1.*universes/);
	assert.throws(() => ens.envelope(want.periods.map(() => 0)), /ca3d error -1.*periods\[0\]/);
	assert.throws(() => ens.envelope(4097), /ca3d error -1.*periods\[0\]/);
	assert.throws(() => ens.envelope(want.periods, { images: ["rotor"] }), /ca3d error -1.*dst is NULL/);
	assert.throws(() => ens.envelope(want.periods, { dst: nursery }), /ca3d error -1.*no image/);
	assert.throws(() => ens.envelope(want.periods, { dst: nursery, images: ["halo"] }), /unknown image/);
	nursery.close();
	ens.close();
	console.log("ok");
}

main();
