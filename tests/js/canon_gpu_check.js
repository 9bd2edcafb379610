// GPU check of the ensemble's canon from Node.js. argv[2]: a directory with expected.json — {universes, orientations, records: per
// universe {key, symmetry (decimal strings), orientation, population, boxMin, boxMax}, digests: per universe 48 decimal strings} — and
// states.bin ([universe][8192] u32; universes 0 .. 2 hold one shape at three places). The expectations are host.canon of those states,
// written by tests/test_js_canon.py.
"use strict";
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

function typed(Type, buf) { return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length)); }
function plain(r) { return { key: r.key.toString(), symmetry: r.symmetry.toString(), orientation: r.orientation, population: r.population, boxMin: r.boxMin, boxMax: r.boxMax }; }

function main()
{
	const dir = process.argv[2];
	const want = JSON.parse(fs.readFileSync(path.join(dir, "expected.json"), "utf8"));
	const states = typed(Uint32Array, fs.readFileSync(path.join(dir, "states.bin")));
	const B = want.universes;
	assert.strictEqual(states.length, B * c.ENSEMBLE_WORDS);

	const ens = new c.Ensemble(0);
	assert.throws(() => ens.canon(), /ca3d error -2.*configure/); // not configured
	ens.configure(B, 64, "moore");
	assert.throws(() => ens.canon(), /ca3d error -2.*universe 0/); // no states yet
	ens.uploadState(0, states);

	const got = ens.canon({ digests: true });
	assert.ok(got.gpuMs > 0);
	assert.deepStrictEqual(got.records.map(plain), want.records);
	assert.deepStrictEqual(got.digests.map((d) => d.map(String)), want.digests);
	assert.strictEqual(typeof got.records[0].key, "bigint");
	assert.strictEqual(got.records[3].symmetry, (1n << 48n) - 1n); // the empty universe
	// without digests, over a range
	const part = ens.canon({ first: 1, count: 2 });
	assert.strictEqual(part.digests, undefined);
	assert.deepStrictEqual(part.records.map(plain), want.records.slice(1, 3));
	assert.deepStrictEqual(ens.readState(), states); // the call only reads

	// the shape turned on the device: one key
	const stage = new c.Ensemble(0);
	stage.configure(want.orientations.length, 64, "moore");
	stage.compose(want.orientations.map((o) => [[1, o, [20, 30, 40]]]), { src: ens, copyRules: false });
	const turned = stage.canon({ digests: true });
	turned.records.forEach((r, k) =>
	{
		assert.strictEqual(r.key.toString(), want.records[1].key, "orientation " + want.orientations[k]);
		assert.strictEqual(r.symmetry, 1n);
		assert.deepStrictEqual(turned.digests[k].map(String).sort(), want.digests[1].slice().sort());
	});
	assert.strictEqual(new Set(turned.digests.map((d) => d[0])).size, want.orientations.length); // six different census digests

	assert.throws(() => ens.canon({ first: 1, count: B }), /ca3d error -1.*universes/); // a range past n
	assert.throws(() => ens.canon({ count: 0 }), /ca3d error -1.*universes/);
	ens.close();
	stage.close();
	console.log("ok");
}

main();
