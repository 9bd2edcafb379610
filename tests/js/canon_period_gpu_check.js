// GPU check of the ensemble's canon over a period from Node.js. argv[2]: a directory with expected.json — {neighbourhood, rules: per
// universe {born, survive}, periods, records: per universe {key, symmetry (decimal strings), orientation, phase, population, closed,
// shift}, keys: per universe periods[k] decimal strings} — and states.bin ([universe][8192] u32). The expectations are
// host.canon_period of the oracle's phases of those states, written by tests/test_js_canon_period.py.
"use strict";
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..", "..");
const c = require(path.join(root, "cellularautomatons3d_amd", "js", "ca3d.js"));

function typed(Type, buf) { return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length)); }
function plain(r)
{
	return { key: r.key.toString(), symmetry: r.symmetry.toString(), orientation: r.orientation, phase: r.phase, population: r.population, closed: r.closed, shift: r.shift };
}

function main()
{
	const dir = process.argv[2];
	const want = JSON.parse(fs.readFileSync(path.join(dir, "expected.json"), "utf8"));
	const states = typed(Uint32Array, fs.readFileSync(path.join(dir, "states.bin")));
	const B = want.periods.length;
	assert.strictEqual(states.length, B * c.ENSEMBLE_WORDS);

	const ens = new c.Ensemble(0);
	assert.throws(() => ens.canonPeriod({ periods: want.periods }), /ca3d error -2.*configure/); // not configured
	ens.configure(B, 64, want.neighbourhood);
	assert.throws(() => ens.canonPeriod({ periods: want.periods }), /ca3d error -2.*universe 0/); // no states yet
	ens.uploadState(0, states);
	assert.throws(() => ens.canonPeriod({ periods: want.periods }), /ca3d error -2.*set_rules.*universe 0/); // no rules yet
	want.rules.forEach((r, u) => ens.setRuleStrings(u, { neighbourhood: want.neighbourhood, born: r.born, survive: r.survive }));

	const got = ens.canonPeriod({ periods: want.periods, keys: true });
	assert.ok(got.gpuMs > 0);
	assert.deepStrictEqual(got.records.map(plain), want.records);
	assert.deepStrictEqual(got.keys.map((k) => k.map(String)), want.keys);
	assert.strictEqual(typeof got.records[0].key, "bigint");
	// without keys, over a range, and with one period for all
	const part = ens.canonPeriod({ first: 1, periods: want.periods.slice(1, 3) });
	assert.strictEqual(part.keys, undefined);
	assert.deepStrictEqual(part.records.map(plain), want.records.slice(1, 3));
	const same = want.periods[0];
	const one = ens.canonPeriod({ periods: same, count: 1, keys: true });
	assert.deepStrictEqual(one.records.map(plain), want.records.slice(0, 1));
	assert.deepStrictEqual(one.keys[0].map(String), want.keys[0]);
	assert.deepStrictEqual(ens.readState(), states); // the call only reads
	assert.strictEqual(ens.summaries()[0].step, 0);

	assert.throws(() => ens.canonPeriod({ first: 1, periods: want.periods }), /ca3d error -1.*universes/); // a range past n
	assert.throws(() => ens.canonPeriod({ periods: [] }), /ca3d error -1.*universes/);
	assert.throws(() => ens.canonPeriod({ periods: want.periods.map(() => 0) }), /ca3d error -1.*periods\[0\]/);
	assert.throws(() => ens.canonPeriod({ periods: 4097, keys: true }), /ca3d error -1.*periods\[0\]/);
	ens.close();
	console.log("ok");
}

main();
