// GPU check of the windows from Node.js. argv[2]: a directory with expected.json — {gridSize, cut: [[universe, [x, y, z]]], stamp: the
// same, modes} — grid.bin (the engine's state), soups.bin ([3][8192] u32), cut.bin (universes 0 .. 2 after the cut) and
// stamp_<mode>.bin (the engine's state after the stamp of the soups in that mode). The expectations are host.cut_window /
// host.stamp_windows of those words, written by tests/test_js_windows.py.
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
	const read = (name) => typed(Uint32Array, fs.readFileSync(path.join(dir, name)));
	const grid = read("grid.bin"), soups = read("soups.bin");
	const G = want.gridSize;
	assert.deepStrictEqual(c.STAMP_MODES, want.modes);
	assert.deepStrictEqual(c.windowTiling(128).length, 8);
	assert.deepStrictEqual(c.windowTiling(G).slice(0, 3), [[0, 0, 0], [64, 0, 0], [0, 64, 0]]);

	const eng = new c.Engine(0), ens = new c.Ensemble(0);
	assert.throws(() => eng.cutWindows(ens, want.cut), /ca3d error -2.*engine/); // not configured
	eng.configure(G);
	eng.setRuleStrings();
	assert.throws(() => eng.cutWindows(ens, want.cut), /ca3d error -2.*ensemble/);
	ens.configure(3, 64);
	assert.throws(() => eng.cutWindows(ens, want.cut), /ca3d error -2.*no state/);
	eng.uploadState(grid);

	// one cut: three windows that wrap, into universes out of order
	const ms = eng.cutWindows(ens, want.cut);
	assert.ok(ms > 0);
	assert.deepStrictEqual(ens.readState(), read("cut.bin"));
	ens.summaries().forEach((s) => assert.deepStrictEqual([s.step, s.hasPrevious], [0, false]));
	assert.deepStrictEqual(eng.readState(), grid); // the engine is only read
	assert.throws(() => eng.cutWindows(ens, [[0, [0, 0, 0]], [0, [1, 1, 1]]]), /ca3d error -1.*window 1/); // one destination twice
	assert.throws(() => eng.cutWindows(ens, [[0, [G, 0, 0]]]), /ca3d error -1.*window 0.*origin/);
	assert.throws(() => eng.cutWindows(ens, []), /ca3d error -1/);
	assert.throws(() => eng.cutWindows(ens, [[0, [0, 0]]]), RangeError);

	// one overlapping stamp a mode, each from the same state; the flat form of the windows once
	ens.uploadState(0, soups);
	for (const mode of want.modes)
	{
		eng.uploadState(grid);
		eng.step(1);
		const windows = mode === "erase" ? Uint32Array.from(want.stamp.flatMap(([u, at]) => [u, ...at])) : want.stamp;
		assert.ok(eng.stampWindows(ens, windows, mode) > 0);
		assert.strictEqual(eng.info().step, 1); // the step counter stays
		eng.uploadState(grid);
		assert.ok(eng.stampWindows(ens, windows, mode) > 0);
		assert.deepStrictEqual(eng.readState(), read("stamp_" + mode + ".bin"), mode);
		assert.strictEqual(eng.summary().hasPrevious, false);
	}
	assert.deepStrictEqual(ens.readState(), soups); // the ensemble is only read
	assert.throws(() => eng.stampWindows(ens, want.stamp, "xor"), /unknown mode/);
	assert.throws(() => eng.stampWindows(ens, [[3, [0, 0, 0]]]), /ca3d error -1.*window 0/);
	eng.close();
	ens.close();
	console.log("ok");
}

main();
