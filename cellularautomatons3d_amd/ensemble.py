"""`Ensemble`: many independent 64^3 universes stepped side by side by one kernel launch (`ca3d_ensemble_*`, include/ca3d.h).

Every universe has its own rule (a table pair of the ensemble's neighbourhood, von Neumann or Moore, or — clustered — three pairs: main, edges, corners), its own step counter, its own summary record and — in `step_until` — its own moment
to stop. No reference counterpart: its UI runs one grid.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _capi, host
from ._capi import ENSEMBLE_ALL, ENSEMBLE_WORDS, RenderStats, Stats
from .engine import STOP_EXTINCT, STOP_MOVING, STOP_PERIODIC, STOP_STILL, Summary, _as_i32, _as_u32, _seed_spec, _summary

_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)

ALL = ENSEMBLE_ALL
NEIGHBOURHOODS = ("von neumann", "moore")  # index = enum ca3d_ensemble_neighbourhood
BOUNDARIES = ("reference", "torus", "closed")  # index = enum ca3d_ensemble_boundary


class Ensemble:
    """One ensemble = one GPU, one HIP stream, `n` universes of 64^3 cells (8192 packed words each)."""

    def __init__(self, device: int = 0):
        self._lib = _capi.load()
        h = C.c_void_p()
        _capi.check(self._lib.ca3d_ensemble_create(int(device), C.byref(h)))
        self._h = h
        self.n = 0
        self.grid_size = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ca3d_ensemble_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def configure(self, n: int, grid_size: int = 64, neighbourhood: str = "von neumann", clustered: bool = False) -> None:
        """`neighbourhood`: "von neumann" or "moore" — of every universe; the rules set afterwards must be of that kind.
        `clustered` (Moore only): every universe carries edges and corners table pairs beside its main one, the reference's clustered rule.
        Every configure goes back to the "reference" boundary; `set_boundary` chooses another afterwards."""
        if neighbourhood not in NEIGHBOURHOODS:
            raise ValueError(f"unknown ensemble neighbourhood {neighbourhood!r}: one of {NEIGHBOURHOODS}")
        if clustered and neighbourhood != "moore":
            raise ValueError(f"a clustered ensemble's main list is Moore (got neighbourhood {neighbourhood!r})")
        if clustered:
            _capi.check(self._lib.ca3d_ensemble_configure_clustered(self._h, grid_size, n))
        else:
            _capi.check(self._lib.ca3d_ensemble_configure_neighbourhood(self._h, grid_size, n, NEIGHBOURHOODS.index(neighbourhood)))
        self.n, self.grid_size = n, grid_size

    def set_boundary(self, name: str) -> None:
        """`ca3d_ensemble_set_boundary`: what the steps queued from now on see behind a universe's six faces — "reference" (- faces
        dead, + faces wrap: the default), "torus" (all wrap) or "closed" (all dead); `host.ensemble_step` is the definition. Moves nothing
        and waits for nothing; `canon_period` is refused while the mode is not "reference"."""
        if name not in BOUNDARIES:
            raise ValueError(f"unknown ensemble boundary {name!r}: one of {BOUNDARIES}")
        _capi.check(self._lib.ca3d_ensemble_set_boundary(self._h, BOUNDARIES.index(name)))

    @property
    def boundary(self) -> str:
        """The boundary the next step runs under (`Ca3dError` -2 before `configure`)."""
        out = C.c_int()
        _capi.check(self._lib.ca3d_ensemble_get_boundary(self._h, C.byref(out)))
        return BOUNDARIES[out.value]

    @property
    def neighbourhood(self) -> str:
        """The configured neighbourhood (`Ca3dError` -2 before `configure`)."""
        nb = C.c_int()
        _capi.check(self._lib.ca3d_ensemble_get_neighbourhood(self._h, C.byref(nb)))
        return NEIGHBOURHOODS[nb.value]

    @property
    def clustered(self) -> bool:
        """Whether the ensemble was configured clustered (`Ca3dError` -2 before `configure`)."""
        out = C.c_int()
        _capi.check(self._lib.ca3d_ensemble_get_clustered(self._h, C.byref(out)))
        return bool(out.value)

    def set_rules(self, u: int, main_offsets, edges_offsets, corners_offsets, survive, born) -> None:
        """The payload of `Engine.set_rules` for universe `u` (`ensemble.ALL`: every universe)."""
        m, e, c = _as_i32(main_offsets), _as_i32(edges_offsets), _as_i32(corners_offsets)
        s, b = _as_u32(survive), _as_u32(born)
        if s.size != _capi.LUT_LEN or b.size != _capi.LUT_LEN:
            raise ValueError("survive/born must hold 81 entries")
        _capi.check(self._lib.ca3d_ensemble_set_rules(
            self._h, u, m.ctypes.data_as(_i32p), m.size, e.ctypes.data_as(_i32p), e.size,
            c.ctypes.data_as(_i32p), c.size, s.ctypes.data_as(_u32p), b.ctypes.data_as(_u32p)))

    def set_rule_strings(self, u: int, born: str = host.DEFAULTS["bornRulesString"], survive: str = host.DEFAULTS["surviveRulesString"],
                         neighbourhood: str = "von neumann", born_edges: str = "27", survive_edges: str = "27",
                         born_corners: str = "27", survive_corners: str = "27") -> None:
        b, s = host.recalculate_rules_values(born, survive, born_edges, survive_edges, born_corners, survive_corners)
        self.set_rules(u, host.NEIGHBOURHOOD_MAP[neighbourhood], host.NEIGHBOURHOOD_MAP["edges"], host.NEIGHBOURHOOD_MAP["corners"], s, b)

    def upload_state(self, first: int, words) -> None:
        """`words`: [count, 8192] (or flat): the states of universes first .. first + count - 1."""
        w = _as_u32(words).ravel()
        if w.size == 0 or w.size % ENSEMBLE_WORDS:
            raise ValueError("a universe holds 8192 words")
        _capi.check(self._lib.ca3d_ensemble_upload_state(self._h, first, w.size // ENSEMBLE_WORDS, w.ctypes.data_as(_u32p), w.size))

    def seed_states(self, first: int, seeds, and_rounds=0, box=None, count: Optional[int] = None) -> None:
        """`ca3d_ensemble_seed_state`: universe first + k becomes `host.seeded_state(64, seeds[k], and_rounds[k], box)`, written on the
        device. `seeds` / `and_rounds`: arrays (one entry per universe) or scalars, which broadcast; all scalars: ONE spec for `count`
        universes (default: all from `first`). A scalar beside an array broadcasts per universe (one spec each, the
        scalar repeated); `count` is only needed in the all-scalar form. `box`: one for all. Records restart at step 0; the fill may still be running on return."""
        sd, ar = np.atleast_1d(np.asarray(seeds, dtype=np.uint64)), np.atleast_1d(np.asarray(and_rounds, dtype=np.uint64))
        scalar = np.ndim(seeds) == 0 and np.ndim(and_rounds) == 0
        if scalar:
            count = self.n - first if count is None else count
            specs = (_capi.SeedStruct * 1)(_seed_spec(64, int(sd[0]), int(ar[0]), box))
        else:
            n = max(sd.size, ar.size)
            if count is not None and count != n:
                raise ValueError("count does not match the per-universe arrays")
            sd, ar, count = np.broadcast_to(sd, n), np.broadcast_to(ar, n), n
            specs = (_capi.SeedStruct * n)(*[_seed_spec(64, int(a), int(b), box) for a, b in zip(sd, ar)])
        _capi.check(self._lib.ca3d_ensemble_seed_state(self._h, first, count, specs, len(specs)))

    def set_rule_tables(self, first: int, born_masks, survive_masks, count: Optional[int] = None) -> None:
        """`ca3d_ensemble_set_rule_tables`: rules as masks (bit c = born / survive at count c; c in 0..6, Moore ensembles 0..26) for universes from
        `first`, in one call. Arrays: one pair per universe (a scalar beside an array is repeated per universe); two scalars: that pair
        for `count` universes (default: all from `first`). Waits for the stream, as `set_rules` does."""
        b, s = np.atleast_1d(_as_u32(born_masks)), np.atleast_1d(_as_u32(survive_masks))
        if np.ndim(born_masks) == 0 and np.ndim(survive_masks) == 0:
            count = self.n - first if count is None else count
        else:
            n = max(b.size, s.size)
            if count is not None and count != n:
                raise ValueError("count does not match the per-universe arrays")
            b, s, count = np.ascontiguousarray(np.broadcast_to(b, n)), np.ascontiguousarray(np.broadcast_to(s, n)), n
        _capi.check(self._lib.ca3d_ensemble_set_rule_tables(self._h, first, count, b.ctypes.data_as(_u32p), s.ctypes.data_as(_u32p), b.size))

    def set_clustered_tables(self, first: int, born_masks, survive_masks, count: Optional[int] = None) -> None:
        """`ca3d_ensemble_set_rule_tables_clustered`: a rule is three masks — main (bits 0..26), edges (0..12), corners (0..8). `[n, 3]`
        arrays: one rule per universe from `first`; two length-3 rows: that rule for `count` universes (default: all from `first`)."""
        b, s = np.ascontiguousarray(_as_u32(born_masks)), np.ascontiguousarray(_as_u32(survive_masks))
        if b.shape != s.shape or b.ndim not in (1, 2) or b.shape[-1] != 3:
            raise ValueError("born_masks / survive_masks: two [n, 3] arrays or two length-3 rows (main, edges, corners)")
        if b.ndim == 1:
            count, n_rules = (self.n - first if count is None else count), 1
        else:
            if count is not None and count != b.shape[0]:
                raise ValueError("count does not match the per-universe arrays")
            count = n_rules = b.shape[0]
        _capi.check(self._lib.ca3d_ensemble_set_rule_tables_clustered(self._h, first, count, b.ctypes.data_as(_u32p), s.ctypes.data_as(_u32p), n_rules))

    def read_state(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n - first if count is None else count
        out = np.empty((count, ENSEMBLE_WORDS), dtype=np.uint32)
        _capi.check(self._lib.ca3d_ensemble_read_state(self._h, first, count, out.ctypes.data_as(_u32p), out.size))
        return out

    def step(self, n_steps: int = 1) -> None:
        """Every universe, unconditionally; asynchronous."""
        _capi.check(self._lib.ca3d_ensemble_step(self._h, n_steps))

    def step_until(self, max_steps: int, check_every: int = 8, stop_mask: int = STOP_EXTINCT | STOP_STILL) -> Tuple[np.ndarray, np.ndarray]:
        """`Engine.step_until` per universe, decided inside the kernel -> (steps_done u32[n], reason u32[n])."""
        done, reason = np.empty(self.n, dtype=np.uint32), np.empty(self.n, dtype=np.uint32)
        _capi.check(self._lib.ca3d_ensemble_step_until(self._h, max_steps, check_every, stop_mask, done.ctypes.data_as(_u32p),
                                                       reason.ctypes.data_as(_u32p)))
        return done, reason

    def step_until_cycle(self, max_steps: int, check_every: int = 8,
                         stop_mask: int = STOP_EXTINCT | STOP_STILL | STOP_PERIODIC) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`Engine.step_until_cycle` per universe, decided inside the kernel -> (steps_done u32[n], reason u32[n], period u32[n])."""
        done, reason, period = (np.empty(self.n, dtype=np.uint32) for _ in range(3))
        _capi.check(self._lib.ca3d_ensemble_step_until_cycle(self._h, max_steps, check_every, stop_mask, done.ctypes.data_as(_u32p),
                                                             reason.ctypes.data_as(_u32p), period.ctypes.data_as(_u32p)))
        return done, reason, period

    def step_until_moving(self, max_steps: int, check_every: int = 8,
                          stop_mask: int = STOP_EXTINCT | STOP_STILL | STOP_PERIODIC | STOP_MOVING) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """`step_until_cycle` that also stops a universe whose state at a check point is its anchor state translated by a vector
        d != 0, both clear of the faces (`ca3d_ensemble_step_until_moving`, STOP_MOVING): a glider or spaceship, decided inside the kernel
        and exact -> (steps_done u32[n], reason u32[n], period u32[n], shift i32[n, 3]). `period` is a multiple of the ship's period,
        `shift[u]` = (dx, dy, dz) its displacement over `period`, zero unless STOP_MOVING is in `reason[u]`."""
        done, reason, period = (np.empty(self.n, dtype=np.uint32) for _ in range(3))
        shift = np.empty((self.n, 3), dtype=np.int32)
        _capi.check(self._lib.ca3d_ensemble_step_until_moving(self._h, max_steps, check_every, stop_mask, done.ctypes.data_as(_u32p),
                                                              reason.ctypes.data_as(_u32p), period.ctypes.data_as(_u32p),
                                                              shift.ctypes.data_as(_i32p)))
        return done, reason, period, shift

    def step_trace(self, max_steps: int, check_every: int = 8,
                   stop_mask: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """`step_until` that records every universe's population curve inside the kernel (`ca3d_ensemble_step_until_trace`): one sample
        (population, births, deaths) per check point, K = `host.trace_samples(max_steps, check_every)` of them at most
        -> (samples u32[n, K, 3], n_samples u32[n], steps_done u32[n], reason u32[n]). Slots past n_samples[u] are zero. `stop_mask`:
        STOP_EXTINCT | STOP_STILL bits; 0 (the default): nothing stops and every universe has K samples."""
        if self.n == 0 or check_every < 1:  # no K to size the array with: the library names the error
            _capi.check(self._lib.ca3d_ensemble_step_until_trace(self._h, max_steps, check_every, stop_mask, None, None, None, 0, None))
        k = host.trace_samples(max_steps, check_every)
        samples = np.zeros((self.n, k, 3), dtype=np.uint32)
        count, done, reason = (np.empty(self.n, dtype=np.uint32) for _ in range(3))
        _capi.check(self._lib.ca3d_ensemble_step_until_trace(self._h, max_steps, check_every, stop_mask, done.ctypes.data_as(_u32p),
                                                             reason.ctypes.data_as(_u32p), samples.ctypes.data_as(_u32p), k,
                                                             count.ctypes.data_as(_u32p)))
        return samples, count, done, reason

    def summaries(self, first: int = 0, count: Optional[int] = None) -> List[Summary]:
        """The universes' records (no per-plane counts): copied, not computed — every launch leaves them up to date."""
        count = self.n - first if count is None else count
        recs = (_capi.SummaryStruct * count)()
        _capi.check(self._lib.ca3d_ensemble_summarize(self._h, first, count, recs))
        return [_summary(r, None) for r in recs]

    def _connectivity(self, name: str) -> int:
        """CA3D_CONNECT_* of "closed", "torus" or "boundary" (torus when this ensemble's boundary is "torus", closed otherwise)."""
        if name == "boundary":
            name = "torus" if self.boundary == "torus" else "closed"
        if name not in _capi.CONNECTIVITIES:
            raise ValueError(f"unknown connectivity {name!r}: one of {tuple(_capi.CONNECTIVITIES) + ('boundary',)}")
        return _capi.CONNECTIVITIES[name]

    def census(self, first: int = 0, count: Optional[int] = None, max_components: int = 64,
               connectivity: str = "closed") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`ca3d_ensemble_census`: the connected objects (26-neighbourhood inside the closed cube) of universes first .. first + count - 1
        (default: all from `first`), found on the device in one launch behind the queued steps
        -> (components [count, max_components] of `host.COMPONENT_DTYPE`, n_components u32[count], remaining u32[count]).
        Components come in the order of their first cells; slots past n_components[u] are zero; remaining[u] counts the live cells in no
        listed component (0: the list is complete). `host.census` is the same on the CPU, `host.unpack_box` opens box_min / box_max.
        The call only reads; `census_gpu_ms()` tells what the launch took.
        `connectivity` (`ca3d_ensemble_census_connected`): "closed" as above; "torus": cells are adjacent modulo 64, an object on a
        face is one object, box_min starts its cyclic box and box_max = box_min + extent - 1 is not reduced (>= 64 through a seam);
        "boundary": torus when this ensemble's boundary is "torus", closed otherwise."""
        connect = self._connectivity(connectivity)
        count = self.n - first if count is None else count
        comps = np.zeros((max(count, 0), max(max_components, 0)), dtype=host.COMPONENT_DTYPE)
        n, rest = (np.zeros(max(count, 0), dtype=np.uint32) for _ in range(2))
        ms = C.c_float(0.0)
        _capi.check(self._lib.ca3d_ensemble_census_connected(self._h, first, count, max_components, connect,
                                                             comps.ctypes.data_as(C.POINTER(_capi.ComponentStruct)),
                                                             n.ctypes.data_as(_u32p), rest.ctypes.data_as(_u32p), C.byref(ms)))
        self._census_ms = float(ms.value)
        return comps, n, rest

    def census_gpu_ms(self) -> float:
        """hipEvent time of the last `census` launch of this object, in milliseconds (None before the first)."""
        return getattr(self, "_census_ms", None)

    def isolate(self, jobs, dst_first: int = 0, src: Optional["Ensemble"] = None, placement: str = "centre",
                copy_rules: bool = True, connectivity: str = "closed") -> Tuple[np.ndarray, np.ndarray]:
        """`ca3d_ensemble_isolate`: universe dst_first + k of THIS ensemble becomes the connected object of universe jobs[k][0] of `src`
        (default: this ensemble) that holds the cell jobs[k][1] (x + 64 y + 4096 z, any cell of the object — a census' first_cell
        will do), alone, translated as `placement` says ("keep", "centre", "origin"), at step 0, found and written on the device in
        one launch -> (population u32[n], shift i32[n, 3]). `copy_rules`: the destination universe takes its source universe's rule
        (both ensembles of one kind). `jobs`: [n, 2]. `host.isolate` is the same on the CPU for one universe; `isolate_gpu_ms()`
        tells what the launch took.
        `connectivity` (`ca3d_ensemble_isolate_connected`): "closed" — the object is the closed census'; "torus" — the torus census',
        moved modulo 64 so that it arrives in one piece; "boundary": torus when the SOURCE ensemble's boundary is "torus", closed
        otherwise."""
        if placement not in _capi.ISOLATE_PLACEMENTS:
            raise ValueError(f"unknown placement {placement!r}: one of {tuple(_capi.ISOLATE_PLACEMENTS)}")
        connect = (self if src is None else src)._connectivity(connectivity)
        j = np.ascontiguousarray(_as_u32(jobs))
        if j.ndim != 2 or j.shape[1] != 2:
            raise ValueError("jobs is an [n, 2] array of (universe, cell)")
        n = j.shape[0]
        out = np.zeros((n, 4), dtype=np.int32)
        ms = C.c_float(0.0)
        flags = _capi.ISOLATE_PLACEMENTS[placement] | (_capi.ISOLATE_COPY_RULES if copy_rules else 0)
        _capi.check(self._lib.ca3d_ensemble_isolate_connected(self._h, dst_first, (self if src is None else src)._h, n,
                                                              j.ctypes.data_as(C.POINTER(_capi.IsolateJobStruct)), flags, connect,
                                                              out.ctypes.data_as(C.POINTER(_capi.IsolatedStruct)), C.byref(ms)))
        self._isolate_ms = float(ms.value)
        return out[:, 0].astype(np.uint32), out[:, 1:].copy()

    def isolate_gpu_ms(self) -> float:
        """hipEvent time of the last `isolate` launch into this object, in milliseconds (None before the first)."""
        return getattr(self, "_isolate_ms", None)

    def compose(self, layouts, dst_first: int = 0, src: Optional["Ensemble"] = None, over: bool = False,
                copy_rules: bool = True) -> np.ndarray:
        """`ca3d_ensemble_compose`, the inverse of `isolate`: universe dst_first + k of THIS ensemble becomes the union of the pieces
        layouts[k], a list of (universe, orientation, (x, y, z)): the WHOLE state of that universe of `src` (default: this ensemble),
        turned by orientation 0 .. 47 (`host.orientation_matrix`) with the turned piece's box_min put at (x, y, z), -64 .. 64 each;
        cells that leave the cube are clipped. `over`: on top of the destination's current state, else from nothing; an empty list
        leaves it empty (or as it is). `copy_rules`: a destination takes the rule of its first piece's universe (both ensembles of one
        kind). One launch for all destinations, at step 0 -> records [n] of `host.COMPOSED_DTYPE` (population, placed, overlap,
        clipped). `host.compose` is the same on the CPU for one destination; `compose_gpu_ms()` tells what the launch took."""
        begin = np.zeros(len(layouts) + 1, dtype=np.uint32)
        flat = []
        for k, layout in enumerate(layouts):
            flat.extend(layout)
            begin[k + 1] = len(flat)
        parts = host.compose_parts(flat)
        out = np.zeros(len(layouts), dtype=host.COMPOSED_DTYPE)
        ms = C.c_float(0.0)
        flags = (_capi.COMPOSE_OVER if over else 0) | (_capi.COMPOSE_COPY_RULES if copy_rules else 0)
        _capi.check(self._lib.ca3d_ensemble_compose(self._h, dst_first, len(layouts), (self if src is None else src)._h,
                                                    parts.ctypes.data_as(C.POINTER(_capi.ComposePartStruct)), begin.ctypes.data_as(_u32p),
                                                    flags, out.ctypes.data_as(C.POINTER(_capi.ComposedStruct)), C.byref(ms)))
        self._compose_ms = float(ms.value)
        return out

    def compose_gpu_ms(self) -> float:
        """hipEvent time of the last `compose` launch into this object, in milliseconds (None before the first)."""
        return getattr(self, "_compose_ms", None)

    def canon(self, first: int = 0, count: Optional[int] = None, digests: bool = False):
        """`ca3d_ensemble_canon`: the name of universes first .. first + count - 1 (default: all from `first`) up to the 48 orientations
        of `compose` and any translation, found on the device in one launch behind the queued steps -> records [count] of
        `host.CANON_DTYPE`: `key`, equal for all turned and shifted copies of a state — `np.unique(rec["key"], return_counts=True)` is a
        catalogue; `orientation`, which turns the state into the one whose digest is the key; `symmetry`, bit o set when turning by o
        leaves the state as it is (`host.symmetry_orientations`, `host.is_chiral`); population, box_min, box_max as in a census record.
        The WHOLE state of a universe is named: isolate objects first. With `digests` -> (records, digests u64[count, 48]), the digest
        of every orientation. `host.canon` is the same on the CPU for one universe. The call only reads; `canon_gpu_ms()` tells what
        the launch took."""
        count = self.n - first if count is None else count
        rec = np.zeros(max(count, 0), dtype=host.CANON_DTYPE)
        dig = np.zeros((max(count, 0), 48), dtype=np.uint64) if digests else None
        ms = C.c_float(0.0)
        _capi.check(self._lib.ca3d_ensemble_canon(self._h, first, count, rec.ctypes.data_as(C.POINTER(_capi.CanonStruct)),
                                                  dig.ctypes.data_as(C.POINTER(C.c_uint64)) if digests else None, C.byref(ms)))
        self._canon_ms = float(ms.value)
        return (rec, dig) if digests else rec

    def canon_gpu_ms(self) -> float:
        """hipEvent time of the last `canon` launch of this object, in milliseconds (None before the first)."""
        return getattr(self, "_canon_ms", None)

    def canon_period(self, periods, first: int = 0, count: Optional[int] = None, keys: bool = False):
        """`ca3d_ensemble_canon_period`: universe first + k (default range: all from `first`) named over periods[k] steps of its own,
        taken INSIDE one launch behind the queued steps; the ensemble is left exactly as it is -> records [count] of
        `host.CANON_PERIOD_DTYPE`: `key`, the smallest `canon` key over the phases t = 0 .. periods[k] - 1 — all phases of all 48
        turned copies of a glider share it —, `phase`, the smallest t that reaches it, that phase's `orientation`, `symmetry` and
        `population`, and `flags_shift`: bit 0 (`host.CANON_CLOSED`) says that after periods[k] steps the state is back up to a
        translation, compared word for word — the period given is a multiple of the true one —, and `host.unpack_shift` gives the
        translation, (0, 0, 0) for an oscillator or a still life. `periods` is one number for all or one per universe, each 1 ..
        `host.CANON_MAX_PERIOD`. With `keys` -> (records, keys u64[count, max(periods)]): the key of every phase, zero past a
        universe's period. Every universe of the range needs a rule. `host.canon_period` is the same on the CPU for one universe;
        `canon_period_gpu_ms()` tells what the launch took."""
        count = self.n - first if count is None else count
        p = _as_u32(periods).ravel()
        if np.ndim(periods) == 0:
            p = np.full(max(count, 0), p[0], dtype=np.uint32)
        if p.size != max(count, 0):
            raise ValueError("periods holds one period for every universe of the range")
        stride = int(p.max()) if p.size else 0
        rec = np.zeros(p.size, dtype=host.CANON_PERIOD_DTYPE)
        # (a period the library refuses must not size an array: the call below fails before it looks at `ks`)
        ks = np.zeros((p.size, stride if stride <= host.CANON_MAX_PERIOD else 0), dtype=np.uint64) if keys else None
        ms = C.c_float(0.0)
        _capi.check(self._lib.ca3d_ensemble_canon_period(self._h, first, count, p.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                         rec.ctypes.data_as(C.POINTER(_capi.CanonPeriodStruct)),
                                                         ks.ctypes.data_as(C.POINTER(C.c_uint64)) if keys else None, stride if keys else 0,
                                                         C.byref(ms)))
        self._canon_period_ms = float(ms.value)
        return (rec, ks) if keys else rec

    def canon_period_gpu_ms(self) -> float:
        """hipEvent time of the last `canon_period` launch of this object, in milliseconds (None before the first)."""
        return getattr(self, "_canon_period_ms", None)

    def envelope(self, periods, first: int = 0, dst: Optional["Ensemble"] = None, dst_first: int = 0, images=(),
                 copy_rules: bool = False) -> np.ndarray:
        """`ca3d_ensemble_envelope`: HOW universe first + k oscillates over periods[k] steps of its own, taken INSIDE one launch behind
        the queued steps under this ensemble's rule and boundary; this ensemble is left exactly as it is -> records of
        `host.ENVELOPE_DTYPE`: `envelope_population` (cells that ever live), `stator_population` (cells that always live), `heat`
        (cells changed, summed over the steps), `population_sum`, the inclusive boxes of the envelope and of the rotor (envelope
        without stator; zero for an empty set), and `flags`: bit 0 (`host.ENVELOPE_RETURNS`) says that after periods[k] steps the
        state is back word for word. `host.envelope_derived` gives rotor population, volatility and heat per step. `periods` is one
        number for every universe from `first` on, or one per universe, each 1 .. `host.CANON_MAX_PERIOD`.
        `images`: any of "envelope", "stator", "rotor"; with n of them universe dst_first + k * n + i of `dst` (this ensemble or
        another one on the same device; required with images, None without) becomes the i-th selected image of source k, in that order,
        at step 0. `copy_rules`: each destination takes its source universe's rule (both ensembles of one kind). `host.envelope` is
        the same on the CPU for one universe; `envelope_gpu_ms()` tells what the launch took."""
        p = _as_u32(periods).ravel()
        if np.ndim(periods) == 0:
            p = np.full(max(self.n - first, 0), p[0], dtype=np.uint32)
        p = np.ascontiguousarray(p)
        flags = 0
        for name in ([images] if isinstance(images, str) else images):
            if name not in host.ENVELOPE_IMAGES:
                raise ValueError(f"unknown image {name!r}: one of {tuple(host.ENVELOPE_IMAGES)}")
            flags |= host.ENVELOPE_IMAGES[name]
        if copy_rules:
            flags |= _capi.ENVELOPE_COPY_RULES
        rec = np.zeros(p.size, dtype=host.ENVELOPE_DTYPE)
        ms = C.c_float(0.0)
        _capi.check(self._lib.ca3d_ensemble_envelope(self._h, first, p.size, p.ctypes.data_as(_u32p), None if dst is None else dst._h,
                                                     dst_first, flags, rec.ctypes.data_as(C.POINTER(_capi.EnvelopeStruct)), C.byref(ms)))
        self._envelope_ms = float(ms.value)
        return rec

    def envelope_gpu_ms(self) -> float:
        """hipEvent time of the last `envelope` launch of this object, in milliseconds (None before the first)."""
        return getattr(self, "_envelope_ms", None)

    def damage(self, steps, first: int = 0, twins=None, flips=None, dst: Optional["Ensemble"] = None, dst_first: int = 0,
               image: bool = False, copy_rules: bool = False, curve: bool = False):
        """`ca3d_ensemble_damage`: how a perturbation of universe first + k spreads over steps[k] steps — the universe and a perturbed
        twin stepped side by side INSIDE one launch behind the queued steps, under the universe's rule and this ensemble's boundary,
        and their Hamming distance d_t taken at every t = 0 .. steps[k]; this ensemble is left exactly as it is -> records of
        `host.DAMAGE_DTYPE`, or (records, curve) with `curve=True`: curve[k, t] = d_t, zero behind steps[k], max(steps) + 1 columns.
        `steps` is one number for every universe from `first` on, or one per universe, each 1 .. `host.CANON_MAX_PERIOD`.
        The twin starts as the universe itself, or as universe twins[k] of this ensemble (`host.DAMAGE_SELF`: itself), with the cells
        of flips[k] flipped: up to `host.DAMAGE_FLIPS` cells (x, y, z) a universe, a cell listed twice cancels; `flips` may also be
        one (x, y, z) for every universe, or an array [count, 4] of flip words (`host.damage_flip_word`, `host.DAMAGE_NO_FLIP`).
        `image`: universe dst_first + k of `dst` (this ensemble or another one on the same device; required with the image, None
        without) becomes the last difference S ^ T, at step 0. `copy_rules`: each destination takes its source universe's rule (both
        ensembles of one kind). `host.damage` is the same on the CPU for one universe; `damage_gpu_ms()` tells what the launch took."""
        p = _as_u32(steps).ravel()
        if np.ndim(steps) == 0:
            p = np.full(max(self.n - first, 0), p[0], dtype=np.uint32)
        p = np.ascontiguousarray(p)
        tw = None
        if twins is not None:
            tw = np.ascontiguousarray(_as_u32(twins).ravel())
            if tw.size != p.size:
                raise ValueError(f"{tw.size} twins for {p.size} universes")
        fl = None
        if flips is not None:
            if isinstance(flips, np.ndarray) and flips.dtype == np.uint32 and flips.shape == (p.size, host.DAMAGE_FLIPS):
                fl = np.ascontiguousarray(flips)
            else:
                per = list(flips)
                if len(per) == 3 and all(np.ndim(v) == 0 for v in per):
                    per = [[per]] * p.size  # one cell for every universe
                if len(per) != p.size:
                    raise ValueError(f"flips for {len(per)} universes, steps for {p.size}")
                fl = np.full((p.size, host.DAMAGE_FLIPS), host.DAMAGE_NO_FLIP, dtype=np.uint32)
                for k, cells in enumerate(per):
                    cells = list(cells)
                    if len(cells) > host.DAMAGE_FLIPS:
                        raise ValueError(f"universe {first + k}: {len(cells)} flips, at most {host.DAMAGE_FLIPS}")
                    fl[k, :len(cells)] = [host.damage_flip_word(c) for c in cells]
        flags = (_capi.DAMAGE_IMAGE_DAMAGE if image else 0) | (_capi.DAMAGE_COPY_RULES if copy_rules else 0)
        rec = np.zeros(p.size, dtype=host.DAMAGE_DTYPE)
        stride = int(p.max()) + 1 if curve and p.size else 0
        samples = np.zeros((p.size, stride), dtype=np.uint32) if curve else None
        ms = C.c_float(0.0)
        _capi.check(self._lib.ca3d_ensemble_damage(self._h, first, p.size, p.ctypes.data_as(_u32p), None if tw is None else tw.ctypes.data_as(_u32p),
                                                   None if fl is None else fl.ctypes.data_as(_u32p), None if dst is None else dst._h, dst_first, flags,
                                                   rec.ctypes.data_as(C.POINTER(_capi.DamageStruct)),
                                                   None if samples is None else samples.ctypes.data_as(_u32p), stride, C.byref(ms)))
        self._damage_ms = float(ms.value)
        return (rec, samples) if curve else rec

    def damage_gpu_ms(self) -> float:
        """hipEvent time of the last `damage` launch of this object, in milliseconds (None before the first)."""
        return getattr(self, "_damage_ms", None)

    def usage(self, steps, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """`ca3d_ensemble_usage`: WHICH entries of its rule tables universe first + k reads over steps[k] steps of its own, taken INSIDE
        one launch behind the queued steps under this ensemble's rule and boundary; this ensemble is left exactly as it is -> records
        of `host.USAGE_DTYPE`: `dead[base + c]` / `alive[base + c]`, the cells dead / alive with count c summed over the steps, per
        class (`host.USAGE_CLASSES`: main, edges, corners; von Neumann and Moore fill main only), and `used_born` / `used_survive`,
        the masks of the table bits that were read. `steps` is one number for every universe of the range (`count` universes from
        `first` on, default: to the end), or one per universe, each 1 .. `host.CANON_MAX_PERIOD`. `host.usage` is the same on the CPU
        for one universe, `host.usage_dont_care` and `host.usage_births_deaths` read a record; `usage_gpu_ms()` tells what the launch
        took."""
        p = _as_u32(steps).ravel()
        if np.ndim(steps) == 0:
            p = np.full(max(self.n - first, 0) if count is None else count, p[0], dtype=np.uint32)
        elif count is not None and count != p.size:
            raise ValueError(f"{p.size} step counts for {count} universes")
        p = np.ascontiguousarray(p)
        rec = np.zeros(p.size, dtype=host.USAGE_DTYPE)
        ms = C.c_float(0.0)
        _capi.check(self._lib.ca3d_ensemble_usage(self._h, first, p.size, p.ctypes.data_as(_u32p), rec.ctypes.data_as(C.POINTER(_capi.UsageStruct)),
                                                  C.byref(ms)))
        self._usage_ms = float(ms.value)
        return rec

    def usage_gpu_ms(self) -> float:
        """hipEvent time of the last `usage` launch of this object, in milliseconds (None before the first)."""
        return getattr(self, "_usage_ms", None)

    def canon_phases(self, periods, first: int = 0, count: Optional[int] = None,
                     max_period: int = 64) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """`canon` over a whole period, for universes already classified as oscillators or ships (`step_until_cycle`,
        `step_until_moving`): universe first + k takes the smallest key over its phases t = 0 .. periods[k] - 1
        -> (key u64[count], phase u32[count], orientation u32[count], symmetry u64[count]), with the phase, orientation and symmetry
        of the smallest t that reaches the key. All phases of all 48 turned copies of a glider then share one key. `canon_period`
        does the same in one launch, leaves the ensemble as it is and also says whether the period closes.

        WHAT IT COSTS AND CHANGES: max(periods) `canon` launches with a `step(1)` behind each. `step` has no range, so afterwards
        EVERY universe of the ensemble, inside the range or not, is max(periods) steps further — a universe of the range is back in
        its phase 0 only when max(periods) is a multiple of its period — and every universe needs rules. A ship must stay clear of
        the faces for that long: `isolate`'s centred placement leaves about 30 cells. A period of 0, or max(periods) > `max_period`,
        is a ValueError before anything is queued."""
        count = self.n - first if count is None else count
        p = np.ascontiguousarray(_as_u32(periods)).ravel()
        if p.size != count:
            raise ValueError("periods holds one period for every universe of the range")
        if p.size == 0 or int(p.min()) == 0:
            raise ValueError("a period is at least 1")
        if int(p.max()) > max_period:
            raise ValueError(f"the largest period is {int(p.max())}: more than max_period = {max_period}")
        key = np.full(count, np.iinfo(np.uint64).max, dtype=np.uint64)
        phase, orientation = (np.zeros(count, dtype=np.uint32) for _ in range(2))
        symmetry = np.zeros(count, dtype=np.uint64)
        for t in range(int(p.max())):
            rec = self.canon(first, count)
            # strictly smaller, or the first round: the smallest t that reaches the key keeps it
            better = (t < p) & ((rec["key"] < key) | (t == 0))
            key[better], phase[better] = rec["key"][better], t
            orientation[better], symmetry[better] = rec["orientation"][better], rec["symmetry"][better]
            self.step(1)
        return key, phase, orientation, symmetry

    def render_sheet(self, uniforms, tile_w: int, tile_h: int, columns: Optional[int] = None, spp: int = 1, first: int = 0,
                     count: Optional[int] = None, light: bool = False, depth: bool = False):
        """`ca3d_ensemble_render_sheet`: universes first .. first + count - 1 (default: all from `first`) as the tiles of one contact
        sheet, one launch; tile k is the frame `Engine.render(uniforms, tile_w, tile_h, spp)` draws of universe first + k at 64^3 with
        "render_skip" 0, bit for bit (`host.sheet_tile` cuts it out). `columns`: tiles per row (default ceil(sqrt(count))); the sheet
        is `host.sheet_shape(count, tile_w, tile_h, columns)`. Returns the presentation sheet u8[H, W, 4]; with `light` / `depth` a
        tuple (presentation, light f16[H, W, 4], depth f16[H, W, 2]) of the ones asked for. Fill `uniforms` with
        `host.uniform_block(tile_w, tile_h, ...)`: one block serves every tile."""
        u = np.ascontiguousarray(uniforms, dtype=np.float32)
        if u.size != 128:
            raise ValueError("the common uniform block holds 128 floats")
        count = self.n - first if count is None else count
        if columns is None:
            columns = max(1, int(np.ceil(np.sqrt(max(count, 1)))))

        def call(*out):
            _capi.check(self._lib.ca3d_ensemble_render_sheet(self._h, first, count, u.ctypes.data_as(C.POINTER(C.c_float)), tile_w, tile_h,
                                                             columns, spp, *out))

        sizable = count >= 1 and columns >= 1 and tile_w >= 1 and tile_h >= 1
        h, w = host.sheet_shape(count, tile_w, tile_h, columns) if sizable else (0, 0)
        if not sizable or h * w > 1 << 26:
            call(None, None, None)  # no sheet to size arrays for: the library refuses the call and names the reason
            raise ValueError("a sheet has at least one tile, one column and one pixel a tile, and at most 2^26 pixels")
        pres = np.empty((h, w, 4), dtype=np.uint8)
        lt = np.empty((h, w, 4), dtype=np.float16) if light else None
        dp = np.empty((h, w, 2), dtype=np.float16) if depth else None
        call(pres.ctypes.data, lt.ctypes.data if light else None, dp.ctypes.data if depth else None)
        if not (light or depth):
            return pres
        return (pres,) + ((lt,) if light else ()) + ((dp,) if depth else ())

    def sheet_stats(self) -> RenderStats:
        """The last sheet (`ca3d_ensemble_get_sheet_stats`): gpu_ms, primary_rays = count * tile_w * tile_h * spp, shadow rays and
        both cell-visit counts summed over its tiles. Waits for the sheet."""
        s = RenderStats()
        _capi.check(self._lib.ca3d_ensemble_get_sheet_stats(self._h, C.byref(s)))
        return s

    def synchronize(self) -> None:
        _capi.check(self._lib.ca3d_ensemble_synchronize(self._h))

    def stats(self) -> Stats:
        s = Stats()
        _capi.check(self._lib.ca3d_ensemble_get_stats(self._h, C.byref(s)))
        return s
