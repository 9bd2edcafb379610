"""Host-side surface of the CA path: rule strings, neighbourhood tables, packed state layout, seeds.

Python mirror of the reference host logic (same names, argument meaning and quirks), used by the tests and
`bench.py` above the C ABI. The JavaScript twin is `js/ca3d.js`. All citations are to
/root/reference/main_pathtraced.js.

Nothing here touches the GPU; nothing here is a CPU fallback for the kernels.
"""
from __future__ import annotations

import math
import re
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

NEIGHBOURS_STORAGE_LEN = 27  # main_pathtraced.js:10
WORK_GROUP_SIZE = 16  # main_pathtraced.js:5

# Offset tables, flat xyz triples (main_pathtraced.js:13-85). Element order is kept: the reference's kernel
# sums over them so order is irrelevant to the result, but the ABI passes them verbatim.
_VN = [1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1]
_VN2D = [1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0]
_MOORE2D = [1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0]
_MOORE = (
    _MOORE2D
    + [1, 0, 1, -1, 0, 1, 0, 1, 1, 0, -1, 1, 1, 1, 1, -1, 1, 1, 1, -1, 1, -1, -1, 1, 0, 0, 1]
    + [1, 0, -1, -1, 0, -1, 0, 1, -1, 0, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 0, 0, -1]
)
_EDGES = [1, 1, 0, -1, 1, 0, 0, 1, 1, 0, 1, -1, 1, -1, 0, -1, -1, 0, 0, -1, 1, 0, -1, -1, 1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1]
_CORNERS = [1, 1, 1, -1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1, 1, -1, -1, -1, -1, -1]

#: main_pathtraced.js:87-94
NEIGHBOURHOOD_MAP: Dict[str, np.ndarray] = {
    "moore": np.array(_MOORE, dtype=np.int32),
    "moore 2D": np.array(_MOORE2D, dtype=np.int32),
    "von neumann": np.array(_VN, dtype=np.int32),
    "von neumann 2D": np.array(_VN2D, dtype=np.int32),
    "edges": np.array(_EDGES, dtype=np.int32),
    "corners": np.array(_CORNERS, dtype=np.int32),
}

#: Defaults of the MainModule constructor (main_pathtraced.js:101, 123-132).
DEFAULTS = {
    "gridSize": 64,
    "neighbourhood": "von neumann",
    "bornRulesString": "1,3",
    "surviveRulesString": "0-6",
    "bornRulesStringEdges": "27",
    "surviveRulesStringEdges": "27",
    "bornRulesStringCorners": "27",
    "surviveRulesStringCorners": "27",
}

_PARSE_INT = re.compile(r"^\s*([+-]?[0-9]+)")


def _js_parse_int(s: str) -> Optional[int]:
    """`parseInt(s, 10)`: leading whitespace and sign allowed, trailing junk ignored, None for NaN."""
    m = _PARSE_INT.match(s)
    return int(m.group(1)) if m else None


def rules_components_to_values(rules_components: str) -> List[int]:
    """`_rulesComponentsToValues` (main_pathtraced.js:554-581).

    Spaces are stripped, components split on ',', 'a-b' is an inclusive range, every value is clamped to 26.
    Components that `parseInt` cannot read contribute nothing (the reference pushes NaN, which its typed-array
    store then ignores).
    """
    result: List[int] = []
    components = rules_components.replace(" ", "").split(",")
    for comp in components:
        if "-" in comp:
            parts = comp.split("-")
            start = _js_parse_int(parts[0])
            end = _js_parse_int(parts[1])
            if start is None or end is None:
                continue
            if end - start > 1_000_000:
                raise ValueError("rule range too long")
            for j in range(start, end + 1):
                result.append(min(j, 26))
        else:
            v = _js_parse_int(comp)
            if v is not None:
                result.append(min(v, 26))
    return result


def recalculate_rules_values(
    born: str = DEFAULTS["bornRulesString"],
    survive: str = DEFAULTS["surviveRulesString"],
    born_edges: str = DEFAULTS["bornRulesStringEdges"],
    survive_edges: str = DEFAULTS["surviveRulesStringEdges"],
    born_corners: str = DEFAULTS["bornRulesStringCorners"],
    survive_corners: str = DEFAULTS["surviveRulesStringCorners"],
) -> Tuple[np.ndarray, np.ndarray]:
    """`_recalculateRulesValues` (main_pathtraced.js:583-622) -> (bornRulesValues, surviveRulesValues).

    Two Uint32Array(81): 27 slots per rule-set at offsets 0 / 27 / 54 (main, edges, corners).
    """
    rulesets = [born, survive, born_edges, survive_edges, born_corners, survive_corners]
    born_values = np.zeros(NEIGHBOURS_STORAGE_LEN * 3, dtype=np.uint32)
    survive_values = np.zeros(NEIGHBOURS_STORAGE_LEN * 3, dtype=np.uint32)
    offset = 0
    for i in range(0, len(rulesets), 2):
        for v in rules_components_to_values(rulesets[i]):
            if 0 <= v + offset < born_values.size:  # typed arrays drop out-of-range stores
                born_values[v + offset] = 1
        for v in rules_components_to_values(rulesets[i + 1]):
            if 0 <= v + offset < survive_values.size:
                survive_values[v + offset] = 1
        offset += NEIGHBOURS_STORAGE_LEN
    return born_values, survive_values


def grid_size_ui_formatter(v: int) -> int:
    """`_gridSizeUIFormatter` (main_pathtraced.js:675-693): round to the closest multiple of 32 (ties down)."""
    out = v
    m = v % 32
    if m > 0:
        out = v - m if m <= 16 else v - m + 32
    return out


def words_per_buffer(grid_size: int) -> int:
    """`new Uint32Array((G / 32) * G * G)` (main_pathtraced.js:1241)."""
    _check_grid(grid_size)
    return (grid_size // 32) * grid_size * grid_size


def trace_samples(max_steps: int, check_every: int) -> int:
    """K of `ca3d_ensemble_step_until_trace` (include/ca3d.h): the samples one universe can leave — one per check point at steps 0,
    check_every, 2 check_every ... of the call, and the last one at max_steps."""
    if check_every < 1 or max_steps < 0:
        raise ValueError("check_every must be at least 1 and max_steps at least 0")
    return -(-max_steps // check_every) + 1


def sheet_shape(count: int, tile_w: int, tile_h: int, columns: int) -> Tuple[int, int]:
    """(H, W) of `ca3d_ensemble_render_sheet`'s sheet (include/ca3d.h): `columns` tiles a row, ceil(count / columns) rows."""
    if count < 1 or columns < 1 or tile_w < 1 or tile_h < 1:
        raise ValueError("a sheet has at least one tile, one column and one pixel a tile")
    return -(-count // columns) * tile_h, columns * tile_w


def sheet_tile(sheet: np.ndarray, k: int, tile_w: int, tile_h: int, columns: int) -> np.ndarray:
    """Tile k of a sheet `[H, W, ...]` as a view: column k % columns, row k // columns."""
    row, col = divmod(k, columns)
    if k < 0 or (row + 1) * tile_h > sheet.shape[0] or columns * tile_w != sheet.shape[1]:
        raise ValueError(f"tile {k} of {columns} columns of {tile_w} x {tile_h} tiles is not in a sheet of shape {sheet.shape}")
    return sheet[row * tile_h:(row + 1) * tile_h, col * tile_w:(col + 1) * tile_w]


def get_cluster_idx_from_grid_coordinates(grid_size: int, x: int, y: int, z: int) -> int:
    """`_getClusterIdxFromGridCoordinates` (main_pathtraced.js:1170-1178)."""
    cols = grid_size // 32
    layer = cols * grid_size
    return ((x // 32) % cols) + (y % grid_size) * cols + (z % grid_size) * layer


def _check_grid(grid_size: int) -> None:
    if grid_size <= 0 or grid_size % 32:
        raise ValueError(f"grid size must be a positive multiple of 32, got {grid_size}")


def initial_state(
    grid_size: int, random_initial_state: bool = False, random: Optional[Callable[[], float]] = None
) -> np.ndarray:
    """Initial packed state of `_setupStorageBuffers` (main_pathtraced.js:1241-1297).

    Default: one cell at (c, c, c), c = floor(G/2) - 1. Random mode: the 5x5x5 block around c, each cell set
    iff `random() > .5`, drawn in the reference's i, j, k loop order; `random` replaces the reference's
    unseeded `Math.random` (defaults to a fixed-seed generator so runs are reproducible). The same data goes
    to both ping-pong buffers (1361-1362).
    """
    _check_grid(grid_size)
    data = np.zeros(words_per_buffer(grid_size), dtype=np.uint32)
    center = math.floor(grid_size * 0.5) - 1
    if random_initial_state:
        if random is None:
            rng = np.random.default_rng(0xCA3D0001)
            random = lambda: float(rng.random())  # noqa: E731
        for i in range(-2, 3):
            for j in range(-2, 3):
                for k in range(-2, 3):
                    idx = get_cluster_idx_from_grid_coordinates(grid_size, center + i, center + j, center + k)
                    bit = np.uint32(1 << ((center + i) & 31))  # JS `1 << center + i` masks the shift count
                    if random() > 0.5:
                        data[idx] |= bit
                    else:
                        data[idx] &= ~bit
    else:
        idx = get_cluster_idx_from_grid_coordinates(grid_size, center, center, center)
        data[idx] = np.uint32(1 << (center % 32))
    return data


def dispatch_shape(grid_size: int) -> Tuple[int, int, int]:
    """`dispatchWorkgroups(G / 32, ceil(G / 16), ceil(G / 16))` (main_pathtraced.js:1805-1806)."""
    wg = math.ceil(grid_size / WORK_GROUP_SIZE)
    return (grid_size // 32, wg, wg)


# ---------------------------------------------------------------------------------------- synthetic inputs


def _mix32(seed: int, i: np.ndarray, rnd: int) -> np.ndarray:
    x = (i.astype(np.uint64) * 0x9E3779B9 + seed + rnd * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def random_fill(n_words: int, seed: int = 0xCA3D0001, and_rounds: int = 0) -> np.ndarray:
    """Counter-based synthetic fill: word[i] = mix32(seed, i); density 2^-(1+and_rounds)."""
    i = np.arange(n_words, dtype=np.uint64)
    w = _mix32(seed, i, 0)
    for r in range(1, and_rounds + 1):
        w &= _mix32(seed, i, r)
    return w


def _seed_box(grid_size: int, box):
    """((x0, y0, z0), (x1, y1, z1)) inclusive, None = the whole grid; validated as `ca3d_seed` is."""
    G = int(grid_size)
    if box is None:
        return (0, 0, 0), (G - 1, G - 1, G - 1)
    lo, hi = tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1])
    if len(lo) != 3 or len(hi) != 3 or any(a < 0 or a > b or b >= G for a, b in zip(lo, hi)):
        raise ValueError(f"box {lo} .. {hi} does not lie in a grid of {G}")
    return lo, hi


def seeded_state(grid_size: int, seed: int, and_rounds: int = 0, box=None, layout: int = 0, z0: int = 0, nz: Optional[int] = None) -> np.ndarray:
    """The definition of `ca3d_seed_state` (include/ca3d.h) in executable form: what the device kernels (csrc/ca_seed.hip) must write.

    Planes [z0, z0 + nz) of a G^3 grid (default: all). PACKED32 (layout 0): word (x >> 5) + y * cols + z * cols * G of the FULL grid is the
    `random_fill` word of that index, ANDed with the mask of its bits whose x lies in the box, and 0 when y or z is outside it. UNPACKED
    (layout 1): cell (x, y, z) is 1 exactly when it is in the box and bit x & 31 of the packed word at (x >> 5) + y * ceil(G / 32) +
    z * ceil(G / 32) * G is set. `box` = ((x0, y0, z0), (x1, y1, z1)) inclusive, global cell coordinates; None: the whole grid."""
    G = int(grid_size)
    if layout == 0:
        _check_grid(G)
    elif G <= 0 or G % 4:
        raise ValueError(f"unpacked grid size must be a positive multiple of 4, got {G}")
    if not 0 <= and_rounds <= 31:
        raise ValueError("and_rounds must be in [0, 31]")
    nz = G - z0 if nz is None else nz
    if z0 < 0 or nz <= 0 or z0 + nz > G:
        raise ValueError("planes outside the grid")
    lo, hi = _seed_box(G, box)
    cols = (G + 31) // 32
    plane = cols * G
    i = np.arange(z0 * plane, (z0 + nz) * plane, dtype=np.uint64)  # enters the hash modulo 2^32 (_mix32 masks)
    w = _mix32(seed, i, 0)
    for r in range(1, and_rounds + 1):
        w &= _mix32(seed, i, r)
    w = w.reshape(nz, G, cols)
    xw = np.arange(cols, dtype=np.int64) * 32
    first = np.clip(lo[0] - xw, 0, 32)  # bits below `first` and from `last` on lie outside the box
    last = np.clip(hi[0] + 1 - xw, 0, 32)
    ones = np.uint64(0xFFFFFFFF)
    xmask = (((ones << first.astype(np.uint64)) & ones) & ~((ones << last.astype(np.uint64)) & ones) & ones).astype(np.uint32)
    xmask[last <= first] = 0
    w = w & xmask[None, None, :]
    ys, zs = np.arange(G), np.arange(z0, z0 + nz)
    w[:, (ys < lo[1]) | (ys > hi[1]), :] = 0
    w[(zs < lo[2]) | (zs > hi[2]), :, :] = 0
    if layout == 0:
        return np.ascontiguousarray(w).reshape(-1)
    bits = (w[:, :, :, None] >> np.arange(32, dtype=np.uint32)[None, None, None, :]) & np.uint32(1)
    return np.ascontiguousarray(bits.reshape(nz, G, cols * 32)[:, :, :G]).reshape(-1)


def cells_to_words(grid_size: int, cells: Iterable[Sequence[int]]) -> np.ndarray:
    """Packed state with exactly the listed (x, y, z) cells alive."""
    data = np.zeros(words_per_buffer(grid_size), dtype=np.uint32)
    for (x, y, z) in cells:
        data[get_cluster_idx_from_grid_coordinates(grid_size, x, y, z)] |= np.uint32(1 << (x % 32))
    return data


def get_cell(grid_size: int, words: np.ndarray, x: int, y: int, z: int) -> int:
    return int((int(words[get_cluster_idx_from_grid_coordinates(grid_size, x, y, z)]) >> (x % 32)) & 1)


# ------------------------------------------------------------------------------------------- state summary
# The definition of ca3d_summarize (include/ca3d.h) in executable form: what the device kernel (csrc/ca_summary.hip) must return,
# usable on checkpoint files and read-back states. No reference counterpart.

_M64 = (1 << 64) - 1


def digest_mix(index: int, word: int) -> int:
    """splitmix64 finaliser of key = (index << 32 | word) modulo 2^64: one term of the state digest (plain Python integers)."""
    z = ((((index << 32) & _M64) | word) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _popcount32(w: np.ndarray) -> np.ndarray:
    """Set bits per u32 word."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(w).astype(np.uint32)
    w = w - ((w >> np.uint32(1)) & np.uint32(0x55555555))
    w = (w & np.uint32(0x33333333)) + ((w >> np.uint32(2)) & np.uint32(0x33333333))
    w = (w + (w >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return (w * np.uint32(0x01010101)) >> np.uint32(24)


def _digest(words: np.ndarray, base_index: int) -> int:
    total = 0
    chunk = 1 << 22
    with np.errstate(over="ignore"):
        for lo in range(0, words.size, chunk):
            w = words[lo:lo + chunk]
            nz = np.flatnonzero(w)
            if nz.size == 0:
                continue
            z = ((nz.astype(np.uint64) + np.uint64(base_index + lo)) << np.uint64(32)) | w[nz].astype(np.uint64)
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            total = (total + int(np.add.reduce(z, dtype=np.uint64))) & _M64
    return total


def state_summary(grid_size: int, words, prev_words=None, layout: int = 0, z0: int = 0) -> dict:
    """The numbers of `ca3d_summarize` for the state `words` (layout 0: PACKED32, 1: UNPACKED) — the whole grid, or the planes
    [z0, z0 + nz) of it when fewer words are given (a slab's owned planes). `prev_words`: the same planes one step earlier (None:
    has_previous False, births = deaths = 0). Box coordinates are global; the digest is keyed by the word's index in the FULL grid,
    so the digests of the slabs of a grid add up (modulo 2^64) to the digest of the grid.

    -> dict(population, births, deaths, digest, has_previous, box_min (x, y, z), box_max, plane_population u32[nz])."""
    G = int(grid_size)
    w = np.ascontiguousarray(words, dtype=np.uint32).ravel()
    cols = G // 32 if layout == 0 else G
    if layout == 0:
        _check_grid(G)
    plane_words = cols * G
    if w.size == 0 or w.size % plane_words:
        raise ValueError("the state must hold whole z planes")
    nz = w.size // plane_words
    if z0 < 0 or z0 + nz > G:
        raise ValueError("planes outside the grid")
    alive = _popcount32(w) if layout == 0 else (w == 1).astype(np.uint32)  # unpacked: alive iff the word == 1 (the legacy kernel's `st == 1u`)
    out = {"has_previous": prev_words is not None, "births": 0, "deaths": 0}
    if prev_words is not None:
        q = np.ascontiguousarray(prev_words, dtype=np.uint32).ravel()
        if q.size != w.size:
            raise ValueError("prev_words must hold the same planes")
        if layout == 0:
            out["births"] = int(_popcount32(w & ~q).sum(dtype=np.uint64))
            out["deaths"] = int(_popcount32(q & ~w).sum(dtype=np.uint64))
        else:
            was = q == 1
            out["births"] = int(np.count_nonzero((w == 1) & ~was))
            out["deaths"] = int(np.count_nonzero(was & (w != 1)))
    a3 = alive.reshape(nz, G, cols)
    planes = a3.sum(axis=(1, 2), dtype=np.uint64)
    out["plane_population"] = planes.astype(np.uint32)
    out["population"] = int(planes.sum(dtype=np.uint64))
    out["digest"] = _digest(w, z0 * plane_words)
    if out["population"] == 0:
        out["box_min"], out["box_max"] = (G, G, G), (0, 0, 0)
        return out
    zs = np.flatnonzero(planes)
    ys = np.flatnonzero(a3.any(axis=(0, 2)))
    xcols = np.flatnonzero(a3.any(axis=(0, 1)))
    if layout == 0:
        w3 = w.reshape(nz, G, cols)
        lo = int(np.bitwise_or.reduce(w3[:, :, xcols[0]], axis=None))
        hi = int(np.bitwise_or.reduce(w3[:, :, xcols[-1]], axis=None))
        x0 = int(xcols[0]) * 32 + ((lo & -lo).bit_length() - 1)
        x1 = int(xcols[-1]) * 32 + hi.bit_length() - 1
    else:
        x0, x1 = int(xcols[0]), int(xcols[-1])
    out["box_min"] = (x0, int(ys[0]), z0 + int(zs[0]))
    out["box_max"] = (x1, int(ys[-1]), z0 + int(zs[-1]))
    return out


def moved_by(grid_size: int, a_words, b_words) -> Optional[Tuple[int, int, int]]:
    """The predicate behind CA3D_STOP_MOVING (include/ca3d.h, ca3d_ensemble_step_until_moving) on the CPU: (dx, dy, dz) when the packed
    state `b_words` is the packed state `a_words` translated by that vector, both non-empty, both bounding boxes strictly inside the grid
    (box_min >= 1, box_max <= G - 2 on every axis) and the vector not zero; None otherwise — equal states included. For following a
    candidate up on the host: `moved_by(64, state_then, state_now)`."""
    G = int(grid_size)
    sa, sb = state_summary(G, a_words), state_summary(G, b_words)
    if sa["population"] == 0 or sa["population"] != sb["population"]:
        return None
    for s in (sa, sb):
        if min(s["box_min"]) < 1 or max(s["box_max"]) > G - 2:
            return None
    d = tuple(int(q - p) for p, q in zip(sa["box_min"], sb["box_min"]))
    if d == (0, 0, 0) or tuple(int(q - p) for p, q in zip(sa["box_max"], sb["box_max"])) != d:
        return None

    def box(words, s):
        cells = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").ravel().view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]
        (x0, y0, z0), (x1, y1, z1) = s["box_min"], s["box_max"]
        return cells[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]

    # (nothing lives outside either box: equal boxes' contents are equal states up to the shift)
    return d if np.array_equal(box(a_words, sa), box(b_words, sb)) else None


# ------------------------------------------------------------------------------------------------- census
# The definition of ca3d_ensemble_census (include/ca3d.h) in executable form: the connected objects of one 64^3 universe.

#: ca3d_component (include/ca3d.h), 32 bytes
COMPONENT_DTYPE = np.dtype([("population", "<u4"), ("first_cell", "<u4"), ("box_min", "<u4"), ("box_max", "<u4"), ("digest", "<u8"),
                            ("reserved", "<u4", (2,))])


def unpack_box(word: int) -> Tuple[int, int, int]:
    """(x, y, z) of a packed box corner x | y << 8 | z << 16 (`ca3d_component.box_min` / `box_max`)."""
    word = int(word)
    return word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF


def _dilate_closed(f: np.ndarray) -> np.ndarray:
    """The 3 x 3 x 3 dilation of a boolean cube [z, y, x] inside the cube: nothing crosses a face."""
    for axis in range(3):
        g = f.copy()
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(hi)] |= f[tuple(lo)]
        g[tuple(lo)] |= f[tuple(hi)]
        f = g
    return f


#: enum CA3D_CONNECT_* (include/ca3d.h): index = value
CONNECTIVITIES = ("closed", "torus")


def _dilate_window(f: np.ndarray, wrap) -> np.ndarray:
    """`_dilate_closed`, except that an axis with wrap[axis] set is a ring: its two ends are neighbours."""
    for axis in range(3):
        if wrap[axis]:
            f = f | np.roll(f, 1, axis=axis) | np.roll(f, -1, axis=axis)
            continue
        g = f.copy()
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(hi)] |= f[tuple(lo)]
        g[tuple(lo)] |= f[tuple(hi)]
        f = g
    return f


def _torus_component(live: np.ndarray, z: int, y: int, x: int) -> np.ndarray:
    """The component of the live cell (z, y, x) of the boolean cube `live` [z, y, x] under the 26-neighbourhood of Z_64^3 -> boolean
    cube. The cube is rolled so that the seed sits at the centre; the fill then works in the closed fill's growing window, which
    before every dilation holds the filled cells with a margin of one, and an axis becomes a ring once the window spans it."""
    G = 64
    c = G // 2
    rolled = np.roll(live, (c - z, c - y, c - x), axis=(0, 1, 2))
    f = np.zeros((G, G, G), dtype=bool)
    f[c, c, c] = True
    lo, hi = [c, c, c], [c + 1, c + 1, c + 1]
    size = 1
    while True:
        lo = [max(v - 1, 0) for v in lo]
        hi = [min(v + 1, G) for v in hi]
        win = tuple(slice(a, b) for a, b in zip(lo, hi))
        f[win] = _dilate_window(f[win], [a == 0 and b == G for a, b in zip(lo, hi)]) & rolled[win]
        grown = int(np.count_nonzero(f[win]))
        if grown == size:
            break
        size = grown
    return np.roll(f, (z - c, y - c, x - c), axis=(0, 1, 2))


def torus_span(coords) -> Tuple[int, int]:
    """(start, extent) of the shortest cyclic interval {start, ..., start + extent - 1 mod 64} that covers the coordinates `coords`
    (a non-empty subset of Z_64) and starts at one of them; ties go to the smallest start. All 64 give (0, 64)."""
    S = np.unique(np.asarray(coords, dtype=np.int64) % 64)
    extents = [int(((S - s) % 64).max()) + 1 for s in S]  # S is sorted: the first minimum is the smallest start
    k = int(np.argmin(extents))
    return int(S[k]), extents[k]


def census(words, max_components: int = 64, connectivity: str = "closed") -> Tuple[np.ndarray, int, int]:
    """`ca3d_ensemble_census` for ONE packed 64^3 universe, in plain numpy: the connected components of its live cells under the
    26-neighbourhood inside the closed cube (no face wraps), ordered by their first cells (smallest x + 64 y + 4096 z)
    -> (components [max_components] of COMPONENT_DTYPE, n_components, remaining). The first min(C, max_components) components are
    listed, the slots behind them are zero, `remaining` is the number of live cells in no listed component. A component's digest is
    `state_summary(64, translated)["digest"]` of the state that holds only it, translated by -box_min.

    `connectivity="torus"` is `ca3d_ensemble_census_connected` with CA3D_CONNECT_TORUS: cells are adjacent when they differ by at most
    1 modulo 64 on every axis; per axis box_min is the start of the shortest cyclic interval that covers the component's coordinates
    (`torus_span`), box_max = box_min + extent - 1 is NOT reduced (>= 64 through a seam), and the translation by -box_min is cyclic."""
    G = 64
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"unknown connectivity {connectivity!r}: one of {CONNECTIVITIES}")
    if not 1 <= int(max_components) <= 1024:
        raise ValueError("max_components is 1 .. 1024")
    w = np.ascontiguousarray(words, dtype="<u4").ravel()
    if w.size != words_per_buffer(G):
        raise ValueError("a universe holds 8192 words")
    rest = np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G).astype(bool)  # [z, y, x]: the flat index is x + 64 y + 4096 z
    out = np.zeros(int(max_components), dtype=COMPONENT_DTYPE)
    n = 0
    while n < max_components:
        live = np.flatnonzero(rest.ravel())
        if live.size == 0:
            break
        first = int(live[0])
        z, y, x = first >> 12, (first >> 6) & 63, first & 63
        if connectivity == "torus":
            f = _torus_component(rest, z, y, x)
            zs, ys, xs = np.nonzero(f)
            (bx, ex), (by, ey), (bz, ez) = torus_span(xs), torus_span(ys), torus_span(zs)
            moved = np.zeros((G, G, G), dtype=np.uint8)
            moved[(zs - bz) % G, (ys - by) % G, (xs - bx) % G] = 1
            rec = out[n]
            rec["population"] = zs.size
            rec["first_cell"] = first
            rec["box_min"] = bx | by << 8 | bz << 16
            rec["box_max"] = (bx + ex - 1) | (by + ey - 1) << 8 | (bz + ez - 1) << 16
            rec["digest"] = state_summary(G, np.packbits(moved.ravel(), bitorder="little").view("<u4"))["digest"]
            rest &= ~f
            n += 1
            continue
        z0, z1, y0, y1, x0, x1 = z, z + 1, y, y + 1, x, x + 1  # the fill works in a window that grows with the component
        f = np.zeros((G, G, G), dtype=bool)
        f[z, y, x] = True
        size = 1
        while True:
            z0, y0, x0 = max(z0 - 1, 0), max(y0 - 1, 0), max(x0 - 1, 0)
            z1, y1, x1 = min(z1 + 1, G), min(y1 + 1, G), min(x1 + 1, G)
            win = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
            f[win] = _dilate_closed(f[win]) & rest[win]
            grown = int(np.count_nonzero(f[win]))
            if grown == size:
                break
            size = grown
        zs, ys, xs = np.nonzero(f)
        bz, by, bx = int(zs.min()), int(ys.min()), int(xs.min())
        moved = np.zeros((G, G, G), dtype=np.uint8)
        moved[zs - bz, ys - by, xs - bx] = 1
        translated = np.packbits(moved.ravel(), bitorder="little").view("<u4")
        rec = out[n]
        rec["population"] = zs.size
        rec["first_cell"] = first
        rec["box_min"] = bx | by << 8 | bz << 16
        rec["box_max"] = int(xs.max()) | int(ys.max()) << 8 | int(zs.max()) << 16
        rec["digest"] = state_summary(G, translated)["digest"]
        rest &= ~f
        n += 1
    return out, n, int(np.count_nonzero(rest))


# ------------------------------------------------------------------------------------------- ensemble step
# The definition of one step of an ensemble universe under each boundary (include/ca3d.h, ca3d_ensemble_set_boundary) in executable
# form: what the ca_ensemble_* kernels must compute. "reference" is the reference's own boundary (- faces dead, + faces wrap).

ENSEMBLE_KINDS = ("von neumann", "moore", "clustered")
ENSEMBLE_BOUNDARIES = ("reference", "torus", "closed")  # index = enum ca3d_ensemble_boundary


def _neighbour(a: np.ndarray, axis: int, d: int, boundary: str) -> np.ndarray:
    """The array whose entry at p is a's entry at p + d along `axis` (d = -1 or +1): np.roll is a wrapping face, a zeroed slice after
    the roll a dead one."""
    out = np.roll(a, -d, axis=axis)
    wraps = boundary == "torus" or (boundary == "reference" and d > 0)
    if not wraps:
        edge = [slice(None)] * a.ndim
        edge[axis] = -1 if d > 0 else 0
        out[tuple(edge)] = 0
    return out


def _table(mask: int, n: int) -> np.ndarray:
    return ((int(mask) >> np.arange(n)) & 1).astype(np.uint8)


def _ensemble_counts(words, kind: str, boundary: str):
    """(cells [z, y, x] of one packed 64^3 universe, the counts its step looks up): one array for "von neumann" (F, 0 .. 6) and "moore"
    (0 .. 26), the three (T, E, C) of the main, edges and corners tables for "clustered". Every axis applies its boundary to what the
    axis before it produced — x, then y, then z — so an edge or corner neighbour exists exactly when each of its three coordinates
    does; the counts are formed separably for that reason."""
    if kind not in ENSEMBLE_KINDS:
        raise ValueError(f"unknown ensemble kind {kind!r}: one of {ENSEMBLE_KINDS}")
    if boundary not in ENSEMBLE_BOUNDARIES:
        raise ValueError(f"unknown ensemble boundary {boundary!r}: one of {ENSEMBLE_BOUNDARIES}")
    G = 64
    w = np.ascontiguousarray(words, dtype="<u4").ravel()
    if w.size != words_per_buffer(G):
        raise ValueError("a universe holds 8192 words")
    a = np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]: the flat index is x + 64 y + 4096 z
    Z, Y, X = 0, 1, 2

    def both(v, axis):  # the two neighbours along one axis, summed
        return _neighbour(v, axis, -1, boundary) + _neighbour(v, axis, +1, boundary)

    if kind == "von neumann":
        return a, (both(a, X) + both(a, Y) + both(a, Z),)
    if kind == "moore":
        s = a
        for axis in (X, Y, Z):
            s = s + both(s, axis)
        return a, (s - a,)  # the 3 x 3 x 3 sum without the cell itself
    left, right = _neighbour(a, X, -1, boundary), _neighbour(a, X, +1, boundary)
    faces_in_plane = left + right + both(a, Y)            # the 4 face neighbours in the cell's own plane
    diagonals_in_plane = both(left, Y) + both(right, Y)   # the 4 in-plane diagonals
    faces = faces_in_plane + both(a, Z)                   # 0 .. 6
    edges = diagonals_in_plane + both(faces_in_plane, Z)  # 0 .. 12
    corners = both(diagonals_in_plane, Z)                 # 0 .. 8
    return a, (faces + edges + corners, edges, corners)


def ensemble_step(words, kind: str, tables, boundary: str = "reference") -> np.ndarray:
    """One step of ONE packed 64^3 universe (8192 words) -> its packed successor, in plain numpy on the unpacked [z, y, x] array.

    `kind`: "von neumann" (counts 0 .. 6 over the six face neighbours), "moore" (0 .. 26) or "clustered". `tables`: the masks
    `Ensemble.set_rule_tables` / `set_clustered_tables` take — (born, survive), bit c = at count c; clustered: (born[3], survive[3]) for
    the main (Moore, 0 .. 26), edges (0 .. 12) and corners (0 .. 8) rule-sets, whose three lookups are ORed; a live cell looks up
    survive at its count, a dead one born. `boundary`: "reference", "torus" or "closed".
    Every axis applies its boundary to what the axis before it produced — x, then y, then z — so an edge or corner neighbour exists
    exactly when each of its three coordinates does; the counts are formed separably for that reason (`_ensemble_counts`)."""
    a, counts = _ensemble_counts(words, kind, boundary)
    alive = a.astype(bool)
    born, survive = tables
    if kind == "von neumann":
        nxt = np.where(alive, _table(survive, 7)[counts[0]], _table(born, 7)[counts[0]])
    elif kind == "moore":
        nxt = np.where(alive, _table(survive, 27)[counts[0]], _table(born, 27)[counts[0]])
    else:
        nxt = np.zeros_like(a)
        for count, n, b, s in zip(counts, (27, 13, 9), born, survive):
            nxt |= np.where(alive, _table(s, n)[count], _table(b, n)[count])
    return np.packbits(nxt.astype(np.uint8).ravel(), bitorder="little").view("<u4").copy()


# ------------------------------------------------------------------------------------------------- isolate
# The definition of ca3d_ensemble_isolate (include/ca3d.h) in executable form, for one universe.

ISOLATE_PLACEMENTS = ("keep", "centre", "origin")


def isolate(words, cell: int, placement: str = "centre", connectivity: str = "closed") -> Tuple[np.ndarray, int, Tuple[int, int, int]]:
    """`ca3d_ensemble_isolate` for ONE packed 64^3 universe, in plain numpy: the connected component (26-neighbourhood inside the
    closed cube, no face wraps: the census') that holds `cell` = x + 64 y + 4096 z, alone, translated by the shift of `placement` —
    "keep": 0; "origin": -box_min; "centre": (64 - extent) // 2 - box_min per axis -> (words u32[8192], population, (dx, dy, dz)).
    Any cell of the component selects it; a dead cell gives zeros, population 0 and a zero shift.

    `connectivity="torus"` is `ca3d_ensemble_isolate_connected` with CA3D_CONNECT_TORUS: the component is the torus census', box_min
    and extent are its cyclic box's (`torus_span`), the shift is the same formula and is applied modulo 64, so the object arrives in
    one piece; the shift returned is the formula's value."""
    G = 64
    if placement not in ISOLATE_PLACEMENTS:
        raise ValueError(f"unknown placement {placement!r}: one of {ISOLATE_PLACEMENTS}")
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"unknown connectivity {connectivity!r}: one of {CONNECTIVITIES}")
    cell = int(cell)
    if not 0 <= cell < G * G * G:
        raise ValueError("a cell is x + 64 y + 4096 z, below 2^18")
    w = np.ascontiguousarray(words, dtype="<u4").ravel()
    if w.size != words_per_buffer(G):
        raise ValueError("a universe holds 8192 words")
    live = np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G).astype(bool)  # [z, y, x]
    z, y, x = cell >> 12, (cell >> 6) & 63, cell & 63
    if not live[z, y, x]:
        return np.zeros(words_per_buffer(G), dtype=np.uint32), 0, (0, 0, 0)
    if connectivity == "torus":
        zs, ys, xs = np.nonzero(_torus_component(live, z, y, x))
        shift = []
        for v in (xs, ys, zs):
            lo, extent = torus_span(v)
            shift.append(0 if placement == "keep" else -lo if placement == "origin" else (G - extent) // 2 - lo)
        dx, dy, dz = shift
        moved = np.zeros((G, G, G), dtype=np.uint8)
        moved[(zs + dz) % G, (ys + dy) % G, (xs + dx) % G] = 1
        return np.packbits(moved.ravel(), bitorder="little").view("<u4").astype(np.uint32), int(zs.size), (dx, dy, dz)
    z0, z1, y0, y1, x0, x1 = z, z + 1, y, y + 1, x, x + 1  # the fill works in a window that grows with the component (census)
    f = np.zeros((G, G, G), dtype=bool)
    f[z, y, x] = True
    size = 1
    while True:
        z0, y0, x0 = max(z0 - 1, 0), max(y0 - 1, 0), max(x0 - 1, 0)
        z1, y1, x1 = min(z1 + 1, G), min(y1 + 1, G), min(x1 + 1, G)
        win = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        f[win] = _dilate_closed(f[win]) & live[win]
        grown = int(np.count_nonzero(f[win]))
        if grown == size:
            break
        size = grown
    zs, ys, xs = np.nonzero(f)
    shift = []
    for v in (xs, ys, zs):
        lo, extent = int(v.min()), int(v.max()) - int(v.min()) + 1
        shift.append(0 if placement == "keep" else -lo if placement == "origin" else (G - extent) // 2 - lo)
    dx, dy, dz = shift
    moved = np.zeros((G, G, G), dtype=np.uint8)
    moved[zs + dz, ys + dy, xs + dx] = 1
    return np.packbits(moved.ravel(), bitorder="little").view("<u4").astype(np.uint32), int(zs.size), (dx, dy, dz)


# ------------------------------------------------------------------------------------------------- compose
# The definition of ca3d_ensemble_compose (include/ca3d.h) in executable form, for one destination, and the 48 orientations it turns
# a piece by.

#: orientation o turns by the signed permutation perm = ORIENTATION_PERMS[o % 6], bit i of o // 6 mirroring OUTPUT axis i
ORIENTATION_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
#: ca3d_compose_part, 24 bytes, and ca3d_composed, 16 bytes (include/ca3d.h)
COMPOSE_PART_DTYPE = np.dtype([("universe", "<u4"), ("orientation", "<u4"), ("at", "<i4", (3,)), ("reserved", "<u4")])
COMPOSED_DTYPE = np.dtype([("population", "<u4"), ("placed", "<u4"), ("overlap", "<u4"), ("clipped", "<u4")])


def _orientation(o) -> Tuple[Tuple[int, int, int], int]:
    if isinstance(o, bool) or int(o) != o or not 0 <= int(o) < 48:
        raise ValueError("an orientation is 0 .. 47")
    return ORIENTATION_PERMS[int(o) % 6], int(o) // 6


def orientation_matrix(o: int) -> np.ndarray:
    """The 3 x 3 integer matrix M of orientation o: output axis i is input axis perm[i], negated where bit i of o // 6 is set, so a
    direction v of the piece turns into M @ v. Determinant +1: a rotation; -1: a reflection."""
    perm, f = _orientation(o)
    m = np.zeros((3, 3), dtype=np.int64)
    for i in range(3):
        m[i, perm[i]] = -1 if f >> i & 1 else 1
    return m


def orientation_from_matrix(m) -> int:
    """The orientation whose `orientation_matrix` is m (a signed permutation matrix; anything else is a ValueError)."""
    m = np.asarray(m)
    if m.shape != (3, 3) or not np.array_equal(np.abs(m).sum(axis=0), (1, 1, 1)) or not np.array_equal(np.abs(m).sum(axis=1), (1, 1, 1)) \
            or not np.isin(m, (-1, 0, 1)).all():
        raise ValueError("not a signed permutation matrix")
    perm = tuple(int(np.flatnonzero(m[i])[0]) for i in range(3))
    f = sum(1 << i for i in range(3) if m[i, perm[i]] < 0)
    return ORIENTATION_PERMS.index(perm) + 6 * f


def orient_vector(o: int, v) -> Tuple[int, int, int]:
    """A direction v = (x, y, z) of a piece — a ship's shift — as it points after the piece is turned by orientation o."""
    return tuple(int(c) for c in orientation_matrix(o) @ np.asarray(v, dtype=np.int64))


def compose_parts(parts) -> np.ndarray:
    """A list of (universe, orientation, (x, y, z)) as an array of COMPOSE_PART_DTYPE (reserved 0)."""
    try:
        flat = np.array([(u, o, at[0], at[1], at[2], len(at)) for u, o, at in parts], dtype=np.int64).reshape(-1, 6)
    except (TypeError, IndexError, ValueError):
        raise ValueError("a part is (universe, orientation, (x, y, z))") from None
    if (flat[:, 5] != 3).any() or (flat[:, :2] < 0).any() or (flat[:, :2] >= 1 << 32).any() or (np.abs(flat[:, 2:5]) >= 1 << 31).any():
        raise ValueError("a part is (universe, orientation, (x, y, z))")
    out = np.zeros(len(flat), dtype=COMPOSE_PART_DTYPE)
    out["universe"], out["orientation"], out["at"] = flat[:, 0], flat[:, 1], flat[:, 2:5]
    return out


def compose(states, parts, base=None) -> Tuple[np.ndarray, np.ndarray]:
    """`ca3d_ensemble_compose` for ONE destination, in plain numpy. `states[u]` is the packed 64^3 state of source universe u (a
    sequence or a dict), `parts` a list of (universe, orientation, (x, y, z)), `base` the destination's state under OVER (None: from
    nothing) -> (words u32[8192], record of COMPOSED_DTYPE). A live cell c of a piece with box (min, max), extent e, goes to q + at:
    r[i] = c[perm[i]] - min[perm[i]], q[i] = e[perm[i]] - 1 - r[i] where output axis i is mirrored, else r[i]; it is set when it lies
    inside the cube and counts as clipped otherwise."""
    G = 64
    nw = words_per_buffer(G)

    def cells(w):
        w = np.ascontiguousarray(w, dtype="<u4").ravel()
        if w.size != nw:
            raise ValueError("a universe holds 8192 words")
        return np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]

    dest = np.zeros((G, G, G), dtype=np.uint8) if base is None else cells(base).copy()
    base_pop = int(dest.sum())
    placed = clipped = 0
    for universe, o, at in parts:
        perm, f = _orientation(o)
        at = tuple(int(v) for v in at)
        if len(at) != 3 or not all(-64 <= v <= 64 for v in at):
            raise ValueError("at is (x, y, z), -64 .. 64 each")
        zs, ys, xs = np.nonzero(cells(states[universe]))
        if zs.size == 0:
            continue
        c = (xs, ys, zs)
        q = []
        for i in range(3):
            src = c[perm[i]]
            r = src - src.min()
            q.append((int(src.max()) - int(src.min()) - r if f >> i & 1 else r) + at[i])
        inside = np.ones(zs.size, dtype=bool)
        for v in q:
            inside &= (v >= 0) & (v < G)
        dest[q[2][inside], q[1][inside], q[0][inside]] = 1
        placed += int(inside.sum())
        clipped += int(zs.size - inside.sum())
    rec = np.zeros((), dtype=COMPOSED_DTYPE)
    rec["population"] = int(dest.sum())
    rec["placed"] = placed
    rec["overlap"] = base_pop + placed - int(dest.sum())
    rec["clipped"] = clipped
    return np.packbits(dest.ravel(), bitorder="little").view("<u4").astype(np.uint32), rec


# ------------------------------------------------------------------------------------------------- canon
# The definition of ca3d_ensemble_canon (include/ca3d.h) in executable form, for one universe: a state's name up to the 48 orientations
# and translation, and its symmetry group.

#: ca3d_canon (include/ca3d.h), 32 bytes
CANON_DTYPE = np.dtype([("key", "<u8"), ("symmetry", "<u8"), ("orientation", "<u4"), ("population", "<u4"), ("box_min", "<u4"),
                        ("box_max", "<u4")])


def _box_digest(box: np.ndarray) -> int:
    """`state_summary(64, words)["digest"]` of the 64^3 state that holds the cells `box` [z, y, x] (u8, at most 64 each way) at the
    origin and nothing else: only the box's rows are packed and mixed."""
    ez, ey, ex = box.shape
    rows = np.zeros((ez, ey, 64), dtype=np.uint8)
    rows[:, :, :ex] = box
    w = np.packbits(rows, axis=-1, bitorder="little").view("<u4").reshape(ez, ey, 2)
    index = ((np.arange(ez, dtype=np.uint64)[:, None, None] * np.uint64(64) + np.arange(ey, dtype=np.uint64)[None, :, None]) * np.uint64(2)
             + np.arange(2, dtype=np.uint64)[None, None, :])
    live = w != 0
    with np.errstate(over="ignore"):
        z = (index[live] << np.uint64(32)) | w[live].astype(np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(np.add.reduce(z, dtype=np.uint64))


def canon(words) -> Tuple[np.ndarray, np.ndarray]:
    """`ca3d_ensemble_canon` for ONE packed 64^3 universe, in plain numpy -> (record of CANON_DTYPE, digests u64[48]). With T_o the state
    turned by orientation o, the turned box's minimum at the origin (`compose([S], [(0, o, (0, 0, 0))])[0]`): digests[o] is
    `state_summary(64, T_o)["digest"]`, key the smallest of them, orientation the smallest o that reaches it, bit o of symmetry set
    exactly when T_o equals T_0 cell for cell. An empty universe: key 0, orientation 0, all 48 symmetry bits, boxes 0. The state is
    cropped to its bounding box before it is turned: a small object costs microseconds an orientation."""
    G = 64
    w = np.ascontiguousarray(words, dtype="<u4").ravel()
    if w.size != words_per_buffer(G):
        raise ValueError("a universe holds 8192 words")
    rec = np.zeros((), dtype=CANON_DTYPE)
    digests = np.zeros(48, dtype=np.uint64)
    cells = np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G)  # [z, y, x]
    zs, ys, xs = (np.flatnonzero(cells.any(axis=a)) for a in ((1, 2), (0, 2), (0, 1)))
    if zs.size == 0:
        rec["symmetry"] = (1 << 48) - 1
        return rec, digests
    lo, hi = (int(xs[0]), int(ys[0]), int(zs[0])), (int(xs[-1]), int(ys[-1]), int(zs[-1]))
    box = cells[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
    symmetry = 0
    turned0 = None
    for o in range(48):
        perm, f = _orientation(o)
        # output coordinate i is input coordinate perm[i]; array axis a holds coordinate 2 - a
        t = np.transpose(box, tuple(2 - perm[2 - a] for a in range(3)))
        mirrored = tuple(2 - i for i in range(3) if f >> i & 1)
        if mirrored:
            t = np.flip(t, axis=mirrored)
        if o == 0:
            turned0 = t
        if t.shape == turned0.shape and np.array_equal(t, turned0):
            symmetry |= 1 << o
        digests[o] = _box_digest(t)
    rec["key"] = digests.min()
    rec["orientation"] = int(np.argmin(digests))  # the first of equal minima
    rec["symmetry"] = symmetry
    rec["population"] = int(box.sum(dtype=np.uint64))
    rec["box_min"] = lo[0] | lo[1] << 8 | lo[2] << 16
    rec["box_max"] = hi[0] | hi[1] << 8 | hi[2] << 16
    return rec, digests


def symmetry_orientations(mask: int) -> List[int]:
    """The orientations 0 .. 47 whose bit is set in a `ca3d_canon.symmetry` mask, ascending: the state's symmetry group."""
    mask = int(mask)
    return [o for o in range(48) if mask >> o & 1]


def is_chiral(mask: int) -> bool:
    """True when the symmetry group `mask` holds no orientation with determinant -1: the state differs from its mirror image however
    that is turned."""
    def mirrors(o):  # the determinant: the permutation's sign (odd: one transposition) times -1 for every mirrored axis
        perm, f = _orientation(o)
        return (sum(perm[i] != i for i in range(3)) == 2) != (bin(f).count("1") & 1 == 1)

    return not any(mirrors(o) for o in symmetry_orientations(mask))


# ------------------------------------------------------------------------------------------ canon over a period
# The definition of ca3d_ensemble_canon_period (include/ca3d.h) in executable form, for one universe whose phases the caller has stepped.

#: ca3d_canon_period (include/ca3d.h), 32 bytes
CANON_PERIOD_DTYPE = np.dtype([("key", "<u8"), ("symmetry", "<u8"), ("orientation", "<u4"), ("phase", "<u4"), ("population", "<u4"),
                               ("flags_shift", "<u4")])
#: bit 0 of `flags_shift`, and the longest period a call takes
CANON_CLOSED = 1
CANON_MAX_PERIOD = 4096


def unpack_shift(flags_shift: int) -> Tuple[int, int, int]:
    """(dx, dy, dz) of a `ca3d_canon_period.flags_shift`: the signed bytes in bits 8 .. 15, 16 .. 23 and 24 .. 31."""
    v = int(flags_shift)
    return tuple(((v >> s & 0xFF) ^ 0x80) - 0x80 for s in (8, 16, 24))


def _at_origin(words) -> Tuple[np.ndarray, Tuple[int, int, int]]:
    """-> (the cells of a packed 64^3 state cropped to its bounding box [z, y, x], box_min (x, y, z)); an empty state: a box of one dead
    cell at (0, 0, 0)."""
    cells = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").ravel().view(np.uint8), bitorder="little").reshape(64, 64, 64)
    zs, ys, xs = (np.flatnonzero(cells.any(axis=a)) for a in ((1, 2), (0, 2), (0, 1)))
    if zs.size == 0:
        return cells[:1, :1, :1], (0, 0, 0)
    return cells[zs[0]:zs[-1] + 1, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1], (int(xs[0]), int(ys[0]), int(zs[0]))


def canon_period(states) -> Tuple[np.ndarray, np.ndarray]:
    """`ca3d_ensemble_canon_period` for ONE universe, in plain numpy over `canon`. `states` is [p + 1, 8192]: the phases S_0 .. S_p of
    a period p >= 1, stepped by the caller (an oracle, `Ensemble.step`) -> (record of CANON_PERIOD_DTYPE, keys u64[p]). keys[t] is
    `canon(S_t)`'s key; the record's key is the smallest of them, `phase` the smallest t that reaches it, orientation, symmetry and
    population that phase's. CLOSED (bit 0 of flags_shift) is set exactly when S_p translated to the origin equals S_0 translated to
    the origin cell for cell; the shift (`unpack_shift`) is then box_min(S_p) - box_min(S_0), and zero when S_0 is empty."""
    s = np.ascontiguousarray(states, dtype="<u4")
    if s.ndim != 2 or s.shape[0] < 2 or s.shape[1] != words_per_buffer(64):
        raise ValueError("states is [p + 1, 8192] with p >= 1: the phases S_0 .. S_p")
    p = s.shape[0] - 1
    if p > CANON_MAX_PERIOD:
        raise ValueError(f"a period is at most {CANON_MAX_PERIOD}")
    recs = [canon(s[t])[0] for t in range(p)]
    keys = np.array([int(r["key"]) for r in recs], dtype=np.uint64)
    t = int(np.argmin(keys))  # the first of equal minima
    rec = np.zeros((), dtype=CANON_PERIOD_DTYPE)
    rec["key"], rec["phase"] = keys[t], t
    for f in ("symmetry", "orientation", "population"):
        rec[f] = recs[t][f]
    (a, amin), (b, bmin) = _at_origin(s[0]), _at_origin(s[p])
    flags_shift = 0
    if a.shape == b.shape and np.array_equal(a, b):
        flags_shift = CANON_CLOSED
        if a.any():
            for i in range(3):
                flags_shift |= ((bmin[i] - amin[i]) & 0xFF) << (8 + 8 * i)
    rec["flags_shift"] = flags_shift
    return rec, keys


# ------------------------------------------------------------------------------------------ envelope over a period
# The definition of ca3d_ensemble_envelope (include/ca3d.h) in executable form, for one universe.

#: ca3d_envelope (include/ca3d.h), 48 bytes; a box corner is x, y, z and a zero byte
ENVELOPE_DTYPE = np.dtype([("period", "<u4"), ("flags", "<u4"), ("heat", "<u4"), ("population_sum", "<u4"), ("envelope_population", "<u4"),
                           ("stator_population", "<u4"), ("envelope_min", "u1", 4), ("envelope_max", "u1", 4), ("rotor_min", "u1", 4),
                           ("rotor_max", "u1", 4), ("reserved", "<u4", 2)])
#: bit 0 of `flags`; the image bits of the call's flags, in the order the images are written
ENVELOPE_RETURNS = 1
ENVELOPE_IMAGES = {"envelope": 1, "stator": 2, "rotor": 4}


def _packed_popcount(words) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8)).sum())


def _packed_box(words) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """(box_min, box_max) of a packed 64^3 state as (x, y, z), inclusive; ((0, 0, 0), (0, 0, 0)) for an empty one."""
    cells = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").ravel().view(np.uint8), bitorder="little").reshape(64, 64, 64)
    xs, ys, zs = (np.flatnonzero(cells.any(axis=a)) for a in ((0, 1), (0, 2), (1, 2)))
    if xs.size == 0:
        return (0, 0, 0), (0, 0, 0)
    return (int(xs[0]), int(ys[0]), int(zs[0])), (int(xs[-1]), int(ys[-1]), int(zs[-1]))


def envelope_of_phases(states) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """`ca3d_ensemble_envelope` of ONE universe whose phases the caller has stepped: `states` is [P + 1, 8192], S_0 .. S_P
    -> (record of ENVELOPE_DTYPE, envelope, stator, rotor), the three images as packed states."""
    s = np.ascontiguousarray(states, dtype="<u4")
    if s.ndim != 2 or s.shape[0] < 2 or s.shape[1] != words_per_buffer(64):
        raise ValueError("states is [P + 1, 8192] with P >= 1: the phases S_0 .. S_P")
    p = s.shape[0] - 1
    if p > CANON_MAX_PERIOD:
        raise ValueError(f"a period is at most {CANON_MAX_PERIOD}")
    env, sta = np.bitwise_or.reduce(s[:p], axis=0), np.bitwise_and.reduce(s[:p], axis=0)
    rot = env & ~sta
    rec = np.zeros((), dtype=ENVELOPE_DTYPE)
    rec["period"] = p
    rec["flags"] = ENVELOPE_RETURNS if np.array_equal(s[p], s[0]) else 0
    rec["heat"] = sum(_packed_popcount(s[t] ^ s[t + 1]) for t in range(p))
    rec["population_sum"] = sum(_packed_popcount(s[t]) for t in range(p))
    rec["envelope_population"], rec["stator_population"] = _packed_popcount(env), _packed_popcount(sta)
    for name, image in (("envelope", env), ("rotor", rot)):
        lo, hi = _packed_box(image)
        rec[name + "_min"][:3], rec[name + "_max"][:3] = lo, hi
    return rec, env, sta, rot


def envelope(state, kind: str, tables, period: int, boundary: str = "reference") -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """`ca3d_ensemble_envelope` for ONE packed 64^3 universe, in plain numpy over `ensemble_step`: the universe is followed over
    `period` steps (1 .. CANON_MAX_PERIOD) of the rule `kind`, `tables` under `boundary`, as `ensemble_step` takes them
    -> (record of ENVELOPE_DTYPE, envelope, stator, rotor). With S_t the state after t steps: the envelope is the OR of S_0 ..
    S_(period-1), the stator their AND, the rotor envelope & ~stator; `heat` sums popcount(S_t ^ S_(t+1)) over t < period,
    `population_sum` popcount(S_t); the boxes are inclusive, zero for an empty set; ENVELOPE_RETURNS (bit 0 of flags) is set exactly
    when S_period equals S_0 word for word. rotor_population, volatility and heat per step: `envelope_derived`."""
    if not 1 <= int(period) <= CANON_MAX_PERIOD:
        raise ValueError(f"a period is 1 .. {CANON_MAX_PERIOD}")
    s = [np.ascontiguousarray(state, dtype="<u4").ravel()]
    for _ in range(int(period)):
        s.append(ensemble_step(s[-1], kind, tables, boundary))
    return envelope_of_phases(np.stack(s))


def envelope_derived(records) -> dict:
    """What follows from ENVELOPE_DTYPE records without another look at the states: `rotor_population` = envelope - stator,
    `volatility` = rotor / envelope (0 for an empty envelope), `heat_per_step` = heat / period, `returns` (bool)."""
    r = np.asarray(records)
    env, rot = r["envelope_population"].astype(np.float64), (r["envelope_population"] - r["stator_population"]).astype(np.uint32)
    return {"rotor_population": rot, "volatility": np.divide(rot, env, out=np.zeros_like(env), where=env != 0),
            "heat_per_step": r["heat"] / np.maximum(r["period"], 1), "returns": (r["flags"] & ENVELOPE_RETURNS) != 0}


# ------------------------------------------------------------------------------------------ damage spreading
# The definition of ca3d_ensemble_damage (include/ca3d.h) in executable form, for one universe.

#: ca3d_damage (include/ca3d.h), 48 bytes; a box corner is x, y, z and a zero byte
DAMAGE_DTYPE = np.dtype([("steps", "<u4"), ("flags", "<u4"), ("healed_at", "<u4"), ("final_distance", "<u4"), ("initial_distance", "<u4"),
                         ("max_distance", "<u4"), ("max_at", "<u4"), ("distance_sum", "<u4"), ("damage_min", "u1", 4), ("damage_max", "u1", 4),
                         ("touched_min", "u1", 4), ("touched_max", "u1", 4)])
#: bit 0 of `flags`; `healed_at` without it; flip words a universe; "the universe itself" among the twins; "no cell" among the flips
DAMAGE_HEALED = 1
DAMAGE_NEVER = 0xFFFFFFFF
DAMAGE_FLIPS = 4
DAMAGE_SELF = 0xFFFFFFFF
DAMAGE_NO_FLIP = 0xFFFFFFFF


def damage_flip_word(cell) -> int:
    """The flip word of cell (x, y, z): x | y << 8 | z << 16."""
    x, y, z = (int(v) for v in cell)
    if not (0 <= x < 64 and 0 <= y < 64 and 0 <= z < 64):
        raise ValueError(f"a flipped cell lies inside the 64^3 universe, not at {(x, y, z)}")
    return x | y << 8 | z << 16


def _damage_over(pairs, p: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(curve, record, D_P) of the pairs (S_t, T_t), t = 0 .. p, that `pairs` yields. It may stop early: after a pair with d_t == 0 it is
    not asked again, and when it ends by itself every later D_t is the last one it gave."""
    curve = np.zeros(p + 1, dtype=np.uint32)
    touched = np.zeros(words_per_buffer(64), dtype=np.uint32)
    for i, (s, t) in enumerate(pairs):
        d = s ^ t
        curve[i] = _packed_popcount(d)
        touched |= d
        if curve[i] == 0 or i == p:
            break
    curve[i:] = curve[i]
    rec = np.zeros((), dtype=DAMAGE_DTYPE)
    zeros = np.flatnonzero(curve == 0)
    rec["steps"] = p
    rec["flags"] = DAMAGE_HEALED if zeros.size else 0
    rec["healed_at"] = zeros[0] if zeros.size else DAMAGE_NEVER
    rec["final_distance"], rec["initial_distance"] = curve[p], curve[0]
    rec["max_distance"], rec["max_at"] = curve.max(), int(np.argmax(curve))
    rec["distance_sum"] = int(curve.astype(np.uint64).sum())
    for name, image in (("damage", d), ("touched", touched)):
        lo, hi = _packed_box(image)
        rec[name + "_min"][:3], rec[name + "_max"][:3] = lo, hi
    return curve, rec, d.astype(np.uint32)


def damage_of_phases(states, twins) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`ca3d_ensemble_damage` of ONE universe whose two trajectories the caller has stepped: `states` is [P + 1, 8192], S_0 .. S_P, and
    `twins` T_0 .. T_P likewise -> (curve, record of DAMAGE_DTYPE, D_P), as `damage` gives them."""
    s, t = np.ascontiguousarray(states, dtype="<u4"), np.ascontiguousarray(twins, dtype="<u4")
    if s.ndim != 2 or s.shape[0] < 2 or s.shape[1] != words_per_buffer(64) or t.shape != s.shape:
        raise ValueError("states and twins are [P + 1, 8192] with P >= 1: S_0 .. S_P and T_0 .. T_P")
    if s.shape[0] - 1 > CANON_MAX_PERIOD:
        raise ValueError(f"a step count is at most {CANON_MAX_PERIOD}")
    return _damage_over(zip(s, t), s.shape[0] - 1)


def damage_twin(state, twin=None, flips=()) -> np.ndarray:
    """T_0 = W ^ F of `damage`: `twin` (None: `state` itself) with the cells (x, y, z) of `flips` XORed in one after another."""
    flips = list(flips)
    if len(flips) > DAMAGE_FLIPS:
        raise ValueError(f"at most {DAMAGE_FLIPS} flips a universe")
    t = np.ascontiguousarray(state if twin is None else twin, dtype="<u4").ravel().astype(np.uint32)
    if t.size != words_per_buffer(64):
        raise ValueError("a universe is 8192 words")
    for cell in flips:
        damage_flip_word(cell)  # inside the universe
        t ^= cells_to_words(64, [tuple(int(v) for v in cell)])
    return t


def damage(state, kind: str, tables, steps: int, boundary: str = "reference", twin=None, flips=()) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`ca3d_ensemble_damage` for ONE packed 64^3 universe, in plain numpy over `ensemble_step`: `state` (S_0) and a perturbed twin are
    followed over `steps` steps (P, 1 .. CANON_MAX_PERIOD) of the rule `kind`, `tables` under `boundary`, as `ensemble_step` takes them
    -> (curve [P + 1] of d_0 .. d_P, record of DAMAGE_DTYPE, D_P as a packed state). The twin starts as T_0 = W ^ F (`damage_twin`): W
    is `twin`, another packed state, or S_0 itself (None); F has exactly the cells (x, y, z) of `flips` set, at most DAMAGE_FLIPS of
    them, XORed in one after another, so a cell listed twice cancels. D_t = S_t ^ T_t, d_t = popcount(D_t). DAMAGE_HEALED (bit 0 of
    flags) is set exactly when some d_t == 0, and `healed_at` is the first such t (DAMAGE_NEVER if none); `max_at` is the first t that
    reaches `max_distance`; `distance_sum` sums d_0 .. d_P; `damage_min` / `damage_max` is the inclusive box of D_P and `touched_min` /
    `touched_max` that of D_0 | .. | D_P, zero for an empty set. Once d_t == 0 both trajectories are one and the rest is zero; once a
    step changes neither state every later sample repeats this one: the stepping stops there, and the result is that of the full P
    steps."""
    p = int(steps)
    if not 1 <= p <= CANON_MAX_PERIOD:
        raise ValueError(f"a step count is 1 .. {CANON_MAX_PERIOD}")
    s0 = np.ascontiguousarray(state, dtype="<u4").ravel().astype(np.uint32)
    if s0.size != words_per_buffer(64):
        raise ValueError("a universe is 8192 words")

    def pairs(s, t):
        while True:
            yield s, t
            s1, t1 = ensemble_step(s, kind, tables, boundary), ensemble_step(t, kind, tables, boundary)
            if np.array_equal(s1, s) and np.array_equal(t1, t):  # two still lifes
                return
            s, t = s1, t1

    return _damage_over(pairs(s0, damage_twin(s0, twin, flips)), p)


# --------------------------------------------------------------------------------------------------- usage
# The definition of ca3d_ensemble_usage (include/ca3d.h) in executable form, for one universe.

USAGE_MAIN, USAGE_EDGES, USAGE_CORNERS, USAGE_BINS = 0, 27, 40, 49
USAGE_CLASSES = {"main": (USAGE_MAIN, 27), "edges": (USAGE_EDGES, 13), "corners": (USAGE_CORNERS, 9)}  # class -> (first bin, bins)
USAGE_DTYPE = np.dtype([("steps", "<u4"), ("flags", "<u4"), ("used_born", "<u4", (3,)), ("used_survive", "<u4", (3,)),
                        ("dead", "<u4", (USAGE_BINS,)), ("alive", "<u4", (USAGE_BINS,)), ("reserved", "<u4", (2,))])
assert USAGE_DTYPE.itemsize == 432


def _usage_classes(kind: str):
    """(first bin, bins) of the tables a kind looks up, in the order of `_ensemble_counts`."""
    if kind not in ENSEMBLE_KINDS:
        raise ValueError(f"unknown ensemble kind {kind!r}: one of {ENSEMBLE_KINDS}")
    if kind == "von neumann":
        return ((USAGE_MAIN, 7),)
    if kind == "moore":
        return ((USAGE_MAIN, 27),)
    return tuple(USAGE_CLASSES.values())


def usage_of_phases(states, kind: str, boundary: str = "reference") -> np.ndarray:
    """The usage record (USAGE_DTYPE, shape ()) of the phases S_0 .. S_(P-1), packed 64^3 states: dead[base + c] / alive[base + c] is
    the number of (t, cell) pairs whose cell is dead / alive in S_t with count c in the class that starts at bin `base`
    (`USAGE_CLASSES`; von Neumann and Moore fill the main class only), the counts as `ensemble_step` forms them under `boundary`;
    used_born[i] / used_survive[i] has bit c set where dead / alive[base_i + c] is not zero."""
    states = list(states)
    if not 1 <= len(states) <= CANON_MAX_PERIOD:
        raise ValueError(f"a step count is 1 .. {CANON_MAX_PERIOD}")
    classes = _usage_classes(kind)
    hist = np.zeros((2, USAGE_BINS), dtype=np.int64)
    for s in states:
        a, counts = _ensemble_counts(s, kind, boundary)
        for (base, n), count in zip(classes, counts):
            hist[:, base:base + n] += np.bincount((a.astype(np.int64) * n + count).ravel(), minlength=2 * n).reshape(2, n)
    rec = np.zeros((), dtype=USAGE_DTYPE)
    rec["steps"] = len(states)
    rec["dead"], rec["alive"] = hist[0], hist[1]
    for i, (base, n) in enumerate(USAGE_CLASSES.values()):
        rec["used_born"][i] = sum(1 << c for c in range(n) if hist[0, base + c])
        rec["used_survive"][i] = sum(1 << c for c in range(n) if hist[1, base + c])
    return rec


def usage(state, kind: str, tables, steps: int, boundary: str = "reference") -> np.ndarray:
    """`ca3d_ensemble_usage` for ONE packed 64^3 universe, in plain numpy over `ensemble_step`: `usage_of_phases` of S_0 = `state` and
    its `steps` - 1 successors under the rule `kind`, `tables` and `boundary`, as `ensemble_step` takes them."""
    p = int(steps)
    if not 1 <= p <= CANON_MAX_PERIOD:
        raise ValueError(f"a step count is 1 .. {CANON_MAX_PERIOD}")
    phases = [np.ascontiguousarray(state, dtype="<u4").ravel().astype(np.uint32)]
    for _ in range(p - 1):
        phases.append(ensemble_step(phases[-1], kind, tables, boundary))
    return usage_of_phases(phases, kind, boundary)


def usage_dont_care(record, kind: str) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(born[3], survive[3]): per class (main, edges, corners) the mask of table bits the run behind `record` never read. Flipping
    any of them leaves every state of that run as it is. A class the kind does not look up has no bits at all (0)."""
    born, survive = [0, 0, 0], [0, 0, 0]
    for i, (_, n) in enumerate(_usage_classes(kind)):  # (the classes a kind looks up come first)
        full = (1 << n) - 1
        born[i] = full & ~int(record["used_born"][i])
        survive[i] = full & ~int(record["used_survive"][i])
    return tuple(born), tuple(survive)


def usage_births_deaths(record, kind: str, tables) -> Tuple[int, int]:
    """(births, deaths) summed over the steps of the run behind `record`: the sum over c of dead[c] born_c and of
    alive[c] (1 - survive_c). Exact for "von neumann" and "moore"; a clustered cell's three lookups are ORed, which the three
    histograms do not determine: ValueError."""
    if kind == "clustered":
        raise ValueError("a clustered universe's three lookups are ORed: births and deaths do not follow from the histograms")
    ((base, n),) = _usage_classes(kind)
    born, survive = tables
    births = sum(int(record["dead"][base + c]) for c in range(n) if int(born) >> c & 1)
    deaths = sum(int(record["alive"][base + c]) for c in range(n) if not int(survive) >> c & 1)
    return births, deaths


# ------------------------------------------------------------------------------------------------- windows
# The definition of ca3d_cut_windows / ca3d_stamp_windows (include/ca3d.h) in executable form: 64^3 windows of a packed G^3 grid,
# addressed as a torus, against packed 64^3 universes.

#: ca3d_window (include/ca3d.h), 16 bytes
WINDOW_DTYPE = np.dtype([("universe", "<u4"), ("origin", "<u4", (3,))])
STAMP_MODES = ("or", "replace", "erase")  # index = enum CA3D_STAMP_*


def window_records(windows) -> np.ndarray:
    """[(universe, (x, y, z)), ...] as records of `WINDOW_DTYPE`. Values are handed over as given (modulo 2^32): the library refuses
    what does not fit."""
    out = np.zeros(len(windows), dtype=WINDOW_DTYPE)
    for k, (universe, origin) in enumerate(windows):
        if len(origin) != 3:
            raise ValueError("a window is (universe, (x, y, z))")
        out[k]["universe"] = int(universe) & 0xFFFFFFFF
        out[k]["origin"] = [int(v) & 0xFFFFFFFF for v in origin]
    return out


def window_tiling(grid_size: int) -> np.ndarray:
    """The origins (x, y, z) of ceil(G / 64)^3 windows that tile a grid of G, x fastest: every cell lies in exactly one window when 64
    divides G; otherwise the last window of an axis wraps round and covers cells of the first again -> i64[n, 3]."""
    G = int(grid_size)
    if G < 64:
        raise ValueError("a window is 64^3 cells: the grid must be 64 or more a side")
    at = 64 * np.arange(-(-G // 64))
    z, y, x = np.meshgrid(at, at, at, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def _window_axes(G: int, origin):
    ox, oy, oz = (int(v) for v in origin)
    if G < 64 or G % 32 or not all(0 <= v < G for v in (ox, oy, oz)):
        raise ValueError("a window's origin lies inside a grid of 64 or more a side")
    i = np.arange(64)
    return (ox + i) % G, (oy + i) % G, (oz + i) % G


def _window_rows(grid: np.ndarray, yi, zi) -> np.ndarray:
    """Cells [64 k, 64 j, G x] of the grid rows a window touches; `grid`: [G, G, G / 32] words."""
    rows = np.ascontiguousarray(grid[np.ix_(zi, yi)])
    return np.unpackbits(rows.view(np.uint8), axis=-1, bitorder="little")


def cut_window(grid_size: int, words, origin) -> np.ndarray:
    """`ca3d_cut_windows` for ONE window of a packed G^3 state: window cell (i, j, k), each 0 .. 63, is grid cell
    ((ox + i) mod G, (oy + j) mod G, (oz + k) mod G) -> words u32[8192] of a 64^3 universe."""
    G = int(grid_size)
    xi, yi, zi = _window_axes(G, origin)
    grid = np.ascontiguousarray(words, dtype="<u4").reshape(G, G, G // 32)
    cells = _window_rows(grid, yi, zi)[:, :, xi]
    return np.packbits(np.ascontiguousarray(cells).ravel(), bitorder="little").view("<u4").copy()


def stamp_windows(grid_size: int, words, windows, mode: str = "or") -> np.ndarray:
    """`ca3d_stamp_windows` on a packed G^3 state: `windows` is a list of (universe_words u32[8192], (ox, oy, oz)). "or": every live cell
    of a universe, mapped as in `cut_window`, is set; "erase": those cells are cleared; "replace": every cell of every window's box is
    cleared first, then every universe is ORed in. The result does not depend on the order of the windows -> the new words."""
    G = int(grid_size)
    if mode not in STAMP_MODES:
        raise ValueError(f"unknown mode {mode!r}: one of {STAMP_MODES}")
    out = np.array(words, dtype="<u4").reshape(G, G, G // 32)
    phases = (("clear", "or") if mode == "replace" else (mode,))
    for phase in phases:
        for universe, origin in windows:
            xi, yi, zi = _window_axes(G, origin)
            cells = _window_rows(out, yi, zi)
            if phase == "clear":
                cells[:, :, xi] = 0
            else:
                u = np.unpackbits(np.ascontiguousarray(universe, dtype="<u4").reshape(64, 64, 2).view(np.uint8), axis=-1, bitorder="little")
                cells[:, :, xi] = cells[:, :, xi] | u if phase == "or" else cells[:, :, xi] & (1 - u)
            out[np.ix_(zi, yi)] = np.packbits(cells, axis=-1, bitorder="little").view("<u4")
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ renderer
# The 128-float common uniform block (MemoryManager.js; allocation order main_pathtraced.js:166, 467-478 ==
# struct CommonBufferLayout, pathtraced_fragment_clustered.wgsl:17-34). Matrices are column-major f32.

UNIFORM_INDEX = {
    "light": 0, "viewMat": 4, "projViewMatInv": 20, "prevViewMat": 36, "prevProjViewMatInv": 52, "windowSize": 68,
    "elapsedTime": 70, "depthSamples": 71, "shadowSamples": 72, "cellSize": 73, "showDepthOverlay": 74,
    "temporalAlpha": 75, "baseReflectivity": 76, "roughness": 79, "materialColor": 80, "gamma": 83,
}

RENDER_DEFAULTS = {  # main_pathtraced.js:116-121, 135-152, 164-165
    "light": (0.721, 1.0, 1.0, 5.0), "depthSamples": 35, "shadowSamples": 30, "cellSize": 0.85, "showDepthOverlay": 0,
    "temporalAlpha": 0.1, "baseReflectivity": (0.17, 0.17, 0.17), "roughness": 0.29, "materialColor": (0.0, 0.0, 0.0),
    "gamma": 2.0, "fov_deg": 75.0, "near": 0.01, "far": 1000.0,
}


def mat4_perspective(fov_rad: float, aspect: float, near: float, far: float) -> np.ndarray:
    """wgpu-matrix mat4.perspective (libs/wgpu-matrix.module.js:3140): depth 0..1, column-major."""
    f = np.float32(math.tan(math.pi * 0.5 - 0.5 * fov_rad))
    m = np.zeros(16, dtype=np.float32)
    m[0] = f / np.float32(aspect)
    m[5] = f
    m[11] = -1.0
    range_inv = np.float32(1.0 / (near - far))
    m[10] = np.float32(far) * range_inv
    m[14] = np.float32(far) * np.float32(near) * range_inv
    return m


def mat4_multiply(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """mat4.multiply(a, b) = a * b on column-major arrays."""
    A = np.asarray(a, dtype=np.float32).reshape(4, 4).T
    B = np.asarray(b, dtype=np.float32).reshape(4, 4).T
    return (A @ B).T.reshape(16).astype(np.float32)


def mat4_inverse(m: np.ndarray) -> np.ndarray:
    M = np.asarray(m, dtype=np.float64).reshape(4, 4).T
    return np.linalg.inv(M).T.reshape(16).astype(np.float32)


def camera_matrix(position=(0.0, 0.0, 0.75), axis=(0.0, 1.0, 0.0), angle_rad: float = 0.0) -> np.ndarray:
    """Camera-to-world `viewMat` (the shader reads cameraPos = viewMat[3].xyz, :812): rotation about `axis`
    followed by translation to `position`. Default = the reference's start pose (main_pathtraced.js:207-213)."""
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    c, s = math.cos(angle_rad), math.sin(angle_rad)
    x, y, z = ax
    R = np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                  [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                  [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = position
    return M.T.reshape(16).astype(np.float32)


def orbit_camera(distance: float = 1.4, axis=(1.0, 1.0, 0.0), angle_rad: float = 0.6) -> np.ndarray:
    """The oblique bench pose: rotate about `axis`, camera at `distance` looking at the origin."""
    m = camera_matrix((0.0, 0.0, 0.0), axis, angle_rad).reshape(4, 4).T.astype(np.float64)
    pos = m[:3, :3] @ np.array([0.0, 0.0, distance])
    return camera_matrix(tuple(pos), axis, angle_rad)


def uniform_block(width: int, height: int, view_mat: Optional[np.ndarray] = None, elapsed_time: float = 0.5,
                  prev_view_mat: Optional[np.ndarray] = None, **overrides) -> np.ndarray:
    """Fill the common block the way `_setupUniformsMemoryCPU` / `_updateMatrices` / `_updateUIValues` do
    (main_pathtraced.js:464-518, 1762-1773). `overrides` may set any key of RENDER_DEFAULTS."""
    p = dict(RENDER_DEFAULTS)
    for k, v in overrides.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    u = np.zeros(128, dtype=np.float32)
    if view_mat is None:
        view_mat = camera_matrix()
    view_mat = np.asarray(view_mat, dtype=np.float32)
    proj = mat4_perspective(p["fov_deg"] * math.pi / 180.0, width / height, p["near"], p["far"])
    pvi = mat4_multiply(proj, mat4_inverse(view_mat))
    I = UNIFORM_INDEX
    u[I["light"]:I["light"] + 4] = p["light"]
    u[I["viewMat"]:I["viewMat"] + 16] = view_mat
    u[I["projViewMatInv"]:I["projViewMatInv"] + 16] = pvi
    if prev_view_mat is not None:
        prev_view_mat = np.asarray(prev_view_mat, dtype=np.float32)
        u[I["prevViewMat"]:I["prevViewMat"] + 16] = prev_view_mat
        u[I["prevProjViewMatInv"]:I["prevProjViewMatInv"] + 16] = mat4_multiply(proj, mat4_inverse(prev_view_mat))
    u[I["windowSize"]:I["windowSize"] + 2] = (width, height)
    u[I["elapsedTime"]] = elapsed_time
    for k in ("depthSamples", "shadowSamples", "cellSize", "showDepthOverlay", "temporalAlpha", "roughness", "gamma"):
        u[I[k]] = p[k]
    u[I["baseReflectivity"]:I["baseReflectivity"] + 3] = p["baseReflectivity"]
    u[I["materialColor"]:I["materialColor"] + 3] = p["materialColor"]
    return u


# --------------------------------------------------------------------------------------------- checkpoints
# The reference keeps its state only in GPU buffers and never reads it back; the engine's
# read_state / upload_state on the raw little-endian words IS the checkpoint payload. The file adds a header.

CHECKPOINT_MAGIC = b"CA3D"
CHECKPOINT_VERSION = 1


def save_checkpoint(path, words: np.ndarray, grid_size: int, step: int = 0, layout: int = 0) -> None:
    """magic 'CA3D' | u32 version | u32 grid size | u32 layout | u64 step | u64 word count | LE u32 words."""
    import struct

    w = np.ascontiguousarray(words, dtype="<u4")
    with open(path, "wb") as f:
        f.write(CHECKPOINT_MAGIC + struct.pack("<IIIQQ", CHECKPOINT_VERSION, grid_size, layout, step, w.size))
        f.write(w.tobytes())


def load_checkpoint(path):
    """-> (words, grid_size, step, layout); raises ValueError on a malformed file."""
    import struct

    with open(path, "rb") as f:
        head = f.read(4 + 28)
        if len(head) != 32 or head[:4] != CHECKPOINT_MAGIC:
            raise ValueError("not a CA3D checkpoint")
        version, grid_size, layout, step, n = struct.unpack("<IIIQQ", head[4:])
        if version != CHECKPOINT_VERSION:
            raise ValueError(f"unsupported checkpoint version {version}")
        expect = (grid_size // 32) * grid_size * grid_size if layout == 0 else grid_size ** 3
        if n != expect:
            raise ValueError("word count does not match the grid size")
        words = np.frombuffer(f.read(n * 4), dtype="<u4")
        if words.size != n:
            raise ValueError("truncated checkpoint")
    return words.astype(np.uint32), grid_size, step, layout
