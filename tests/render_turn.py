"""Scenes turned by the 24 proper rotations of the cube — TEST INFRASTRUCTURE, no GPU.

The volume is centred on the origin and cell c sits at (c + 1/2) / G - 1/2 on every axis, so a signed permutation of the axes maps cells
onto cells exactly: an index flip is an exact mirror. Turning the cells, the camera and the light together by the same rotation Q gives
the same picture from code that sees every sign and every dominant axis of a ray changed: the renderer's counterpart of the graded
states of the CA step. A rotation is a 3 x 3 integer matrix in the convention of `host.orientation_matrix`: a point or
direction v (x, y, z) turns into Q @ v."""
import itertools

import numpy as np

from cellularautomatons3d_amd import host


def _rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            q = np.zeros((3, 3), dtype=np.int64)
            for i in range(3):
                q[i, perm[i]] = signs[i]
            if round(np.linalg.det(q)) == 1:
                out.append(q)
    assert len(out) == 24 and np.array_equal(out[0], np.eye(3, dtype=np.int64))
    return tuple(out)


#: the 24 proper rotations of the cube as signed permutation matrices; ROTATIONS[0] is the identity
ROTATIONS = _rotations()


def _view_axis_six():
    """One rotation index for each of the six directions the start pose's view axis -z can be turned to: +x, -x, +y, -y, +z, -z."""
    six = []
    for axis in range(3):
        for sign in (1, -1):
            want = np.zeros(3, dtype=np.int64)
            want[axis] = sign
            six.append(next(k for k, q in enumerate(ROTATIONS) if k and np.array_equal(q @ np.array([0, 0, -1]), want)))
    return tuple(six)


#: six of the 24 (the identity not among them) that take the view axis -z to +x, -x, +y, -y, +z, -z
VIEW_AXIS_SIX = _view_axis_six()


def _perm_signs(Q):
    Q = np.asarray(Q)
    host.orientation_from_matrix(Q)  # anything but a signed permutation matrix is a ValueError
    perm = tuple(int(np.flatnonzero(Q[i])[0]) for i in range(3))
    return perm, tuple(int(Q[i, perm[i]]) for i in range(3))


def turn_cells(words, G, Q):
    """The packed state (bit b of word w + C * (y + G * z) is cell x = 32 w + b) turned by Q: the cell at c goes to c' with
    c'[i] = c[perm[i]], or G - 1 - c[perm[i]] where Q[i, perm[i]] is -1. Unpack, transpose, flip, repack; G any multiple of 32."""
    if G % 32:
        raise ValueError("G is a multiple of 32")
    perm, signs = _perm_signs(Q)
    w = np.ascontiguousarray(words, dtype="<u4").ravel()
    if w.size != host.words_per_buffer(G):
        raise ValueError("words does not hold a G^3 state")
    a = np.unpackbits(w.view(np.uint8), bitorder="little").reshape(G, G, G).transpose(2, 1, 0)  # a[x, y, z]
    b = a.transpose(perm)  # b[j] = a[c] with j[i] = c[perm[i]]
    for i in range(3):
        if signs[i] < 0:
            b = np.flip(b, axis=i)
    return np.packbits(np.ascontiguousarray(b.transpose(2, 1, 0)).ravel(), bitorder="little").view("<u4").astype(np.uint32)


def turn_view(view_mat, Q):
    """The camera-to-world matrix (16 floats, column-major, as `host.camera_matrix` returns it) turned by Q: rotation part and position.
    Exact in float32: Q only permutes and negates."""
    m = np.asarray(view_mat, dtype=np.float32).reshape(4, 4).T
    q4 = np.eye(4, dtype=np.float32)
    q4[:3, :3] = np.asarray(Q, dtype=np.float32)
    return np.ascontiguousarray((q4 @ m).T).reshape(16).astype(np.float32)


def turn_light(light, Q):
    """The light (x, y, z[, magnitude]) turned by Q; the magnitude stays."""
    l = tuple(float(v) for v in light)
    p = np.asarray(Q, dtype=np.float64) @ np.array(l[:3])
    return tuple(float(v) for v in p) + l[3:]


def turned_scene(cells, G, Q, W, H, view_mat=None, **overrides):
    """(turned cells, uniform block of the turned camera and light): what every turned test renders. `overrides` as in
    `host.uniform_block`; its light, or the default one, is turned too."""
    vm = host.camera_matrix() if view_mat is None else view_mat
    light = overrides.pop("light", host.RENDER_DEFAULTS["light"])
    return turn_cells(cells, G, Q), host.uniform_block(W, H, turn_view(vm, Q), light=turn_light(light, Q), **overrides)


def bin_names():
    """The 24 (octant, dominant axis) bins in the order `ray_census` counts them, as text like '+-+ y'."""
    return [f"{'+' if o & 1 else '-'}{'+' if o & 2 else '-'}{'+' if o & 4 else '-'} {'xyz'[a]}" for o in range(8) for a in range(3)]


def _bins(d):
    octant = (d[..., 0] > 0).astype(np.int64) + 2 * (d[..., 1] > 0) + 4 * (d[..., 2] > 0)
    return octant * 3 + np.abs(d).argmax(-1)


def ray_bins(u, depth, W, H, spp=1, view_mat=None, light=None):
    """Per pixel: (hit mask [H, W], bin of the primary ray [H, W], bin of the direction from the hit point to the light [H, W]).

    Ray directions come from the uniform block the way the oracle's shade_sample does (render_oracle.c get_ray, mat_dir): the pixel's
    first sample at ((px + o) / W, 1 - (py + o) / H), o = 1/2 at one sample a pixel and 1/4 at four (the sample whose depth a frame
    stores), the camera-space ray normalize((u - 1/2) W / H, v - 1/2, -cot(37.5 deg) / 2) through the rotation part of viewMat. Hit
    points are camera + ray * depth with the ORACLE's depth. A pixel has hit a cell when that depth is shorter than the ray's way out
    of the volume (a miss stores the exit depth, 0 outside the volume's silhouette): visible cubes are shrunk by cellSize, so a hit
    never lies within 1e-5 of the exit. `view_mat` and `light` default to the block's own."""
    u = np.asarray(u, dtype=np.float32)
    I = host.UNIFORM_INDEX
    vm = np.asarray(u[I["viewMat"]:I["viewMat"] + 16] if view_mat is None else view_mat, dtype=np.float32).reshape(4, 4).T
    lpos = np.asarray(u[I["light"]:I["light"] + 3] if light is None else light, dtype=np.float32)[:3]
    o = np.float32(0.5 if spp == 1 else 0.25)
    vu = ((np.arange(W, dtype=np.float32) + o) / np.float32(W))[None, :]
    vv = (np.float32(1.0) - (np.arange(H, dtype=np.float32) + o) / np.float32(H))[:, None]
    r = u[I["windowSize"]] / u[I["windowSize"] + 1]
    z = np.float32(0.5) * np.float32(1.0 / np.tan(37.5 * 3.14159265359 / 180.0))
    cam_dir = np.stack(np.broadcast_arrays((vu - np.float32(0.5)) * r, vv - np.float32(0.5), -z), axis=-1).astype(np.float32)
    cam_dir /= np.sqrt((cam_dir * cam_dir).sum(-1, keepdims=True))
    ray = cam_dir @ vm[:3, :3].T
    cam = vm[:3, 3]
    d = np.asarray(depth, dtype=np.float32)
    d = d[..., 0] if d.ndim == 3 else d
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / ray.astype(np.float64)
        t_exit = np.maximum((-0.5 - cam) * inv, (0.5 - cam) * inv).min(-1)
    hit = (d > 0) & (d < t_exit - 1e-5)
    p = cam + ray * d[..., None]
    return hit, _bins(ray), _bins(lpos - p)


def ray_census(u, view_mat, light, depth, W, H, spp=1):
    """Two arrays of 24 counts over the pixels that hit a cell: primary ray directions, and the directions from the hit point to the
    light, binned by sign octant (bit 0: x ascending, bit 1: y, bit 2: z) times 3 plus the dominant axis; `bin_names()` names them."""
    hit, primary, shadow = ray_bins(u, depth, W, H, spp, view_mat, light)
    return np.bincount(primary[hit], minlength=24), np.bincount(shadow[hit], minlength=24)
