"""The scene of the colour layer's tests (tests/test_gpu_colour.py, tests/test_colour_ref.py): a loaded volume with a wall and a
floor, three cameras, and their frames.  Plain numpy; the parameter object is anything with lv_colour_params' fields."""
import types

import numpy as np

F = np.float32
RGB8, BGR8, MONO8 = 0, 1, 2   # LV_IMAGE_*

NX, NY, NZ = 64, 64, 32
RES = 0.2
ORIGIN = (-6.4, -6.4, -3.2)
TRUNC_CELLS = 3
T = TRUNC_CELLS * 256
WALL_X, FLOOR_Z = 5.03, -0.97
EYES = ((0.13, -0.21, 0.37), (1.31, 2.17, 0.93), (-2.07, 0.55, 1.49))
TARGETS = ((5.0, 1.0, -0.5), (5.0, -1.0, -0.8), (4.0, 0.5, -1.0))
DIST = (-0.05, 0.01, 0.001, -0.0005, 0.0)
FLAT = ((200, 40, 90), (130, 220, 10), (77, 77, 77))   # r, g, b each view's flat image shows
# (zbuf_scale, window, image width, height, focal length): the settings the parity is held at
SETTINGS = ((16, 1, 640, 480, 400.0), (8, 2, 640, 480, 400.0), (16, 2, 640, 480, 400.0), (4, 1, 160, 120, 100.0))


def look_at(t, target):
    """R camera -> world (x right, y down, z forward) of a camera at t looking at target, the world's z up."""
    z = np.asarray(target, np.float64) - np.asarray(t, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1).astype(F)


def volume(nx=NX, ny=NY, nz=NZ, origin=ORIGIN, seed=3):
    """(S, W) [nz, ny, nx] int32: S = W * clip(floor(256 d / res), -T, T), d the signed distance to the nearer of the wall
    x = 5.03 and the floor z = -0.97, positive on the cameras' side; W in 1..3: a tenth of the voxels at 1 (below the tests'
    min_weight of 2), a twentieth at 0."""
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    x = origin[0] + RES * (i + 0.5)
    z = origin[2] + RES * (k + 0.5)
    d_wall, d_floor = WALL_X - x, z - FLOOR_Z
    d = np.where(np.abs(d_wall) < np.abs(d_floor), d_wall, d_floor)
    W = rng.integers(2, 4, (nz, ny, nx)).astype(np.int32)
    W[rng.uniform(size=W.shape) < 0.10] = 1
    W[rng.uniform(size=W.shape) < 0.05] = 0
    S = (W * np.clip(np.floor(256.0 * d / RES), -T, T)).astype(np.int32)
    return S, W


def frames(width=640, height=480, focal=400.0, images=None, n=3):
    """The three views (rgb8 with strided rows, bgr8 with distortion, mono8); images: three [h, w, 3] / [h, w] uint8 arrays in
    the views' formats, default the flat ones."""
    k = width / 640.0
    out = []
    for v in range(n):
        fmt = (RGB8, BGR8, MONO8)[v % 3]
        if images is not None:
            img = images[v]
        elif fmt == MONO8:
            img = np.full((height, width), FLAT[v % 3][0], np.uint8)
        else:
            rgb = FLAT[v % 3]
            img = np.empty((height, width, 3), np.uint8)
            img[:] = rgb[::-1] if fmt == BGR8 else rgb
        if fmt == RGB8:   # rows 21 bytes apart from packed
            wide = np.zeros((height, width + 7, 3), np.uint8)
            wide[:, :width] = img
            img = wide[:, :width]
        e = np.asarray(EYES[v % 3], np.float64) + 0.01 * (v // 3) * np.array([1.0, -1.0, 0.5])
        out.append(dict(R=look_at(e, TARGETS[v % 3]), t=e.astype(F), fx=focal, fy=focal, cx=319.63 * k, cy=240.21 * k, image=img, format=fmt,
                        dist=np.asarray(DIST if fmt == BGR8 else np.zeros(5), F)))
    return out


def colour_params(zbuf_scale=16, window=1, band=256, min_weight=2, max_weight=64, margin_abs=0.5):
    """lv_colour_params' fields as a plain object (the defaults of lv_default_colour_params otherwise)."""
    view = types.SimpleNamespace(min_depth=0.3, max_depth=60.0, max_norm_radius=1.5, zbuf_scale=zbuf_scale, window=window,
                                 margin_abs=margin_abs, margin_rel=0.01, blend=0)
    return types.SimpleNamespace(view=view, band=band, min_weight=min_weight, max_weight=max_weight, reserved=0)
