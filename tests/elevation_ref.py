"""The elevation map's rule (include/limovelo_hip.h "Elevation map") in numpy: the reference that lv_elevation.hpp on the host
(tests/test_elevation_host.py) and the kernels of lv_elevation.hip (tests/test_gpu_elevation.py) are held to, by equality.  The
quantisation is f32 in the documented order; everything after it is integers (np.minimum.at, np.maximum.at, bincount, and a
plain loop for the stencil)."""
import math

import numpy as np

F = np.float32
NONE = 2147483647
SLOPE_MAX = 2 ** 31 - 1
LAYERS = ("lo", "top", "span", "step", "slope2", "count", "band_count", "cls", "height")   # in the order of LV_ELEV_LO ..


def params(origin=(-51.2, -51.2, -3.2), resolution=0.2, nx=512, ny=512, min_points=3, head=1920, max_span=153, max_step=128, max_slope2=34727):
    return dict(origin=tuple(float(F(v)) for v in origin), resolution=float(F(resolution)), nx=int(nx), ny=int(ny), min_points=int(min_points),
                head=int(head), max_span=int(max_span), max_step=int(max_step), max_slope2=int(max_slope2))


def quant(prm, pts):
    """(ok [n] bool, q [n, 3] int64): floorf(((p - origin) / resolution) * 256) per axis in f32; ok: finite and |q| < 2^24 on all."""
    p = np.asarray(pts, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = np.floor(((p - np.array(prm["origin"], F)) / F(prm["resolution"])) * F(256.0))
        assert f.dtype == F
        ok = (np.abs(f) < F(16777216.0)).all(axis=1)
    return ok, np.where(ok[:, None], f, 0).astype(np.int64)


def cells_of(prm, pts, planar=False):
    """(used [n] bool, cell [n] int64 (0 where not used), z [n] int64).  planar: z is neither quantised nor judged (the query)."""
    p = np.array(np.asarray(pts, F).reshape(-1, 3))
    if planar:
        p[:, 2] = prm["origin"][2]
    ok, q = quant(prm, p)
    i, j = q[:, 0] >> 8, q[:, 1] >> 8
    used = ok & (i >= 0) & (i < prm["nx"]) & (j >= 0) & (j < prm["ny"])
    return used, np.where(used, j * prm["nx"] + i, 0), q[:, 2]


def build(prm, pts):
    """(layers, stats): layers maps each name of LAYERS to its [ny, nx] array (int32, uint32, int8, f32 as the library's); stats
    uint64 [4]: points used, overhang points, known cells, lethal cells."""
    nx, ny = prm["nx"], prm["ny"]
    nc = nx * ny
    used, cell, z = cells_of(prm, pts)
    cell, z = cell[used], z[used]
    n = np.bincount(cell, minlength=nc).astype(np.int64)
    lo = np.full(nc, NONE, np.int64)
    np.minimum.at(lo, cell, z)
    band = z - lo[cell] <= prm["head"]
    nb = np.bincount(cell[band], minlength=nc).astype(np.int64)
    top = np.full(nc, -NONE, np.int64)
    np.maximum.at(top, cell[band], z[band])
    known = (nb >= prm["min_points"]).reshape(ny, nx)
    lo2, top2 = lo.reshape(ny, nx), top.reshape(ny, nx)
    span = np.zeros((ny, nx), np.int64)
    step = np.zeros((ny, nx), np.int64)
    slope2 = np.zeros((ny, nx), np.int64)

    def kn(i, j):
        return 0 <= i < nx and 0 <= j < ny and bool(known[j, i])

    def grad(l0, m, p):   # m, p: (i, j) of the cells at -1 and +1
        km, kp = kn(*m), kn(*p)
        if km and kp:
            return int(lo2[p[1], p[0]]) - int(lo2[m[1], m[0]])
        if kp:
            return 2 * (int(lo2[p[1], p[0]]) - l0)
        if km:
            return 2 * (l0 - int(lo2[m[1], m[0]]))
        return 0

    for j, i in zip(*np.nonzero(known)):
        i, j = int(i), int(j)
        l0 = int(lo2[j, i])
        span[j, i] = int(top2[j, i]) - l0
        s = 0
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if (di or dj) and kn(i + di, j + dj):
                    s = max(s, abs(int(lo2[j + dj, i + di]) - l0))
        step[j, i] = s
        gx, gy = grad(l0, (i - 1, j), (i + 1, j)), grad(l0, (i, j - 1), (i, j + 1))
        slope2[j, i] = min(gx * gx + gy * gy, SLOPE_MAX)   # (python integers: exact)
    lethal = known & ((span > prm["max_span"]) | (step > prm["max_step"]) | (slope2 > prm["max_slope2"]))
    cls = np.where(known, np.where(lethal, 100, 0), -1).astype(np.int8)
    with np.errstate(all="ignore"):
        c = np.where(known, lo2, 0).astype(F) / F(256.0)
        m = F(prm["resolution"]) * c
        height = np.where(known, F(prm["origin"][2]) + m, F(np.nan)).astype(F)
    layers = dict(lo=lo2.astype(np.int32), top=top2.astype(np.int32), span=span.astype(np.int32), step=step.astype(np.int32),
                  slope2=slope2.astype(np.int32), count=n.reshape(ny, nx).astype(np.uint32), band_count=nb.reshape(ny, nx).astype(np.uint32),
                  cls=cls, height=height)
    stats = np.array([len(cell), int((~band).sum()), int(known.sum()), int(lethal.sum())], np.uint64)
    return layers, stats


def query(prm, layers, pts):
    """(height [n] f32, cls [n] int8) of the cell of every point's x, y; NaN and -1 where it has none."""
    used, cell, _ = cells_of(prm, pts, planar=True)
    h = np.where(used, layers["height"].reshape(-1)[cell], F(np.nan)).astype(F)
    k = np.where(used, layers["cls"].reshape(-1)[cell], -1).astype(np.int8)
    return h, k


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_layers(got, want):
    """None, or the first layer that differs with where it does."""
    for name in LAYERS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if not same_bits(g, w):
            if g.shape != w.shape or g.dtype != w.dtype:
                return name, (g.shape, g.dtype, w.shape, w.dtype)
            u = np.dtype("u%d" % g.dtype.itemsize)
            return name, np.argwhere(g.view(u) != w.view(u))[:6].tolist()
    return None


def sub_units(metres, resolution):
    return int(math.floor(float(metres) / float(resolution) * 256))


def distance_cells_obstacles(cells, unknown_is_obstacle):
    """[ny, nx] bool: the obstacles lv_occ_distance_build_cells reads out of a plane of cells."""
    c = np.asarray(cells, np.int8)
    return (c == 100) | ((c < 0) if unknown_is_obstacle else np.zeros(c.shape, bool))
