"""The occupancy grid's rule (include/limovelo_hip.h "Occupancy grid") in numpy: what tests/test_occupancy_host.py holds the host
build of lv_occupancy.hpp to and tests/test_gpu_occupancy.py the kernels, voxel for voxel.  Quantisation in np.float32 operations
in the stated order, the walk vectorised over the rays in int64, the sets boolean arrays."""
import numpy as np

F = np.float32
Q = 256
T_LIMIT = F(8192.0)
Q_LIMIT = F(16777216.0)
FIELDS = ("origin", "resolution", "nx", "ny", "nz", "min_range", "max_range", "l_hit", "l_miss", "l_min", "l_max", "l_occ", "l_free")


def params(**kw):
    """A plain dict of the parameters (the defaults of lv_default_occupancy_params, overridden by kw)."""
    p = dict(origin=(-51.2, -51.2, -3.2), resolution=0.2, nx=512, ny=512, nz=64, min_range=1.0, max_range=80.0, l_hit=0.85,
             l_miss=-0.4, l_min=-2.0, l_max=3.5, l_occ=0.4, l_free=-0.4)
    p.update(kw)
    return p


def params_of(cp):
    """The dict of a capi.OccupancyParams."""
    return {f: (tuple(float(v) for v in cp.origin) if f == "origin" else getattr(cp, f)) for f in FIELDS}


def quant_f(p, origin, resolution):
    """floorf(((p - origin) / resolution) * 256) in f32, as f32 (per axis; p [..., 3] or a scalar with scalar origin)."""
    with np.errstate(all="ignore"):
        return np.floor(((np.asarray(p, F) - np.asarray(origin, F)) / F(resolution)) * F(Q))


def view_origin(prm, t):
    """qs [3] int64 of the sensor origin t, or None when the view gives no evidence."""
    with np.errstate(all="ignore"):
        c = (np.asarray(t, F) - np.asarray(prm["origin"], F)) / F(prm["resolution"])
        if not np.all(np.abs(c) < T_LIMIT):
            return None
        return np.floor(c * F(Q)).astype(np.int64)


def returns(prm, R, t, pts):
    """(qe [m, 3] int64, hit [m] bool) of the returns of one view that are not ignored; hit False: the return was cut."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    R = np.asarray(R, F).reshape(3, 3)
    t = np.asarray(t, F).reshape(3)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r2 = x * x + y * y + z * z
        mn, mx = F(prm["min_range"]), F(prm["max_range"])
        keep = finite & ~(r2 < mn * mn)
        cut = r2 > mx * mx
        c = np.where(cut, mx / np.sqrt(r2), F(1)).astype(F)
        x, y, z = (np.where(cut, v * c, v).astype(F) for v in (x, y, z))
        qf = np.stack([quant_f(((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a], prm["origin"][a], prm["resolution"]) for a in range(3)],
                      axis=1)
        keep &= np.all(np.abs(qf) < Q_LIMIT, axis=1)   # (NaN fails too)
    return qf[keep].astype(np.int64), ~cut[keep]


def walk(qs, qe):
    """The cells of every walk qs [3] or [m, 3] -> qe [m, 3] (int64 sub-units): a list over the steps of (cells [m, 3], alive [m]):
    cells[i] is the cell ray i stands in BEFORE its step of that index, alive[i] whether it still has that step to make.  Also
    returns ve [m, 3]."""
    qe = np.asarray(qe, np.int64).reshape(-1, 3)
    qs = np.broadcast_to(np.asarray(qs, np.int64), qe.shape)
    d = qe - qs
    ad = np.abs(d)
    s = np.sign(d)
    v = qs >> 8
    ve = qe >> 8
    r = np.abs(ve - v)
    n = np.where(s > 0, ((v + 1) << 8) - qs, np.where(s < 0, qs - (v << 8), 0))
    v = v.copy()
    steps = []
    while True:
        alive = np.any(r > 0, axis=1)
        if not alive.any():
            break
        steps.append((v.copy(), alive))
        a = np.full(len(qe), -1, np.int64)
        for b in range(3):
            can = r[:, b] > 0
            first = a < 0
            # b replaces a unless n_a * ad_b <= n_b * ad_a (a the lower axis keeps the tie)
            ia = np.maximum(a, 0)
            na, ada = np.take_along_axis(n, ia[:, None], 1)[:, 0], np.take_along_axis(ad, ia[:, None], 1)[:, 0]
            better = ~(na * ad[:, b] <= n[:, b] * ada)
            a = np.where(can & (first | better), b, a)
        idx = np.nonzero(alive)[0]
        ax = a[idx]
        v[idx, ax] += s[idx, ax]
        n[idx, ax] += Q
        r[idx, ax] -= 1
    assert np.array_equal(v, ve)
    return steps, ve


def view_sets(prm, R, t, pts):
    """(free [nz, ny, nx] bool, hit [nz, ny, nx] bool, rays used, rays cut) of one view: Free_v (already without Hit_v), Hit_v."""
    nx, ny, nz = prm["nx"], prm["ny"], prm["nz"]
    free = np.zeros((nz, ny, nx), bool)
    hit = np.zeros((nz, ny, nx), bool)
    qs = view_origin(prm, t)
    pts = np.asarray(pts, F).reshape(-1, 3)
    if qs is None or len(pts) == 0:
        return free, hit, 0, 0
    qe, is_hit = returns(prm, R, t, pts)
    if len(qe) == 0:
        return free, hit, 0, 0

    def mark(dst, cells, sel):
        c = cells[sel]
        ok = (c[:, 0] >= 0) & (c[:, 0] < nx) & (c[:, 1] >= 0) & (c[:, 1] < ny) & (c[:, 2] >= 0) & (c[:, 2] < nz)
        c = c[ok]
        dst[c[:, 2], c[:, 1], c[:, 0]] = True

    steps, ve = walk(qs, qe)
    for cells, alive in steps:
        mark(free, cells, alive)
    mark(hit, ve, is_hit)
    mark(free, ve, ~is_hit)
    free &= ~hit
    return free, hit, len(qe), int(np.sum(~is_hit))


def update(prm, L, free, hit):
    """L after one view (a new array): the voxels of hit take l_hit, those of free l_miss, clamped; NaN starts from 0."""
    L = np.array(L, F)
    with np.errstate(all="ignore"):
        for sel, delta in ((hit, prm["l_hit"]), (free, prm["l_miss"])):
            base = np.where(np.isnan(L[sel]), F(0), L[sel]).astype(F)
            L[sel] = np.minimum(np.maximum(base + F(delta), F(prm["l_min"])), F(prm["l_max"]))
    return L


def empty(prm):
    return np.full((prm["nz"], prm["ny"], prm["nx"]), np.nan, F)


def integrate(prm, L, views):
    """(L after the views in order, stats [4] uint64) from L [nz, ny, nx]; views = [(R, t, points)]."""
    stats = np.zeros(4, np.uint64)
    for R, t, pts in views:
        free, hit, used, cut = view_sets(prm, R, t, pts)
        L = update(prm, L, free, hit)
        stats += np.array([used, cut, free.sum(), hit.sum()], np.uint64)
    return L, stats


def project(prm, L, k_lo, k_hi):
    """[ny, nx] int8: 100 if any L >= l_occ over the layers k_lo..k_hi (clipped), else 0 if any L <= l_free, else -1."""
    k0, k1 = max(k_lo, 0), min(k_hi, prm["nz"] - 1)
    out = np.full((prm["ny"], prm["nx"]), -1, np.int8)
    if k0 > k1:
        return out
    band = L[k0:k1 + 1]
    with np.errstate(all="ignore"):
        out[np.any(band <= F(prm["l_free"]), axis=0)] = 0
        out[np.any(band >= F(prm["l_occ"]), axis=0)] = 100
    return out


def query(prm, L, pts):
    """[n] f32: L at the voxel of each world point, NaN outside the grid."""
    qf = quant_f(np.asarray(pts, F).reshape(-1, 3), prm["origin"], prm["resolution"])
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < Q_LIMIT, axis=1)
    v = np.where(ok[:, None], qf, 0).astype(np.int64) >> 8
    ok &= (v[:, 0] >= 0) & (v[:, 0] < prm["nx"]) & (v[:, 1] >= 0) & (v[:, 1] < prm["ny"]) & (v[:, 2] >= 0) & (v[:, 2] < prm["nz"])
    out = np.full(len(v), np.nan, F)
    out[ok] = L[v[ok, 2], v[ok, 1], v[ok, 0]]
    return out


def same_bits(a, b):
    """Log-odds compared as bits, NaN by isnan."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))
