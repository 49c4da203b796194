"""The distance field's rule (include/limovelo_hip.h "Distance field") in numpy: what tests/test_distance_host.py holds the host
build of lv_distance.hpp to and tests/test_gpu_occ_distance.py the kernels, voxel for voxel.  The obstacle mask from the log-odds
(the planar one through occupancy_ref.project), the separable transform in int64, then sign, truncation, metres, query, gradient
and stats.  Squared distances are integers, the metres f32 operations in the stated order: everything is compared by equality."""
import numpy as np

import occupancy_ref as ocr

F = np.float32
FAR = 2147483647
BIG = np.int64(1) << 40   # "no obstacle" inside the int64 transform
FIELDS = ("planar", "k_lo", "k_hi", "unknown_is_obstacle", "signed_field", "max_cells")


def dparams(**kw):
    """A plain dict of lv_distance_params (all zero, overridden by kw)."""
    p = dict.fromkeys(FIELDS, 0)
    p.update(kw)
    return p


def obstacle_mask(prm, L, dp):
    """bool [nz, ny, nx], or [1, ny, nx] of a planar field: which voxels are obstacles."""
    L = np.asarray(L, F)
    with np.errstate(all="ignore"):
        if dp["planar"]:
            proj = ocr.project(prm, L, dp["k_lo"], dp["k_hi"])
            m = proj == 100
            if dp["unknown_is_obstacle"]:
                m |= proj == -1
            return m[None]
        m = L >= F(prm["l_occ"])
        if dp["unknown_is_obstacle"]:
            m |= np.isnan(L)
    return m


def _pass(f, axis):
    """min over j' of f[j'] + (j - j')^2 along axis (int64)."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    idx = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (f.ndim - 1))
    out = np.empty_like(f)
    for j in range(n):
        out[j] = np.min(f + (idx - j) ** 2, axis=0)
    return np.moveaxis(out, 0, axis)


def edt2(mask):
    """int64 squared distance of every voxel to the nearest True voxel of mask (>= BIG where there is none)."""
    f = np.where(mask, np.int64(0), BIG)
    for axis in range(mask.ndim):
        f = _pass(f, axis)
    return f


def field(mask, dp):
    """s2 int32 (the shape of mask) from the obstacle mask: sign, FAR and truncation as stored."""
    out = edt2(mask)
    s = np.where(out >= BIG, np.int64(FAR), out)
    if dp["signed_field"]:
        inn = edt2(~mask)
        s = np.where(mask, np.where(inn >= BIG, np.int64(-FAR), -inn), s)
    else:
        s = np.where(mask, np.int64(0), s)
    if dp["max_cells"]:
        lim = int(dp["max_cells"]) ** 2
        finite = np.abs(s) != FAR
        s = np.where(finite & (s > lim), FAR, np.where(finite & (s < -lim), -FAR, s))
    return s.astype(np.int32)


def build(prm, L, dp):
    """(s2 int32 [nz, ny, nx] or [ny, nx] when planar, stats [4] uint64) of a grid's log-odds."""
    mask = obstacle_mask(prm, L, dp)
    s2 = field(mask, dp)
    if dp["planar"]:
        s2 = s2[0]
    return s2, stats(s2, mask.sum())


def stats(s2, n_obstacles):
    s = np.asarray(s2, np.int64)
    finite = np.abs(s) != FAR
    pos, neg = s[finite & (s > 0)], -s[finite & (s < 0)]
    return np.array([n_obstacles, finite.sum(), pos.max() if len(pos) else 0, neg.max() if len(neg) else 0], np.uint64)


def metres(s2, resolution):
    """f32: resolution * sqrtf(|s2|) with the sign of s2; 0 -> +0, +-FAR -> +-inf."""
    s = np.asarray(s2, np.int64)
    with np.errstate(all="ignore"):
        m = F(resolution) * np.sqrt(np.abs(s).astype(F))
        m = np.where(s < 0, -m, m).astype(F)
    m[s == FAR] = np.inf
    m[s == -FAR] = -np.inf
    m[s == 0] = F(0.0)
    return m


def query(prm, dp, s2, pts):
    """(dist [n] f32, grad [n, 3] f32) of world points against a finished field s2."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    s2 = np.asarray(s2, np.int32)
    s3 = s2[None] if dp["planar"] else s2
    dims = np.array(s3.shape[::-1])   # nx, ny, nz
    res = F(prm["resolution"])
    m = metres(s3, res)
    qf = ocr.quant_f(pts, prm["origin"], prm["resolution"])
    if dp["planar"]:
        qf[:, 2] = 0
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < ocr.Q_LIMIT, axis=1)
    v = np.where(ok[:, None], qf, 0).astype(np.int64) >> 8
    ok &= np.all((v >= 0) & (v < dims), axis=1)
    n = len(pts)
    dist = np.full(n, np.nan, F)
    grad = np.zeros((n, 3), F)
    for p in np.nonzero(ok)[0]:
        i, j, k = v[p]
        m0 = m[k, j, i]
        dist[p] = m0
        if not np.isfinite(m0):
            continue
        for a in range(3):
            lo, hi = v[p].copy(), v[p].copy()
            lo[a] -= 1
            hi[a] += 1
            mm = m[lo[2], lo[1], lo[0]] if lo[a] >= 0 else F(np.nan)
            mp = m[hi[2], hi[1], hi[0]] if hi[a] < dims[a] else F(np.nan)
            um, up = np.isfinite(mm), np.isfinite(mp)
            with np.errstate(all="ignore"):
                if um and up:
                    grad[p, a] = F(mp - mm) / F(res + res)
                elif up:
                    grad[p, a] = F(mp - m0) / res
                elif um:
                    grad[p, a] = F(m0 - mm) / res
    return dist, grad


def random_logodds(rng, shape, p_occ, p_unknown=1.0 / 3.0, prm=None):
    """A grid of log-odds [nz, ny, nx] for tests: p_occ of the voxels occupied (values from l_occ itself up to l_max), p_unknown
    NaN, the rest free or strictly between l_free and l_occ (which makes them neither)."""
    prm = prm or ocr.params()
    u = rng.uniform(size=shape)
    L = rng.uniform(prm["l_min"], prm["l_free"], shape).astype(F)
    between = rng.uniform(size=shape) < 0.3
    L[between] = rng.uniform(0.75 * prm["l_free"], 0.75 * prm["l_occ"], between.sum()).astype(F)
    L[u < p_occ + p_unknown] = np.nan
    occ = u < p_occ
    L[occ] = np.where(rng.uniform(size=occ.sum()) < 0.3, F(prm["l_occ"]), rng.uniform(prm["l_occ"], prm["l_max"], occ.sum())).astype(F)
    return L


def probe_points(prm, rng, n=60, n_centres=200):
    """World points for query tests: in every corner voxel and on every face of the grid (inside and just outside), non-finite
    ones (a NaN z among them: a planar field does not look at it), far ones, random ones round the grid and the centres of random
    voxels."""
    lo = np.array(prm["origin"], np.float64)
    dims = np.array([prm["nx"], prm["ny"], prm["nz"]])
    res = prm["resolution"]
    hi = lo + dims * res
    corners = [np.where(c, hi - 0.25 * res, lo + 0.25 * res) for c in np.ndindex(2, 2, 2)]
    faces = []
    for a in range(3):
        for side in (lo[a] + 0.25 * res, hi[a] - 0.25 * res, lo[a] - 0.25 * res, hi[a] + 0.25 * res):
            q = rng.uniform(lo, hi)
            q[a] = side
            faces.append(q)
    odd = [[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]], [lo[0] + 0.5 * res, lo[1] + 0.5 * res, np.nan], [1e30, 0, 0], lo, hi]
    centres = lo + (rng.integers(0, dims, (n_centres, 3)) + 0.5) * res
    return np.concatenate([corners, faces, odd, rng.uniform(lo - res, hi + res, (n, 3)), centres]).astype(F)


def brute(mask):
    """edt2 by the O(N^2) minimum over all voxel pairs (tiny grids only)."""
    idx = np.stack(np.nonzero(np.ones(mask.shape, bool)), axis=1).astype(np.int64)
    obs = idx[mask.reshape(-1)]
    if len(obs) == 0:
        return np.full(mask.shape, BIG, np.int64)
    d = ((idx[:, None, :] - obs[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return d.reshape(mask.shape)


def same_bits(a, b):
    """f32 compared as bits, NaN by isnan."""
    return ocr.same_bits(a, b)
