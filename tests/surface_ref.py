"""The rules of lv_map_normals / lv_map_remove_outliers in numpy (include/limovelo_hip.h "Surface normals and outlier removal").

Neighbour sets by f32 calc_dist in the device's operation order and (d2, id) order — the statement tests/test_gpu_map_query.py
makes with np_knn, restated here; everything after in f64.  The candidates of a point come from a k-d tree with a margin and are
re-ranked by the f32 keys; a point whose margin cannot be proven falls back to brute force, so the sets are exact."""
import numpy as np
from scipy.spatial import cKDTree

NONE = -1


def calc_dist(q, m):
    """f32 (qx - mx)^2 + (qy - my)^2 + (qz - mz)^2, left to right; q [..., 3], m [..., 3] broadcast."""
    q = np.asarray(q, np.float32)
    m = np.asarray(m, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = q[..., 0] - m[..., 0], q[..., 1] - m[..., 1], q[..., 2] - m[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def _keys(d, ids, max_d2):
    ok = np.isfinite(d) & (d <= max_d2)
    return np.where(ok, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64), np.uint64(~np.uint64(0)))


def knn_self(xyz, k, max_dist, extra=8):
    """(idx [m, k] int64 (NONE = unfilled), d2 [m, k] f32, n [m]): lv_map_knn of every point against its own cloud."""
    xyz = np.asarray(xyz, np.float32)
    m = len(xyz)
    md = np.float32(max_dist)
    max_d2 = md * md
    kk = min(k + extra, m)
    tree = cKDTree(xyz.astype(np.float64))
    dd, ii = tree.query(xyz.astype(np.float64), k=kk)
    dd, ii = dd.reshape(m, kk), ii.reshape(m, kk)
    valid = ii < m
    cand = np.where(valid, ii, 0)
    d = calc_dist(xyz[:, None, :], xyz[cand])
    d = np.where(valid, d, np.float32(np.inf))
    key = np.sort(_keys(d, cand, max_d2), axis=1)[:, :min(k, kk)]
    real = key != np.uint64(~np.uint64(0))
    idx = np.full((m, k), NONE, np.int64)
    d2 = np.full((m, k), np.inf, np.float32)
    idx[:, :key.shape[1]] = np.where(real, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), NONE)
    d2[:, :key.shape[1]] = np.where(real, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
    # proof of the margin: every point outside the candidates is farther (f64) than the largest key kept, with room for the f32
    # rounding of calc_dist (relative 4 eps32), or beyond max_dist; otherwise brute force for that point
    if kk < m:
        nk = key.shape[1]
        full = real[:, nk - 1] if nk == k else np.zeros(m, bool)
        kth = np.minimum(np.where(full, d2[:, nk - 1].astype(np.float64), np.inf), np.float64(max_d2))
        unsure = ~(dd[:, -1] ** 2 > kth * (1 + 1e-5) + 1e-30)
        ar = np.arange(m)
        for i in np.nonzero(unsure)[0]:
            kb = np.sort(_keys(calc_dist(xyz[i], xyz), ar, max_d2))[:k]
            rb = kb != np.uint64(~np.uint64(0))
            idx[i] = NONE
            d2[i] = np.inf
            idx[i, :len(kb)] = np.where(rb, (kb & np.uint64(0xFFFFFFFF)).astype(np.int64), NONE)
            d2[i, :len(kb)] = np.where(rb, (kb >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
    return idx, d2, (idx != NONE).sum(axis=1).astype(np.int32)


def mean_dist64(d2, n):
    """f64 (sum_j sqrt(d2_j)) / (n - 1) in neighbour order, +inf when n = 1."""
    s = np.zeros(len(d2))
    for j in range(d2.shape[1]):
        s = s + np.where(j < n, np.sqrt(np.where(j < n, d2[:, j], 0).astype(np.float64)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 1, s / (n - 1), np.inf)


def orient0_sign(v):
    """+-1 per row: the component of largest magnitude positive, ties to the lower axis."""
    a = np.argmax(np.abs(v), axis=1)   # (argmax returns the first maximum)
    return np.where(v[np.arange(len(v)), a] < 0, -1.0, 1.0)


def normals(xyz, k=10, max_dist=2.0, min_neighbours=5, orient=0, viewpoint=(0.0, 0.0, 0.0)):
    """dict: normals [m, 3] f64 (unit, signed), curvature, mean_dist (f64), n_used, gap = (l1 - l0) / l2, sign_margin (relative
    distance of the deciding quantity from its tie), idx."""
    xyz = np.asarray(xyz, np.float32)
    m = len(xyz)
    idx, d2, n = knn_self(xyz, k, max_dist)
    p = xyz.astype(np.float64)
    o = np.where((idx != NONE)[:, :, None], p[np.where(idx != NONE, idx, 0)] - p[:, None, :], 0.0)
    s = np.zeros((m, 3))
    for j in range(k):
        s = s + o[:, j]
    nn = np.maximum(n, 1).astype(np.float64)
    mean = s / nn[:, None]
    C = np.zeros((m, 3, 3))
    for j in range(k):
        c = np.where((j < n)[:, None], o[:, j] - mean, 0.0)
        C = C + c[:, :, None] * c[:, None, :]
    C = C / nn[:, None, None]
    lam, vec = np.linalg.eigh(C)
    v = vec[:, :, 0].copy()
    tr = lam.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        curv = np.where(tr > 0, lam[:, 0] / tr, 0.0)
        gap = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    sg = orient0_sign(v)
    av = np.sort(np.abs(v), axis=1)
    margin = (av[:, 2] - av[:, 1]) / np.maximum(av[:, 2], 1e-300)
    if orient:
        tv = np.asarray(viewpoint, np.float64)[None, :] - p
        dot = (v[:, 0] * tv[:, 0] + v[:, 1] * tv[:, 1]) + v[:, 2] * tv[:, 2]
        sg = np.where(dot > 0, 1.0, np.where(dot < 0, -1.0, sg))
        margin = np.abs(dot) / np.maximum(np.linalg.norm(tv, axis=1), 1e-300)
    v = v * sg[:, None]
    few = n < min_neighbours
    v[few] = 0.0
    curv = np.where(few, np.nan, curv)
    return dict(normals=v, curvature=curv, mean_dist=mean_dist64(d2, n), n_used=n, gap=gap, sign_margin=margin, idx=idx, few=few)


def outliers_statistical(xyz, k=10, std_mul=2.0, max_dist=2.0):
    """(flags [m] bool, d [m] f64, (mu, sigma, threshold))."""
    idx, d2, n = knn_self(xyz, k + 1, max_dist)
    d = np.where(n == k + 1, mean_dist64(d2, n), np.inf)
    fin = np.isfinite(d)
    nf = int(fin.sum())
    mu = d[fin].sum() / nf if nf else 0.0
    sigma = float(np.sqrt(((d[fin] - mu) ** 2).sum() / (nf - 1))) if nf > 1 else 0.0
    thr = mu + float(np.float32(std_mul)) * sigma
    return d > thr, d, (mu, sigma, thr)


def radius_counts(xyz, radius):
    """[m]: the number of OTHER points with f32 d2 <= f32(radius)^2."""
    xyz = np.asarray(xyz, np.float32)
    r = np.float32(radius)
    r2 = r * r
    tree = cKDTree(xyz.astype(np.float64))
    pairs = tree.query_pairs(float(radius) * (1 + 1e-5) + 1e-12, output_type="ndarray")
    cnt = np.zeros(len(xyz), np.int64)
    if len(pairs):
        # calc_dist is symmetric in its arguments up to the sign of the differences, which the squares remove
        ok = calc_dist(xyz[pairs[:, 0]], xyz[pairs[:, 1]]) <= r2
        cnt += np.bincount(pairs[ok, 0], minlength=len(xyz))
        cnt += np.bincount(pairs[ok, 1], minlength=len(xyz))
    return cnt


def outliers_radius(xyz, radius=0.5, min_neighbours=5):
    return radius_counts(xyz, radius) < min_neighbours


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))
