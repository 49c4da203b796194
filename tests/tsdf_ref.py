"""The TSDF's rule and its mesh (include/limovelo_hip.h "TSDF and mesh") in numpy and Python integers, written from the header's
text: what tests/test_tsdf_host.py holds the host build of lv_tsdf.hpp to and tests/test_gpu_tsdf.py the kernels, voxel for
voxel, vertex for vertex, index for index.  The returns and the walk are those of "Occupancy grid" and come from
tests/occupancy_ref.py; everything after them is int64 (every value stays below 2^55) with exact square roots from math.isqrt."""
import math

import numpy as np

import occupancy_ref as ocr

F = np.float32
I = np.int64
Q = 256
FIELDS = ("origin", "resolution", "nx", "ny", "nz", "min_range", "max_range", "trunc_cells", "max_weight", "carve")


def params(**kw):
    """A plain dict of the parameters (the defaults of lv_default_tsdf_params, overridden by kw)."""
    p = dict(origin=(-51.2, -51.2, -3.2), resolution=0.2, nx=512, ny=512, nz=64, min_range=1.0, max_range=80.0, trunc_cells=3,
             max_weight=10000, carve=0)
    p.update(kw)
    return p


def params_of(cp):
    """The dict of a capi.TsdfParams."""
    return {f: (tuple(float(v) for v in cp.origin) if f == "origin" else getattr(cp, f)) for f in FIELDS}


def empty(prm):
    shape = (prm["nz"], prm["ny"], prm["nx"])
    return np.zeros(shape, np.int32), np.zeros(shape, np.int32)


def _trunc_div(a, b):
    """C's a / b for int64 arrays, b > 0."""
    return np.sign(a) * (np.abs(a) // b)


def call_sums(prm, views):
    """(dS, dW [nz, ny, nx] int64, rays used, rays cut) of one call: the contributions of every ray of every view."""
    nx, ny, nz = prm["nx"], prm["ny"], prm["nz"]
    T = prm["trunc_cells"] * Q
    carve = prm["carve"] != 0
    dS = np.zeros((nz, ny, nx), I)
    dW = np.zeros((nz, ny, nx), I)
    used = cut = 0
    for R, t, pts in views:
        pts = np.asarray(pts, F).reshape(-1, 3)
        qs = ocr.view_origin(prm, t)
        if qs is None or len(pts) == 0:
            continue
        qe, is_hit = ocr.returns(prm, R, t, pts)
        if not carve:
            qe = qe[is_hit]
            is_hit = is_hit[is_hit]
        d = qe - qs
        ln = np.array([math.isqrt(int(v)) for v in np.sum(d * d, axis=1)], I)
        keep = ln > 0
        qe, is_hit, d, ln = qe[keep], is_hit[keep], d[keep], ln[keep]
        if len(qe) == 0:
            continue
        used += len(qe)
        cut += int(np.sum(~is_hit))
        ext = _trunc_div(d * T, ln[:, None])
        ext[~is_hit] = 0
        qb = qe + ext
        from_sensor = ~is_hit | carve | (ln <= T)
        start = np.where(from_sensor[:, None], qs[None, :], qe - ext)
        steps, ve = ocr.walk(start, qb)
        visits = [(cells, alive) for cells, alive in steps] + [(ve, np.ones(len(ve), bool))]
        for cells, alive in visits:
            c = Q * cells + 128
            s = np.sum((qe - c) * d, axis=1) // ln     # (numpy's // is floor division)
            s = np.where(is_hit, np.minimum(s, T), T)
            ok = alive & (s >= -T)
            ok &= (cells[:, 0] >= 0) & (cells[:, 0] < nx) & (cells[:, 1] >= 0) & (cells[:, 1] < ny) & (cells[:, 2] >= 0) & (cells[:, 2] < nz)
            v = cells[ok]
            np.add.at(dS, (v[:, 2], v[:, 1], v[:, 0]), s[ok])
            np.add.at(dW, (v[:, 2], v[:, 1], v[:, 0]), 1)
    return dS, dW, used, cut


def integrate(prm, S, W, views):
    """(S, W after one call, stats [4] uint64) from S, W [nz, ny, nx] int32; views = [(R, t, points)]."""
    dS, dW, used, cut = call_sums(prm, views)
    mw = int(prm["max_weight"])
    Wn = W.astype(I) + dW
    Sn = S.astype(I) + dS
    over = Wn > mw
    S2 = np.where(over, (Sn * mw) // np.maximum(Wn, 1), Sn)
    W2 = np.where(over, mw, Wn)
    touched = dW > 0
    S2 = np.where(touched, S2, S)
    W2 = np.where(touched, W2, W)
    assert np.all(np.abs(S2) <= prm["trunc_cells"] * Q * W2)
    return S2.astype(np.int32), W2.astype(np.int32), np.array([used, cut, dW.sum(), touched.sum()], np.uint64)


def metres(prm, S, W):
    with np.errstate(all="ignore"):
        return (F(prm["resolution"]) * ((S.astype(F) / W.astype(F)) / F(256.0))).astype(F)


def query(prm, S, W, pts):
    """(metres [n] f32, weight [n] int32) at the voxel of each world point; NaN and 0 outside the grid."""
    qf = ocr.quant_f(np.asarray(pts, F).reshape(-1, 3), prm["origin"], prm["resolution"])
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < ocr.Q_LIMIT, axis=1)
    v = np.where(ok[:, None], qf, 0).astype(I) >> 8
    ok &= (v[:, 0] >= 0) & (v[:, 0] < prm["nx"]) & (v[:, 1] >= 0) & (v[:, 1] < prm["ny"]) & (v[:, 2] >= 0) & (v[:, 2] < prm["nz"])
    m = np.full(len(v), np.nan, F)
    w = np.zeros(len(v), np.int32)
    m[ok] = metres(prm, S, W)[v[ok, 2], v[ok, 1], v[ok, 0]]
    w[ok] = W[v[ok, 2], v[ok, 1], v[ok, 0]]
    return m, w


def same_metres(a, b):
    return ocr.same_bits(a, b)


def mesh(prm, S, W, min_weight=1):
    """dict(sub [V, 3] int32, xyz [V, 3] f32, tri [F, 3] uint32, counts [4] uint64) of the volume: naive surface nets."""
    nx, ny, nz = prm["nx"], prm["ny"], prm["nz"]
    S = S.astype(I)
    W = W.astype(I)
    known = W >= min_weight
    inside = S < 0
    cx, cy, cz = max(nx - 1, 0), max(ny - 1, 0), max(nz - 1, 0)

    def corner(arr, dx, dy, dz):   # the cells' corner (dx, dy, dz), an array over the cells [cz, cy, cx]
        return arr[dz:dz + cz, dy:dy + cy, dx:dx + cx]

    corners = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    all_known = np.ones((cz, cy, cx), bool)
    n_inside = np.zeros((cz, cy, cx), I)
    for o in corners:
        all_known &= corner(known, *o)
        n_inside += corner(inside, *o)
    active = all_known & (n_inside > 0) & (n_inside < 8)
    # the vertices
    kk, jj, ii = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
    base = [Q * ii + 128, Q * jj + 128, Q * kk + 128]
    total = [np.zeros((cz, cy, cx), I) for _ in range(3)]
    count = np.zeros((cz, cy, cx), I)
    for a in range(3):
        for A in corners:
            if A[a] == 1:
                continue
            B = tuple(A[b] + (1 if b == a else 0) for b in range(3))
            SA, WA, SB, WB = corner(S, *A), corner(W, *A), corner(S, *B), corner(W, *B)
            cross = active & (corner(inside, *A) != corner(inside, *B))
            num = SA * WB
            den = SA * WB - SB * WA
            neg = den < 0
            num = np.where(neg, -num, num)
            den = np.where(neg, -den, den)
            t = np.where(cross, (Q * num) // np.where(cross, den, 1), 0)
            assert np.all((t >= 0) & (t <= Q))
            for b in range(3):
                total[b] += np.where(cross, base[b] + Q * A[b] + (t if b == a else 0), 0)
            count += cross
    assert np.all(count[active] >= 1) and np.all(count <= 12)
    sub = np.stack([(total[b][active] // count[active]) for b in range(3)], axis=1).astype(np.int32)   # (C order = linear order)
    with np.errstate(all="ignore"):
        xyz = np.stack([F(prm["origin"][b]) + F(prm["resolution"]) * (sub[:, b].astype(F) / F(256.0)) for b in range(3)], axis=1).astype(F)
    vid = np.full((cz, cy, cx), -1, I)
    vid[active] = np.arange(int(active.sum()))
    # the faces
    quads = []
    refused = 0
    for a in range(3):
        e = [0, 0, 0]
        e[a] = 1
        n = [nx, ny, nz]
        m = [n[0] - e[0], n[1] - e[1], n[2] - e[2]]   # the voxels p with p + e_a in the grid
        if min(m) <= 0:
            continue
        pA = (slice(0, m[2]), slice(0, m[1]), slice(0, m[0]))
        pB = (slice(e[2], e[2] + m[2]), slice(e[1], e[1] + m[1]), slice(e[0], e[0] + m[0]))
        edge = known[pA] & known[pB] & (inside[pA] != inside[pB])
        b, c = (a + 1) % 3, (a + 2) % 3
        for k, j, i in zip(*np.nonzero(edge)):
            p = [int(i), int(j), int(k)]
            ids = []
            for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
                v = list(p)
                v[b] += ob
                v[c] += oc
                if min(v) < 0 or v[0] > nx - 2 or v[1] > ny - 2 or v[2] > nz - 2 or not active[v[2], v[1], v[0]]:
                    ids = None
                    break
                ids.append(int(vid[v[2], v[1], v[0]]))
            if ids is None:
                refused += 1
                continue
            if not inside[p[2], p[1], p[0]]:
                ids = [ids[0], ids[3], ids[2], ids[1]]
            quads.append((3 * ((p[2] * ny + p[1]) * nx + p[0]) + a, ids))
    quads.sort(key=lambda q: q[0])
    tri = np.array([t for _, q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint32).reshape(-1, 3)
    counts = np.array([len(sub), len(tri), int(active.sum()), refused], np.uint64)
    return dict(sub=sub, xyz=xyz, tri=tri, counts=counts)
