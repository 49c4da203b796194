"""The rule of ray casting on the TSDF surface (include/limovelo_hip.h "Surface ray casting") in numpy and Python integers, written
from the header's text: what tests/test_tsdf_ray_host.py holds the host build of lv_tsdf_ray.hpp to and tests/test_gpu_tsdf_ray.py
the kernels, field for field, normal bit for normal bit, colour byte for colour byte.  The ends and the walk are
tests/occ_ray_ref.py's (ends, walk) on the TSDF's parameters, the volumes tests/tsdf_ref.py's, the voxel colour
tests/colour_ref.py's.  Volumes are [nz, ny, nx] int32, layers [nz, ny, nx, 4] uint32."""
import math

import numpy as np

import colour_ref as cr
import occ_ray_ref as orr
import occupancy_ref as ocr

F = np.float32
I = np.int64
IGNORED, CLEAR, HIT, BLOCKED = 0, 1, 2, 3
UNKNOWN, OUT, IN = 0, 1, 2
RESULT_FIELDS = ("status", "cell", "steps", "axis", "depth", "t", "n_known", "n_unknown")
RESULT_DTYPE = np.dtype([(f, np.int32) for f in RESULT_FIELDS])


def states(S, W, min_weight=1):
    """[nz, ny, nx] uint8: KNOWN iff W >= min_weight; a KNOWN cell is IN iff S < 0, otherwise OUT."""
    return np.where(np.asarray(W) >= int(min_weight), np.where(np.asarray(S) < 0, IN, OUT), UNKNOWN).astype(np.uint8)


def _inside(prm, c):
    return (c[:, 0] >= 0) & (c[:, 0] < prm["nx"]) & (c[:, 1] >= 0) & (c[:, 1] < prm["ny"]) & (c[:, 2] >= 0) & (c[:, 2] < prm["nz"])


def _linear(prm, c):
    return (c[:, 2] * prm["ny"] + c[:, 1]) * prm["nx"] + c[:, 0]


def _isqrt(v):
    return np.array([math.isqrt(int(x)) for x in v], I)


def normals_at(prm, S, W, cells, min_weight=1):
    """f32 [m, 3]: the normal at the KNOWN cells [m, 3] (i, j, k): the gradient of phi = S / W over the KNOWN neighbours, normalised;
    zeros where an axis has no KNOWN neighbour or the gradient vanishes.  Every operation f32, in the header's order."""
    cells = np.asarray(cells, I).reshape(-1, 3)
    m = len(cells)
    dims = np.array([prm["nx"], prm["ny"], prm["nz"]], I)
    with np.errstate(all="ignore"):
        phi = np.asarray(S).astype(F) / np.asarray(W).astype(F)
    known = np.asarray(W) >= int(min_weight)

    def at(arr, c):
        return arr[c[:, 2], c[:, 1], c[:, 0]]

    phi_b = at(phi, cells)
    g = np.zeros((m, 3), F)
    valid = np.ones(m, bool)
    for a in range(3):
        e = np.zeros(3, I)
        e[a] = 1
        lo_c, hi_c = cells - e, cells + e
        lo_in, hi_in = lo_c[:, a] >= 0, hi_c[:, a] < dims[a]
        lo_c, hi_c = np.where(lo_in[:, None], lo_c, cells), np.where(hi_in[:, None], hi_c, cells)
        lo, hi = lo_in & at(known, lo_c), hi_in & at(known, hi_c)
        p_lo, p_hi = at(phi, lo_c), at(phi, hi_c)
        with np.errstate(all="ignore"):
            both = (p_hi - p_lo).astype(F)
            fwd = (F(2.0) * (p_hi - phi_b).astype(F)).astype(F)
            bwd = (F(2.0) * (phi_b - p_lo).astype(F)).astype(F)
        g[:, a] = np.where(lo & hi, both, np.where(hi, fwd, bwd))
        valid &= lo | hi
    with np.errstate(all="ignore"):
        norm = np.sqrt(((g[:, 0] * g[:, 0]).astype(F) + (g[:, 1] * g[:, 1]).astype(F)).astype(F) + (g[:, 2] * g[:, 2]).astype(F)).astype(F)
        valid &= norm > 0
        n = (g / norm[:, None]).astype(F)
    return np.where(valid[:, None], n, F(0)).astype(F)


def cast_q(prm, S, W, qs, qe, min_weight=1, layer=None):
    """(results [m] RESULT_DTYPE, normals [m, 3] f32, rgba [m, 4] uint8) of the rays qs -> qe in sub-units."""
    qe = np.asarray(qe, I).reshape(-1, 3)
    qs = np.broadcast_to(np.asarray(qs, I), qe.shape)
    m = len(qe)
    st = states(S, W, min_weight)
    S64, W64 = np.asarray(S).astype(I), np.asarray(W).astype(I)
    out = np.zeros(m, RESULT_DTYPE)
    done = np.zeros(m, bool)
    nk = np.zeros(m, I)
    nu = np.zeros(m, I)
    total = np.zeros(m, I)
    prev_out = np.zeros(m, bool)          # c_(s - 1) is inside the grid and OUT
    prev_cells = np.zeros((m, 3), I)
    A = np.zeros((m, 3), I)
    B = np.zeros((m, 3), I)
    num_s = np.zeros(m, I)
    den_s = np.ones(m, I)
    for s, (has, cells, axis, num, den) in enumerate(orr.walk(qs, qe)):
        total[has] = s
        idx = np.nonzero(has & ~done & _inside(prm, cells))[0]
        c = cells[idx]
        sc = st[c[:, 2], c[:, 1], c[:, 0]]
        stop = sc == IN
        h = idx[stop]
        out["status"][h] = np.where(prev_out[h], HIT, BLOCKED)
        out["cell"][h], out["steps"][h], out["axis"][h] = _linear(prm, c[stop]), s, axis[h]
        out["n_known"][h], out["n_unknown"][h] = nk[h], nu[h]
        A[h], B[h], num_s[h], den_s[h] = prev_cells[h], cells[h], num[h], den[h]
        done[h] = True
        p = idx[~stop]
        nk[p] += sc[~stop] == OUT
        nu[p] += sc[~stop] == UNKNOWN
        prev_out = np.zeros(m, bool)
        prev_out[p] = sc[~stop] == OUT
        prev_cells = cells
    clear = np.nonzero(~done)[0]
    ve = qe[clear] >> 8
    out["status"][clear] = CLEAR
    out["cell"][clear] = np.where(_inside(prm, ve), _linear(prm, ve), -1)
    out["steps"][clear], out["axis"][clear] = total[clear], -1
    out["n_known"][clear], out["n_unknown"][clear] = nk[clear], nu[clear]
    # the depth
    d = qe - qs
    l2 = np.sum(d * d, axis=1)
    ln = _isqrt(l2)
    depth = ln.copy()
    t = np.full(m, -1, I)
    blocked = out["status"] == BLOCKED
    depth[blocked] = np.where(out["steps"][blocked] == 0, 0, (num_s[blocked] * ln[blocked]) // den_s[blocked])
    hit = np.nonzero(out["status"] == HIT)[0]
    if len(hit):
        a, b = A[hit], B[hit]
        assert np.all(np.abs(b - a).sum(axis=1) == 1)
        SA, WA, SB, WB = (arr[c[:, 2], c[:, 1], c[:, 0]] for c in (a, b) for arr in (S64, W64))
        num = SA * WB
        den = num - SB * WA
        assert np.all(den > 0) and np.all(num >= 0)
        th = (256 * num) // den
        assert np.all((th >= 0) & (th <= 256))
        ax = out["axis"][hit].astype(I)
        u = np.sum((256 * a + 128 - qs[hit]) * d[hit], axis=1) + np.abs(d[hit, ax]) * th
        u = np.clip(u, 0, l2[hit])
        assert np.all(ln[hit] >= 1)
        depth[hit] = u // ln[hit]
        t[hit] = th
    out["depth"], out["t"] = depth, t
    normals = np.zeros((m, 3), F)
    rgba = np.zeros((m, 4), np.uint8)
    if len(hit):
        normals[hit] = normals_at(prm, S, W, B[hit], min_weight)
        if layer is not None:
            eb = np.asarray(layer)[B[hit, 2], B[hit, 1], B[hit, 0]]
            ea = np.asarray(layer)[A[hit, 2], A[hit, 1], A[hit, 0]]
            rgba[hit] = np.where((eb[:, 3] > 0)[:, None], cr.voxel_colour(eb), cr.voxel_colour(ea))
    return out, normals, rgba


def _ignored(n):
    out = np.zeros(n, RESULT_DTYPE)
    out["cell"] = -1
    return out, np.zeros((n, 3), F), np.zeros((n, 4), np.uint8)


def raycast(prm, S, W, frm, to, min_weight=1, layer=None):
    """lv_surf_raycast: (results [n], normals [n, 3] f32, rgba [n, 4] uint8)."""
    ok, qs, qe = orr.ends(prm, frm, to)
    out, normals, rgba = _ignored(len(ok))
    if ok.any():
        out[ok], normals[ok], rgba[ok] = cast_q(prm, S, W, qs[ok], qe[ok], min_weight, layer)
    return out, normals, rgba


def metres(prm, res):
    """f32 [n]: resolution * ((float)depth / 256.0f) for HIT and BLOCKED rays, inf for CLEAR ones, NaN for IGNORED ones."""
    m = (F(prm["resolution"]) * (res["depth"].astype(F) / F(256.0))).astype(F)
    m[res["status"] == CLEAR] = np.inf
    m[res["status"] == IGNORED] = np.nan
    return m


def used_returns(prm, R, t, pts):
    """(used [n] bool, qe [used.sum(), 3]) of one view's returns, by occupancy_ref.returns taken one return at a time."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    qe, _ = ocr.returns(prm, R, t, pts)
    used = np.array([len(ocr.returns(prm, R, t, p[None, :])[0]) == 1 for p in pts], bool).reshape(-1)
    assert used.sum() == len(qe)
    return used, qe


def raycast_views(prm, S, W, views, min_weight=1, layer=None):
    """lv_surf_raycast_views over views = [(R, t, pattern end points)]: (results, normals, rgba over every return of every view in
    order, stats [4] uint64: rays used, HIT, BLOCKED, CLEAR)."""
    parts = []
    for R, t, pts in views:
        pts = np.asarray(pts, F).reshape(-1, 3)
        out, normals, rgba = _ignored(len(pts))
        qs = ocr.view_origin(prm, t)
        if qs is not None and len(pts):
            used, qe = used_returns(prm, R, t, pts)
            if used.any():
                out[used], normals[used], rgba[used] = cast_q(prm, S, W, qs, qe, min_weight, layer)
        parts.append((out, normals, rgba))
    out, normals, rgba = (np.concatenate([p[i] for p in parts]) for i in range(3))
    stats = np.array([np.sum(out["status"] != IGNORED)] + [np.sum(out["status"] == k) for k in (HIT, BLOCKED, CLEAR)], np.uint64)
    return out, normals, rgba, stats
