"""numpy (f64) statement of lv_map_remove_dynamic's rule (include/limovelo_hip.h "Dynamic-point removal") for the GPU tests.

The device computes atan2f / sqrtf in f32, which numpy does not pin, so a point's count is given as an interval [lo, hi]: for
every view, each alternative the f32 arithmetic could take is tried — a pixel coordinate within 1e-3 px of a bin edge (either
neighbouring bin, or outside the rows), a range within 1e-4 m of min_range / max_range (judged or not), r_img - r within 1e-4 m of
the threshold (seen through or not).  A point is AMBIGUOUS when its alternatives change the count (lo != hi); every other point
has exactly one admissible count.  Scan returns are kept off bin edges by the tests (edge_safe), so the images are exact."""
import math

import numpy as np

PX_EPS = 1e-3
M_EPS = 1e-4


def geometry(p):
    """(inv_col, v_min, inv_row) in f64 from an lv_visibility_params."""
    rad = math.pi / 180.0
    return p.width / (2.0 * math.pi), p.v_min_deg * rad, p.height / ((p.v_max_deg - p.v_min_deg) * rad)


def _coords(xyz, p):
    x, y, z = (xyz[:, i].astype(np.float64) for i in range(3))
    inv_col, v_min, inv_row = geometry(p)
    xy2 = x * x + y * y
    with np.errstate(invalid="ignore"):
        u = (np.arctan2(y, x) + math.pi) * inv_col
        v = (np.arctan2(z, np.sqrt(xy2)) - v_min) * inv_row
    return u, v, np.sqrt(xy2 + z * z)


def edge_safe(xyz, p):
    """The returns whose pixel and range are not within the tolerances of an edge (non-finite ones are kept: they are ignored
    on both sides)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    u, v, r = _coords(xyz, p)
    fin = np.all(np.isfinite(xyz), axis=1)
    with np.errstate(invalid="ignore"):
        fu, fv = u - np.floor(u), v - np.floor(v)
        ok = (np.minimum(fu, 1 - fu) > PX_EPS) & (np.minimum(fv, 1 - fv) > PX_EPS) & (np.abs(r - p.min_range) > M_EPS)
    return xyz[~fin | ok]


def image(xyz, p):
    """The window-min range image [height, width] of one view's returns (+inf: no evidence)."""
    W, H, w = p.width, p.height, p.window
    img = np.full(H * W, np.inf)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz):
        u, v, r = _coords(xyz, p)
        with np.errstate(invalid="ignore"):
            ok = np.all(np.isfinite(xyz), axis=1) & (r > p.min_range) & (v >= 0) & (v <= H)
        row = np.minimum(np.floor(v[ok]).astype(np.int64), H - 1)
        col = np.floor(u[ok]).astype(np.int64)
        col = np.where(col >= W, col - W, np.maximum(col, 0))
        np.minimum.at(img, row * W + col, r[ok])
    img = img.reshape(H, W)
    out = img.copy()
    for d in range(1, w + 1):
        out = np.minimum(out, np.minimum(np.roll(img, d, axis=1), np.roll(img, -d, axis=1)))
    img, out = out, out.copy()
    for d in range(1, w + 1):
        out[d:] = np.minimum(out[d:], img[:-d])
        out[:-d] = np.minimum(out[:-d], img[d:])
    return out


def hits(map_xyz, views, p):
    """(lo, hi, judged) per map point: the interval of its count and whether any view judged it (range and row inside).
    views: [(R [3, 3], t [3], returns [n, 3])]."""
    W, H = p.width, p.height
    pts = np.asarray(map_xyz, np.float32).astype(np.float64)
    n = len(pts)
    lo = np.zeros(n, np.int64)
    hi = np.zeros(n, np.int64)
    judged = np.zeros(n, bool)
    for R, t, ret in views:
        img = image(edge_safe(ret, p), p)
        ps = (pts - np.asarray(t, np.float32).astype(np.float64)) @ np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)
        u, v, r = _coords(ps, p)
        fu, fv = np.floor(u), np.floor(v)
        rows = [fv, np.where(v - fv < PX_EPS, fv - 1, np.where(fv + 1 - v < PX_EPS, fv + 1, fv))]
        cols = [fu, np.where(u - fu < PX_EPS, fu - 1, np.where(fu + 1 - u < PX_EPS, fu + 1, fu))]
        in_lo = (r >= p.min_range + M_EPS) & (r <= p.max_range - M_EPS)          # judged for sure
        in_hi = (r >= p.min_range - M_EPS) & (r <= p.max_range + M_EPS)          # judged possibly
        thr = np.maximum(p.margin_abs, p.margin_rel * r)
        omin = np.full(n, 1, np.int64)
        omax = np.zeros(n, np.int64)
        for rr in rows:
            for cc in cols:
                ok_row = (rr >= 0) & (rr <= H - 1)
                ri = np.clip(rr, 0, H - 1).astype(np.int64)
                ci = (cc.astype(np.int64) % W)
                ri_img = img[ri, ci]
                with np.errstate(invalid="ignore"):
                    diff = ri_img - r - thr
                fin = np.isfinite(ri_img)
                jmin = (fin & (diff > M_EPS)).astype(np.int64)
                jmax = (fin & (diff > -M_EPS)).astype(np.int64)
                cmin = np.where(ok_row & in_lo, jmin, 0)
                cmax = np.where(ok_row & in_hi, jmax, 0)
                omin = np.minimum(omin, cmin)
                omax = np.maximum(omax, cmax)
                judged |= ok_row & in_lo
        lo += omin
        hi += omax
    return lo, hi, judged
