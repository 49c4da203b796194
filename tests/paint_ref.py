"""numpy (f64) statement of lv_map_paint's rule (include/limovelo_hip.h "Map painting") for the GPU tests.

The device projects in f32, which numpy does not pin, so every per-view decision is given as an interval: a point is SURELY seen
by a view when every outcome the f32 arithmetic could take sees it, POSSIBLY seen when one could.  A decision is ambiguous when
  - u or v lies within 1e-3 px of an image border or of an occlusion-cell edge,
  - z lies within 1e-4 m of min_depth / max_depth,
  - sqrt(x^2 + y^2) lies within 1e-6 of max_norm_radius,
  - z - zbuf lies within 1e-4 m of the threshold.
The occlusion buffer is computed twice: from the unambiguous points alone (an upper bound of the device's cells) and with every
ambiguous point in every cell it could fall in (a lower bound).  A point's count is DECIDED when every view's decision is."""
import numpy as np

PX_EPS = 1e-3
M_EPS = 1e-4
NR_EPS = 1e-6


def texels(img, fmt):
    """[H, W, 3] f64 r, g, b of an image of format LV_IMAGE_* (0 rgb8, 1 bgr8, 2 mono8)."""
    a = np.asarray(img).astype(np.float64)
    if fmt == 2:
        return np.repeat(a[:, :, None], 3, axis=2)
    return a[:, :, ::-1] if fmt == 1 else a


def project(pts, f):
    """(z, rho, u, v) in f64 of map points pts [n, 3] (f32 values) in view f: depth, undistorted norm radius, pixel coordinates."""
    R = np.asarray(f["R"], np.float32).astype(np.float64).reshape(3, 3)
    t = np.asarray(f["t"], np.float32).astype(np.float64)
    pc = (np.asarray(pts, np.float32).astype(np.float64) - t) @ R
    X, Y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    k1, k2, p1, p2, k3 = np.asarray(f.get("dist", np.zeros(5)), np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x, y = X / z, Y / z
        r2 = x * x + y * y
        c = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        xd = x * c + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * c + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        u = np.float64(np.float32(f["fx"])) * xd + np.float64(np.float32(f["cx"]))
        v = np.float64(np.float32(f["fy"])) * yd + np.float64(np.float32(f["cy"]))
    return z, np.sqrt(r2), u, v


def _window_min(cells, w):
    out = cells.copy()
    src = cells
    for d in range(1, w + 1):
        out[:, d:] = np.minimum(out[:, d:], src[:, :-d])
        out[:, :-d] = np.minimum(out[:, :-d], src[:, d:])
    src = out.copy()
    for d in range(1, w + 1):
        out[d:] = np.minimum(out[d:], src[:-d])
        out[:-d] = np.minimum(out[:-d], src[d:])
    return out


def bilinear(tex, u, v):
    """The sample [n, 3] of texels tex [H, W, 3] at (u, v) inside the image, taps clamped."""
    H, W = tex.shape[:2]
    x0 = np.clip(np.floor(u).astype(np.int64), 0, W - 1)
    y0 = np.clip(np.floor(v).astype(np.int64), 0, H - 1)
    fx, fy = (u - x0)[:, None], (v - y0)[:, None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    a = tex[y0, x0] + fx * (tex[y0, x1] - tex[y0, x0])
    b = tex[y1, x0] + fx * (tex[y1, x1] - tex[y1, x0])
    return a + fy * (b - a)


def view_decisions(pts, f, p):
    """(sure [n] bool, possible [n] bool, z [n], u [n], v [n]): is each point seen by view f under parameters p (lv_paint_params)."""
    H, W = np.asarray(f["image"]).shape[:2]
    s, w = int(p.zbuf_scale), int(p.window)
    cw, ch = -(-W // s), -(-H // s)
    z, rho, u, v = project(pts, f)
    mn, mx, nr = float(np.float32(p.min_depth)), float(np.float32(p.max_depth)), float(np.float32(p.max_norm_radius))
    with np.errstate(invalid="ignore"):
        sure = (z >= mn + M_EPS) & (z <= mx - M_EPS) & (rho <= nr - NR_EPS) & (u >= PX_EPS) & (u <= W - 1 - PX_EPS) & (v >= PX_EPS) & \
               (v <= H - 1 - PX_EPS)
        maybe = (z >= mn - M_EPS) & (z <= mx + M_EPS) & (rho <= nr + NR_EPS) & (u >= -PX_EPS) & (u <= W - 1 + PX_EPS) & \
                (v >= -PX_EPS) & (v <= H - 1 + PX_EPS)
    n = len(z)
    idx = np.flatnonzero(maybe)
    uu, vv, zz = np.clip(u[idx], 0, W - 1), np.clip(v[idx], 0, H - 1), z[idx]
    # a cell coordinate and the neighbour it could be instead (itself when the point is clear of a cell edge)
    cands = []
    for q, nc in ((uu, cw), (vv, ch)):
        a = (q + 0.5) / s
        c = np.floor(a)
        fr = (q + 0.5) - c * s
        alt = np.where(fr < PX_EPS, c - 1, np.where(s - fr < PX_EPS, c + 1, c))
        cands.append((np.clip(c, 0, nc - 1).astype(np.int64), np.clip(alt, 0, nc - 1).astype(np.int64)))
    (cx, cx2), (cy, cy2) = cands
    amb = ~sure[idx] | (cx != cx2) | (cy != cy2)
    hi_buf = np.full(ch * cw, np.inf)      # upper bound: the unambiguous points only
    np.minimum.at(hi_buf, (cy * cw + cx)[~amb], zz[~amb])
    lo_buf = hi_buf.copy()                 # lower bound: every ambiguous point in every cell it could take
    for a in (cx, cx2):
        for b in (cy, cy2):
            np.minimum.at(lo_buf, (b * cw + a)[amb], zz[amb])
    hi_win = _window_min(hi_buf.reshape(ch, cw), w).ravel()
    lo_win = _window_min(lo_buf.reshape(ch, cw), w).ravel()
    thr = np.maximum(np.float32(p.margin_abs), np.float32(p.margin_rel) * zz)
    s_all = np.ones(len(idx), bool)
    p_any = np.zeros(len(idx), bool)
    for a in (cx, cx2):
        for b in (cy, cy2):
            k = b * cw + a
            with np.errstate(invalid="ignore"):
                s_all &= zz - lo_win[k] <= thr - M_EPS
                p_any |= zz - hi_win[k] <= thr + M_EPS
    out_s = np.zeros(n, bool)
    out_p = np.zeros(n, bool)
    out_s[idx] = sure[idx] & s_all
    out_p[idx] = p_any
    return out_s, out_p, z, u, v


def paint(pts, frames, p):
    """(rgb [n, 3], depth [n], lo [n], hi [n], decided [n]): the reference outputs for every map point (rgb and depth on the
    decided points, where every view's decision is sure), the interval [lo, hi] of each count."""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    lo = np.zeros(n, np.int64)
    hi = np.zeros(n, np.int64)
    decided = np.ones(n, bool)
    acc = np.zeros((n, 3))
    best = np.full(n, np.inf)
    near = np.zeros((n, 3))
    for f in frames:
        sure, maybe, z, u, v = view_decisions(pts, f, p)
        lo += sure
        hi += maybe
        decided &= sure == maybe
        k = np.flatnonzero(sure)
        if len(k):
            img = np.asarray(f["image"])
            smp = bilinear(texels(img, int(f.get("format", 2 if img.ndim == 2 else 0))), u[k], v[k])
            acc[k] += smp
            closer = z[k] < best[k]
            near[k[closer]] = smp[closer]
            best[k] = np.minimum(best[k], z[k])
    rgb = np.zeros((n, 3))
    if int(p.blend) == 0:
        ok = lo > 0
        rgb[ok] = acc[ok] / lo[ok, None]
    else:
        rgb = near
    return rgb, best, lo, hi, decided
