"""The rule of lv_map_planes (include/limovelo_hip.h "Plane segmentation") restated with numpy and Python ints: the reference of
tests/test_planes_host.py and tests/test_gpu_map_planes.py.  Nothing here comes from the code under test.

uint64 hash in Python ints; the hypothesis planes in numpy f64, one operation per line of the rule (numpy does not fuse); the
inlier test as a K x n f32 score matrix; the refit in exact Python ints with a line-by-line port of sym3_eig (lv_surface.hpp) on
Python floats (IEEE f64, unfused, math.sqrt correctly rounded)."""
import math

import numpy as np

F = np.float32
M64 = (1 << 64) - 1
QUANT_MAX = 1 << 22
DEFAULTS = dict(distance=0.1, iterations=512, max_planes=1, min_inliers=100, seed=0, constraint=0, axis=(0.0, 0.0, 1.0),
                max_angle=float(F(10.0 * math.pi / 180.0)), refine=1)


def b32(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def b64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- step 2: the draws
def mix(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, r, h, j, n):
    u = mix((seed & M64) ^ mix((r << 40) | (h << 8) | j))
    return (u * n) >> 64


def draws(seed, r, K, n):
    """[K, 3] indices"""
    return np.array([[draw(seed, r, h, j, n) for j in range(3)] for h in range(K)], np.int64).reshape(K, 3)


# ---- the resolved rule
def resolve(params):
    """axis normalised in f64 and both thresholds, as the host resolves them once (libm's cos / sin)"""
    p = {**DEFAULTS, **params}
    q = dict(p, axis_hat=(0.0, 0.0, 0.0), cos_max=0.0, sin_max=0.0, refine=1 if p["refine"] else 0, distance=F(p["distance"]))
    if p["constraint"] != 0:
        x, y, z = (float(F(v)) for v in p["axis"])
        ln = math.sqrt((x * x + y * y) + z * z)
        a = float(F(p["max_angle"]))
        q.update(axis_hat=(x / ln, y / ln, z / ln), cos_max=math.cos(a), sin_max=math.sin(a))
    return q


# ---- step 3: the plane of a hypothesis (vectorised over hypotheses)
def sign_rule(n, constraint, axis):
    """[K] of +1 / -1 for the normals n [K, 3] (f64): towards the axis with constraint 1, else / on a zero dot product the
    component of largest magnitude positive, ties to the lower axis"""
    big = n[:, 0].copy()
    for a in (1, 2):
        take = np.abs(n[:, a]) > np.abs(big)
        big = np.where(take, n[:, a], big)
    sg = np.where(big < 0.0, -1.0, 1.0)
    if constraint == 1:
        d = (n[:, 0] * axis[0] + n[:, 1] * axis[1]) + n[:, 2] * axis[2]
        sg = np.where(d > 0.0, 1.0, np.where(d < 0.0, -1.0, sg))
    return sg


def hypotheses(p0, p1, p2, constraint=0, axis=(0.0, 0.0, 0.0), cos_max=0.0, sin_max=0.0):
    """(valid [K] bool, normal [K, 3] f32, zero where invalid) of the f32 point triples [K, 3]"""
    p0, p1, p2 = (np.asarray(p, F).reshape(-1, 3).astype(np.float64) for p in (p0, p1, p2))
    with np.errstate(all="ignore"):
        u = p1 - p0
        v = p2 - p0
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        cc = (cx * cx + cy * cy) + cz * cz
        uu = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        valid = cc > 1e-12 * (uu * vv)
        ln = np.sqrt(cc)
        n = np.stack([cx / ln, cy / ln, cz / ln], axis=1)
        n = np.where(valid[:, None], n, 0.0)
        n = sign_rule(n, constraint, axis)[:, None] * n
        if constraint != 0:
            t = np.abs((n[:, 0] * axis[0] + n[:, 1] * axis[1]) + n[:, 2] * axis[2])
            valid = valid & ((t >= cos_max) if constraint == 1 else (t <= sin_max))
        return valid, np.where(valid[:, None], n, 0.0).astype(F)


# ---- step 4: the inlier test
def signed(normal, anchor, pts):
    """s [K, n] f32 of the planes (normal, anchor [K, 3] f32) against pts [n, 3] f32"""
    normal, anchor, pts = (np.asarray(a, F).reshape(-1, 3) for a in (normal, anchor, pts))
    with np.errstate(all="ignore"):
        qx = pts[None, :, 0] - anchor[:, None, 0]
        qy = pts[None, :, 1] - anchor[:, None, 1]
        qz = pts[None, :, 2] - anchor[:, None, 2]
        return (normal[:, None, 0] * qx + normal[:, None, 1] * qy) + normal[:, None, 2] * qz


def inliers(normal, anchor, pts, distance):
    return np.abs(signed(normal, anchor, pts)) <= F(distance)


def counts(valid, normal, anchor, pts, distance, chunk=64):
    """[K] inlier counts (0 for an invalid hypothesis): the K x n score matrix, a few rows at a time"""
    out = np.zeros(len(valid), np.int64)
    for lo in range(0, len(valid), chunk):
        out[lo:lo + chunk] = inliers(normal[lo:lo + chunk], anchor[lo:lo + chunk], pts, distance).sum(axis=1)
    return np.where(valid, out, 0)


# ---- step 6: the refit
def quant(p, a):
    """(ok, g) of g = rintf((p - a) * 256), f32; ok: |g| <= 2^22"""
    with np.errstate(all="ignore"):
        r = np.rint((np.asarray(p, F) - np.asarray(a, F)) * F(256.0))
        ok = np.abs(r) <= F(QUANT_MAX)
    return ok, np.where(ok, r, F(0)).astype(np.int64)


def sums(pts, anchor):
    """the exact sums (Python ints) of the points whose three coordinates quantise: n_fit, S1[3], S2[6] (xx xy xz yy yz zz)"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    ok, g = quant(pts, np.asarray(anchor, F)[None, :])
    g = g[ok.all(axis=1)]
    s1 = [sum(int(v) for v in g[:, a]) for a in range(3)]
    s2 = [sum(int(x) * int(y) for x, y in zip(g[:, a], g[:, b])) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return len(g), s1, s2


def moment(n, s1, s2):
    """M = n S2 - S1 S1^T in Python ints, each entry converted to f64 once (int -> float rounds to nearest even)"""
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return [float(n * s2[k] - s1[a] * s1[b]) for k, (a, b) in enumerate(pairs)]


def _rotate(app, aqq, apq, aop, aoq, v0p, v0q, v1p, v1q, v2p, v2q):
    if apq == 0.0:
        return app, aqq, apq, aop, aoq, v0p, v0q, v1p, v1q, v2p, v2q
    d = aqq - app
    two = 2.0 * apq
    den = abs(d) + math.sqrt(d * d + two * two)
    t = two / den if den > 0.0 else (-1.0 if two < 0.0 else 1.0)
    if d < 0.0:
        t = -t
    cs = 1.0 / math.sqrt(t * t + 1.0)
    sn = t * cs
    tau = sn / (1.0 + cs)
    app = app - t * apq
    aqq = aqq + t * apq
    apq = 0.0
    op, oq = aop, aoq
    aop = op - sn * (oq + tau * op)
    aoq = oq + sn * (op - tau * oq)
    out = []
    for vp, vq in ((v0p, v0q), (v1p, v1q), (v2p, v2q)):
        out += [vp - sn * (vq + tau * vp), vq + sn * (vp - tau * vq)]
    return (app, aqq, apq, aop, aoq, *out)


def _rayleigh(m00, m01, m02, m11, m12, m22, x, y, z):
    nn = math.sqrt(x * x + y * y + z * z)
    x, y, z = x / nn, y / nn, z / nn
    mx = m00 * x + m01 * y + m02 * z
    my = m01 * x + m11 * y + m12 * z
    mz = m02 * x + m12 * y + m22 * z
    return x * mx + y * my + z * mz, x, y, z


def sym3_eig(c):
    """(l [3], v0 [3]): the port of lv::sym3_eig, line by line"""
    c0, c1, c2, c3, c4, c5 = (float(v) for v in c)
    big = max(abs(c0), abs(c1), abs(c2), abs(c3), abs(c4), abs(c5))
    if not (big > 0.0) or not (big < math.inf):
        e = big if big > 0.0 else 0.0
        return [e, e, e], [0.0, 0.0, 1.0]
    e = math.frexp(big)[1] - 1
    s, si = math.ldexp(1.0, -e), math.ldexp(1.0, e)
    m00, m01, m02, m11, m12, m22 = c0 * s, c1 * s, c2 * s, c3 * s, c4 * s, c5 * s
    a00, a01, a02, a11, a12, a22 = m00, m01, m02, m11, m12, m22
    v00, v01, v02, v10, v11, v12, v20, v21, v22 = 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0
    for _ in range(5):
        a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21 = _rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22 = _rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22 = _rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    q0, v00, v10, v20 = _rayleigh(m00, m01, m02, m11, m12, m22, v00, v10, v20)
    q1, v01, v11, v21 = _rayleigh(m00, m01, m02, m11, m12, m22, v01, v11, v21)
    q2, v02, v12, v22 = _rayleigh(m00, m01, m02, m11, m12, m22, v02, v12, v22)
    l0 = min(q0, min(q1, q2))
    w0 = 1.0 if q0 == l0 else 0.0
    w1 = 1.0 if (q0 != l0 and q1 == l0) else 0.0
    w2 = 1.0 - w0 - w1
    x0 = (w0 * v00 + w1 * v01) + w2 * v02
    y0 = (w0 * v10 + w1 * v11) + w2 * v12
    z0 = (w0 * v20 + w1 * v21) + w2 * v22
    l2 = max(q0, max(q1, q2))
    l1 = max(min(q0, q1), min(max(q0, q1), q2))
    return [l0 * si, l1 * si, l2 * si], [x0, y0, z0]


def refit(n_fit, m, s1, constraint, axis, normal, anchor):
    """(done, normal f32 [3], anchor f32 [3], rms) from the folded sums"""
    normal, anchor = np.asarray(normal, F).copy(), np.asarray(anchor, F).copy()
    if n_fit < 3:
        return False, normal, anchor, math.nan
    l, v = sym3_eig(m)
    sg = float(sign_rule(np.array([v]), constraint, axis)[0])
    normal = np.array([sg * x for x in v], np.float64).astype(F)
    anchor = np.array([float(anchor[a]) + float(s1[a]) / (256.0 * float(n_fit)) for a in range(3)], np.float64).astype(F)
    return True, normal, anchor, math.sqrt(l[0] if l[0] > 0.0 else 0.0) / (256.0 * float(n_fit))


def offset(normal, anchor):
    n, a = (np.asarray(v, F).astype(np.float64) for v in (normal, anchor))
    return -float((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2])


# ---- the whole rule
def round_counts(pts, q, r):
    """(idx [K, 3], valid [K], normal [K, 3], anchor [K, 3], count [K]) of round r over the candidates pts [n, 3]"""
    K, n = q["iterations"], len(pts)
    idx = draws(q["seed"], r, K, n)
    distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    valid, normal = hypotheses(pts[idx[:, 0]], pts[idx[:, 1]], pts[idx[:, 2]], q["constraint"], q["axis_hat"], q["cos_max"], q["sin_max"])
    valid = valid & distinct
    anchor = pts[idx[:, 0]]
    return idx, valid, normal, anchor, counts(valid, normal, anchor, pts, q["distance"])


def segment(xyz, params=None, mask=None):
    """dict(labels [m] int32, planes [list of dicts], n_planes) of the living points xyz [m, 3] f32 in map order"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    q = resolve(params or {})
    labels = np.full(len(xyz), -1, np.int32)
    free = np.ones(len(xyz), bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    planes = []
    for r in range(q["max_planes"]):
        cand = np.flatnonzero(free)
        n = len(cand)
        if n < 3 or n < q["min_inliers"]:
            break
        pts = xyz[cand]
        _, valid, normal, anchor, cnt = round_counts(pts, q, r)
        if not valid.any():
            break
        h = int(np.argmax(cnt))   # (the first of the largest: ties to the smaller h; an invalid hypothesis counts 0)
        if not valid[h] or cnt[h] < q["min_inliers"]:
            break
        nrm, anc = normal[h].copy(), anchor[h].copy()
        rec = dict(support=int(cnt[h]), hypothesis=h, candidates=n, n_fit=0, flags=0, rms=math.nan)
        if q["refine"]:
            win = inliers(nrm[None], anc[None], pts, q["distance"])[0]
            n_fit, s1, s2 = sums(pts[win], anc)
            done, nrm, anc, rms = refit(n_fit, moment(n_fit, s1, s2), s1, q["constraint"], q["axis_hat"], nrm, anc)
            rec.update(n_fit=n_fit, flags=1 if done else 0, rms=rms)
        member = inliers(nrm[None], anc[None], pts, q["distance"])[0]
        labels[cand[member]] = r
        free[cand[member]] = False
        rec.update(normal=nrm, anchor=anc, d=offset(nrm, anc), inliers=int(member.sum()))
        planes.append(rec)
    return dict(labels=labels, planes=planes, n_planes=len(planes))


# ---- which inputs are degenerate
def degenerate(xyz):
    """None, "duplicate" (every point equals the first) or "collinear" (every triple is a sliver: all points within f32 rounding
    of one line, judged on the exact offsets from the first point)"""
    xyz = np.asarray(xyz, F).reshape(-1, 3).astype(np.float64)
    off = xyz - xyz[0]
    if not off.any():
        return "duplicate"
    far = off[np.argmax((off * off).sum(axis=1))]
    c = np.cross(off, far[None, :])
    cc, uu, vv = (c * c).sum(axis=1), (off * off).sum(axis=1), (far * far).sum()
    return "collinear" if np.all(cc <= 1e-12 * uu * vv) else None
