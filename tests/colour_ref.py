"""numpy statement of the colour layer's rule (include/limovelo_hip.h "Colour layer") for the tests.

Candidates, fold, voxel and vertex colours are integers and are restated exactly.  The per-view decisions on the candidates'
centres are paint_ref.view_decisions', so every count is an interval [lo, hi] and a voxel is DECIDED when every view's decision
is, as for lv_map_paint.  Volumes are [nz, ny, nx] arrays (x fastest), layers [nz, ny, nx, 4] uint32 (C[0], C[1], C[2], Wc)."""
import numpy as np

import paint_ref as pr

F = np.float32
U = np.uint64


def candidates(S, W, min_weight, band):
    """bool [nz, ny, nx]: W >= min_weight and |S| <= band * W."""
    S = np.asarray(S, np.int64)
    W = np.asarray(W, np.int64)
    return (W >= int(min_weight)) & (np.abs(S) <= int(band) * W)


def centres(origin, resolution, shape, flat):
    """f32 [n, 3]: the centres of the voxels with linear indices `flat` of a volume of shape (nz, ny, nx): per axis
    origin + resolution * ((float)(256 i + 128) / 256), f32 and unfused."""
    nz, ny, nx = shape
    flat = np.asarray(flat, np.int64)
    ijk = np.stack([flat % nx, (flat // nx) % ny, flat // (nx * ny)], axis=1)
    v = (256 * ijk + 128).astype(F)
    o = np.asarray(origin, F)
    return (o[None, :] + F(resolution) * (v / F(256.0))).astype(F)


def quantise(s):
    """The level 0..255 of a sample s in [0, 255]: (uint32)(s + 0.5)."""
    return np.minimum(np.floor(np.asarray(s, np.float64) + 0.5), 255).astype(U)


def fold(sums, n, dC, max_weight):
    """The layer entries sums [m, 4] after n [m] seeing views whose levels sum to dC [m, 3]; entries with n = 0 stay."""
    sums = np.asarray(sums, U).copy()
    n = np.asarray(n, U)
    dC = np.asarray(dC, U)
    mw = U(max_weight)
    Wn = sums[:, 3] + n
    Cn = sums[:, :3] + dC
    over = Wn > mw
    C = np.where(over[:, None], (Cn * mw) // np.maximum(Wn, U(1))[:, None], Cn)
    out = np.concatenate([C, np.where(over, mw, Wn)[:, None]], axis=1)
    hit = n > 0
    sums[hit] = out[hit]
    return sums.astype(np.uint32)


def voxel_colour(sums):
    """uint8 [..., 4] r, g, b, a of entries [..., 4]: (2 C + Wc) / (2 Wc), alpha 255; Wc = 0: zeros."""
    s = np.asarray(sums, U)
    w = s[..., 3:4]
    ok = w > 0
    c = np.where(ok, (U(2) * s[..., :3] + w) // np.maximum(U(2) * w, U(1)), 0)
    return np.concatenate([c, np.where(ok, 255, 0)], axis=-1).astype(np.uint8)


def vertex_colour(corners):
    """uint8 [V, 4] from the entries of each vertex's 8 corner voxels, corners [V, 8, 4]."""
    corners = np.asarray(corners, U)
    col = voxel_colour(corners).astype(U)
    has = corners[:, :, 3] > 0
    k = has.sum(axis=1).astype(U)
    total = (col[:, :, :3] * has[:, :, None]).sum(axis=1).astype(U)
    ok = k > 0
    c = np.where(ok[:, None], (U(2) * total + k[:, None]) // np.maximum(U(2) * k, U(1))[:, None], 0)
    return np.concatenate([c, np.where(ok, 255, 0)[:, None]], axis=1).astype(np.uint8)


def active_cells(S, W, min_weight=1):
    """bool [nz - 1, ny - 1, nx - 1]: the active cells of the mesh rule (all 8 corners known, not all of one sign)."""
    S = np.asarray(S, np.int64)
    W = np.asarray(W, np.int64)
    nz, ny, nx = S.shape
    cz, cy, cx = max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)
    known, inside = W >= min_weight, S < 0
    all_known = np.ones((cz, cy, cx), bool)
    n_in = np.zeros((cz, cy, cx), np.int64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                all_known &= known[dz:dz + cz, dy:dy + cy, dx:dx + cx]
                n_in += inside[dz:dz + cz, dy:dy + cy, dx:dx + cx]
    return all_known & (n_in > 0) & (n_in < 8)


def mesh_colours(S, W, layer, min_weight=1):
    """uint8 [V, 4]: the vertex colours of the mesh of (S, W), in vertex order (the cells' linear order), from layer."""
    act = active_cells(S, W, min_weight)
    kk, jj, ii = np.nonzero(act)   # (C order of [cz, cy, cx] is the linear order)
    layer = np.asarray(layer)
    corners = np.stack([layer[kk + ((n >> 2) & 1), jj + ((n >> 1) & 1), ii + (n & 1)] for n in range(8)], axis=1)
    return vertex_colour(corners.reshape(-1, 8, 4))


def shift_layer(a, d):
    """The volume or layer a ([nz, ny, nx, ...]) after a recentre by d = (dx, dy, dz): new (i, j, k) holds old (i + d), else 0."""
    out = np.zeros_like(a)
    nz, ny, nx = a.shape[:3]
    dx, dy, dz = (int(v) for v in d)

    def span(n, s):   # destination and source slices along one axis
        lo, hi = max(0, -s), min(n, n - s)
        return (slice(lo, hi), slice(lo + s, hi + s)) if hi > lo else (slice(0, 0), slice(0, 0))

    (zx, sx), (zy, sy), (zz, sz) = span(nx, dx), span(ny, dy), span(nz, dz)
    out[zz, zy, zx] = a[sz, sy, sx]
    return out


def _gate(pts, f, p):
    """(sure, maybe) bool [n]: does the point pass steps 1 to 3 of view f (paint_ref's margins)."""
    H, W = np.asarray(f["image"]).shape[:2]
    z, rho, u, v = pr.project(pts, f)
    mn, mx, nr = float(F(p.min_depth)), float(F(p.max_depth)), float(F(p.max_norm_radius))
    e, m, r = pr.PX_EPS, pr.M_EPS, pr.NR_EPS
    with np.errstate(invalid="ignore"):
        sure = (z >= mn + m) & (z <= mx - m) & (rho <= nr - r) & (u >= e) & (u <= W - 1 - e) & (v >= e) & (v <= H - 1 - e)
        maybe = (z >= mn - m) & (z <= mx + m) & (rho <= nr + r) & (u >= -e) & (u <= W - 1 + e) & (v >= -e) & (v <= H - 1 + e)
    return sure, maybe


def integrate(S, W, layer, origin, resolution, frames, prm):
    """One lv_colour_integrate on the volume (S, W) and the layer [nz, ny, nx, 4] (None: all zero), prm an lv_colour_params.
    dict(flat: the candidates' linear indices; lo, hi [m]: the interval of each candidate's n; decided [m] bool; dC [m, 3]: the
    levels summed over the surely seeing views; after [nz, ny, nx, 4] uint32: the layer after the call, right on the decided
    voxels (the others keep their old entry); stats_lo, stats_hi [4] uint64; possible, undecided: the (voxel, view) decisions
    that could be seen and those of them the reference leaves open)."""
    S = np.asarray(S)
    shape = S.shape
    layer = np.zeros(shape + (4,), np.uint32) if layer is None else np.asarray(layer, np.uint32)
    flat = np.flatnonzero(candidates(S, W, prm.min_weight, prm.band).ravel())
    pts = centres(origin, resolution, shape, flat)
    m = len(flat)
    lo, hi = np.zeros(m, np.int64), np.zeros(m, np.int64)
    decided = np.ones(m, bool)
    dC = np.zeros((m, 3), U)
    pairs_lo = pairs_hi = undecided = 0
    for f in frames:
        g_sure, g_maybe = _gate(pts, f, prm.view) if m else (np.zeros(0, bool), np.zeros(0, bool))
        pairs_lo += int(g_sure.sum())
        pairs_hi += int(g_maybe.sum())
        if not m:
            continue
        sure, maybe, z, u, v = pr.view_decisions(pts, f, prm.view)
        lo += sure
        hi += maybe
        decided &= sure == maybe
        undecided += int((sure != maybe).sum())
        k = np.flatnonzero(sure)
        if len(k):
            img = np.asarray(f["image"])
            smp = pr.bilinear(pr.texels(img, int(f.get("format", 2 if img.ndim == 2 else 0))), u[k], v[k])
            dC[k] += quantise(smp)
    after = layer.reshape(-1, 4).copy()
    ok = decided
    after[flat[ok]] = fold(after[flat[ok]], lo[ok], dC[ok], prm.max_weight)
    stats_lo = np.array([m, pairs_lo, lo.sum(), (lo > 0).sum()], U)
    stats_hi = np.array([m, pairs_hi, hi.sum(), (hi > 0).sum()], U)
    return dict(flat=flat, lo=lo, hi=hi, decided=decided, dC=dC, after=after.reshape(shape + (4,)), stats_lo=stats_lo, stats_hi=stats_hi,
                possible=int(hi.sum()), undecided=undecided)
