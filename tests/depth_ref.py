"""numpy statement of the depth fusion's rule (include/limovelo_hip.h "Depth fusion") for the tests.

Every f32 step is one np.float32 elementwise operation in the order the header writes it (the manner of occupancy_ref.quant_f and
rollout_ref): the projection is spelled out term by term, never as a matrix product, so the device and the emulator are held to
this file by EQUALITY on S, W and the four stats.  Volumes are [nz, ny, nx] arrays (x fastest).  A frame is a dict: R [3, 3] and
t [3] camera -> world, fx, fy, cx, cy, optional dist (k1, k2, p1, p2, k3), depth ([h, w] uint16 or float32), optional depth_scale
(uint16 only, default 0.001).  Parameters are a Params (or anything with its four attributes)."""
from dataclasses import dataclass

import numpy as np

F = np.float32
I = np.int64
Q = 256


@dataclass
class Params:
    min_depth: float = 0.3
    max_depth: float = 10.0
    max_norm_radius: float = 1.5
    carve: int = 0


def centre(origin, resolution, i):
    """f32: origin + resolution * ((float)(256 i + 128) / 256), the colour layer's centre."""
    v = (Q * np.asarray(i, I) + 128).astype(F)
    return F(origin) + F(resolution) * (v / F(256.0))


def centres(origin, resolution, shape):
    """(x, y, z) f32 [nz, ny, nx] each: the centre of every voxel."""
    nz, ny, nx = shape
    x = centre(origin[0], resolution, np.arange(nx))
    y = centre(origin[1], resolution, np.arange(ny))
    z = centre(origin[2], resolution, np.arange(nz))
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return X, Y, Z


def project(px, py, pz, f, prm):
    """"Map painting" steps 1 to 3 on the points (px, py, pz): (ok, z, u, v); z, u, v mean nothing where ok is False."""
    R = np.asarray(f["R"], F).reshape(9)
    t = np.asarray(f["t"], F).reshape(3)
    dist = f.get("dist")
    k1, k2, p1, p2, k3 = (F(x) for x in np.asarray(np.zeros(5) if dist is None else dist, F).reshape(5))
    fx, fy, cx, cy = F(f["fx"]), F(f["fy"]), F(f["cx"]), F(f["cy"])
    h, w = np.asarray(f["depth"]).shape
    two, one = F(2.0), F(1.0)
    with np.errstate(all="ignore"):
        dx, dy, dz = px - t[0], py - t[1], pz - t[2]
        X = (R[0] * dx + R[3] * dy) + R[6] * dz
        Y = (R[1] * dx + R[4] * dy) + R[7] * dz
        z = (R[2] * dx + R[5] * dy) + R[8] * dz
        ok = (z >= F(prm.min_depth)) & (z <= F(prm.max_depth))
        x = X / z
        y = Y / z
        r2 = x * x + y * y
        ok &= r2 <= F(prm.max_norm_radius) * F(prm.max_norm_radius)
        r4 = r2 * r2
        r6 = r4 * r2
        cd = ((one + k1 * r2) + k2 * r4) + k3 * r6
        xy = x * y
        xd = (x * cd + (two * p1) * xy) + p2 * (r2 + (two * x) * x)
        yd = (y * cd + p1 * (r2 + (two * y) * y)) + (two * p2) * xy
        u = fx * xd + cx
        v = fy * yd + cy
        ok &= (u >= F(0.0)) & (u <= F(w - 1)) & (v >= F(0.0)) & (v <= F(h - 1))
    for a in (z, u, v):
        assert a.dtype == F
    return ok, z, u, v


def measured(raw, fmt_scale, prm):
    """(valid, D) of raw pixel values: uint16 (D = (float)raw * depth_scale, raw 0 invalid) or float32 (the value)."""
    raw = np.asarray(raw)
    if raw.dtype == np.uint16:
        D = raw.astype(F) * F(fmt_scale)
        valid = raw != 0
    else:
        assert raw.dtype == F
        D = raw
        valid = np.ones(raw.shape, bool)
    with np.errstate(invalid="ignore"):
        valid = valid & (D >= F(prm.min_depth)) & (D <= F(prm.max_depth))
    return valid, D


def quantise(D, z, resolution, T, carve):
    """(adds, s, q): step 5 on valid pairs.  q f32 = floorf(((D - z) / resolution) * 256); adds False behind -T and, without carve,
    beyond +T; s int64 (T beyond +T)."""
    with np.errstate(all="ignore"):
        q = np.floor(((D - z) / F(resolution)) * F(256.0))
    assert q.dtype == F
    behind = q < -F(T)
    far = q > F(T)
    adds = ~behind & (~far | bool(carve))
    s = np.where(far, T, np.where(adds & np.isfinite(q), q, 0)).astype(I)   # (q is NaN only on pairs that are not valid)
    return adds, s, q


def view(shape, origin, resolution, T, f, prm):
    """One view on every voxel of the volume: dict of [nz, ny, nx] arrays: ok (passes step 2), valid (ok with a valid D), far
    (valid, q > T), behind (valid, q < -T), band (valid, inside), adds (contributes), s int64, q f32."""
    X, Y, Z = centres(origin, resolution, shape)
    ok, z, u, v = project(X, Y, Z, f, prm)
    img = np.asarray(f["depth"])
    h, w = img.shape
    with np.errstate(all="ignore"):
        px = np.where(ok, np.floor(u + F(0.5)), 0).astype(I)
        py = np.where(ok, np.floor(v + F(0.5)), 0).astype(I)
    assert px.min() >= 0 and px.max() <= w - 1 and py.min() >= 0 and py.max() <= h - 1
    valid, D = measured(img[py, px], f.get("depth_scale", 0.001), prm)
    valid &= ok
    adds, s, q = quantise(D, z, resolution, T, prm.carve)
    adds &= valid
    far = valid & (q > F(T))
    behind = valid & (q < -F(T))
    return dict(ok=ok, valid=valid, far=far, behind=behind, band=valid & ~far & ~behind, adds=adds, s=np.where(adds, s, 0), q=q)


def fold(S, W, dS, dW, max_weight):
    """tsdf_fold on every voxel with dW > 0, int64 throughout: (S, W) int32 after."""
    mw = int(max_weight)
    Wn = np.asarray(W, I) + dW
    Sn = np.asarray(S, I) + dS
    over = Wn > mw
    S2 = np.where(over, (Sn * mw) // np.maximum(Wn, 1), Sn)   # (// floors)
    W2 = np.where(over, mw, Wn)
    hit = dW > 0
    return np.where(hit, S2, S).astype(np.int32), np.where(hit, W2, W).astype(np.int32)


def integrate(S, W, origin, resolution, trunc_cells, max_weight, frames, prm):
    """One lv_depth_integrate on the volume (S, W): dict(S, W int32 after; stats [4] uint64: pairs that pass step 2, those with a
    valid D, the sum of dW, voxels with dW > 0; views: view()'s dict per frame)."""
    S = np.asarray(S, np.int32)
    W = np.asarray(W, np.int32)
    T = int(trunc_cells) * Q
    dS = np.zeros(S.shape, I)
    dW = np.zeros(S.shape, I)
    views = []
    pairs = valid = 0
    for f in frames:
        r = view(S.shape, origin, resolution, T, f, prm)
        pairs += int(r["ok"].sum())
        valid += int(r["valid"].sum())
        dS += r["s"]
        dW += r["adds"]
        views.append(r)
    S2, W2 = fold(S, W, dS, dW, max_weight)
    assert np.all(np.abs(S2.astype(I)) <= T * W2.astype(I))
    stats = np.array([pairs, valid, dW.sum(), (dW > 0).sum()], np.uint64)
    return dict(S=S2, W=W2, stats=stats, views=views)
