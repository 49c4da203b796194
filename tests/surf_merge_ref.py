"""numpy statement of the submap merge's rule (include/limovelo_hip.h "Submap merging") for the tests.

Every f64 step is one np.float64 elementwise operation in the order the header writes it (the rotation is spelled out term by
term, never as a matrix product); everything after the lattice is int64.  The device and the emulator are held to this file by
EQUALITY on S, W and the four stats.  Volumes are [nz, ny, nx] arrays (x fastest).  A destination is a dict: origin [3],
resolution, trunc_cells, max_weight, S, W.  A submap is a dict: origin [3], resolution, trunc_cells, S, W.  A pose is (t [3],
q [4] as x, y, z, w), submap -> world."""
import numpy as np

import depth_ref as dr

F = np.float32
D = np.float64
I = np.int64
FR = 32
OUTSIDE, UNKNOWN, KNOWN = 0, 1, 2
TRILINEAR, NEAREST = 0, 1


def rot(q):
    """R(q) as lv_graph.hpp's gr_rot builds it, f64, [3, 3]."""
    x, y, z, w = (D(v) for v in q)
    two, one = D(2.0), D(1.0)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], D)


def quat(axis, angle):
    """A unit quaternion x, y, z, w about `axis`."""
    a = np.asarray(axis, D)
    a = a / np.linalg.norm(a)
    q = np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])
    return q / np.linalg.norm(q)


IDENTITY = (np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]))


def scale(sub_resolution, resolution):
    """kq of step 6, or None where lv_surf_merge refuses the ratio."""
    k = np.floor((F(sub_resolution) / F(resolution)) * F(4096.0) + F(0.5))
    assert k.dtype == F
    return int(k) if 512 <= k <= 32768 else None


def lattice(centres, sub, pose, interp=TRILINEAR):
    """Steps 2 and 3 on f32 centres (x, y, z arrays): (inside, e [3] int64).  inside False: |u| >= 2^24 or not finite."""
    t, q = pose
    R = rot(q)
    t = np.asarray(t, D)
    d = [np.asarray(c, F).astype(D) - t[a] for a, c in enumerate(centres)]
    inside = np.ones(d[0].shape, bool)
    e = []
    with np.errstate(all="ignore"):
        for b in range(3):
            x = (R[0, b] * d[0] + R[1, b] * d[1]) + R[2, b] * d[2]
            u = (x - D(F(sub["origin"][b]))) / D(F(sub["resolution"])) - D(0.5)
            ok = np.abs(u) < D(16777216.0)
            inside &= ok
            u = np.where(ok, u, 0.0)
            e.append(FR * np.floor(u + D(0.5)).astype(I) if interp == NEAREST else np.floor(u * D(32.0) + D(0.5)).astype(I))
    return inside, e


def gather(sub, inside, e, min_weight=1):
    """Steps 4 and 5: dict(state, m, Wn int64, i [3], f [3]); m and Wn are zero unless KNOWN."""
    S = np.asarray(sub["S"], I)
    W = np.asarray(sub["W"], I)
    n = S.shape[::-1]   # nx, ny, nz
    i = [v >> 5 for v in e]
    f = [v & 31 for v in e]
    state_in = inside.copy()
    for b in range(3):
        state_in &= (i[b] >= 0) & (i[b] <= n[b] - 1) & ((f[b] == 0) | (i[b] + 1 <= n[b] - 1))
    known = state_in.copy()
    m = np.zeros(inside.shape, I)
    Wn = np.zeros(inside.shape, I)
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        w = np.ones(inside.shape, I)
        for b in range(3):
            w = w * (f[b] if o[b] else FR - f[b])
        read = state_in & (w != 0)
        idx = [np.where(read, i[b] + o[b], 0) for b in range(3)]
        assert all(v.min() >= 0 and v.max() <= n[b] - 1 for b, v in enumerate(idx))
        Sc = np.where(read, S[idx[2], idx[1], idx[0]], 0)
        Wc = np.where(read, W[idx[2], idx[1], idx[0]], 0)
        known &= ~read | (Wc >= min_weight)
        a = (Sc * 256) // np.maximum(Wc, 1)   # (// floors)
        assert np.abs(a).max(initial=0) <= 1 << 20
        m += np.where(read, w * a, 0)
        Wn += np.where(read, w * Wc, 0)
    state = np.where(state_in, np.where(known, KNOWN, UNKNOWN), OUTSIDE)
    m = np.where(known, m, 0)
    Wn = np.where(known, Wn, 0)
    assert np.abs(m).max(initial=0) <= 1 << 35 and Wn.max(initial=0) <= 1 << 33
    return dict(state=state, m=m, Wn=Wn, i=i, f=f)


def delta(kq, Td, m, Wn, known):
    """Steps 6 and 7: dict(dS, dW int64, dropped, clamped bool)."""
    prod = m * I(kq)
    assert np.abs(prod).max(initial=0) <= 1 << 50
    sbar = prod // I(1 << 27)
    lim = 256 * int(Td)
    dropped = known & (sbar < -lim)
    clamped = known & (sbar > lim)
    sbar = np.minimum(sbar, lim)
    adds = known & ~dropped
    dW = np.where(adds, np.maximum(1, Wn >> 15), 0)
    dS = np.where(adds, (sbar * dW) // 256, 0)
    return dict(dS=dS, dW=dW, dropped=dropped, clamped=clamped)


def merge(dest, sub, pose, min_weight=1, interp=TRILINEAR):
    """One lv_surf_merge of `sub` at `pose` into `dest`: dict(S, W int32 after; stats [4] uint64: voxels not OUTSIDE, voxels that
    contribute, the sum of dW, voxels DROPPED; state, dS, dW, dropped, clamped, folded, i, f per destination voxel).  None where
    the resolution ratio is refused."""
    S = np.asarray(dest["S"], np.int32)
    W = np.asarray(dest["W"], np.int32)
    kq = scale(sub["resolution"], dest["resolution"])
    if kq is None:
        return None
    Td = 256 * int(dest["trunc_cells"])
    inside, e = lattice(dr.centres(dest["origin"], dest["resolution"], S.shape), sub, pose, interp)
    g = gather(sub, inside, e, min_weight)
    d = delta(kq, Td, g["m"], g["Wn"], g["state"] == KNOWN)
    S2, W2 = dr.fold(S, W, d["dS"], d["dW"], dest["max_weight"])
    assert np.all(np.abs(S2.astype(I)) <= Td * W2.astype(I))
    assert np.abs(S.astype(I) + d["dS"]).max(initial=0) <= 1 << 31
    folded = (d["dW"] > 0) & (W.astype(I) + d["dW"] > int(dest["max_weight"]))
    stats = np.array([(g["state"] != OUTSIDE).sum(), (d["dW"] > 0).sum(), d["dW"].sum(), d["dropped"].sum()], np.uint64)
    return dict(S=S2, W=W2, stats=stats, state=g["state"], dS=d["dS"], dW=d["dW"], dropped=d["dropped"], clamped=d["clamped"], folded=folded,
                i=g["i"], f=g["f"], e=e, m=g["m"], Wn=g["Wn"], kq=kq)


def box(dest, sub, pose):
    """surf_merge_box: the destination voxels (lo [3], hi [3]) as x, y, z with hi exclusive that the call is launched over: the eight
    corners of the submap's box of metres carried to the world in f64, widened by a voxel and 1e-3 of the box's size and of its
    distance from the volume's origin, clipped to the grid.  None: the submap cannot meet the volume."""
    R = rot(pose[1])
    t = np.asarray(pose[0], D)
    n = sub["S"].shape[::-1]
    so, sr = [D(F(v)) for v in sub["origin"]], D(F(sub["resolution"]))
    lo, hi = [], []
    for a in range(3):
        xs = []
        for k in range(8):
            c = [so[b] + (D(n[b]) * sr if (k >> b) & 1 else D(0.0)) for b in range(3)]
            xs.append(((R[a, 0] * c[0] + R[a, 1] * c[1]) + R[a, 2] * c[2]) + t[a])
        wlo, whi = min(xs), max(xs)
        res, o, dim = D(F(dest["resolution"])), D(F(dest["origin"][a])), dest["S"].shape[2 - a]
        slack = res + D(1e-3) * (whi - wlo) + D(1e-3) * max(abs(wlo - o), abs(whi - o))
        flo = np.floor((wlo - slack - o) / res - D(0.5))
        fhi = np.ceil((whi + slack - o) / res - D(0.5)) + D(1.0)
        if not flo < dim or not fhi > 0:
            return None
        lo.append(int(flo) if flo > 0 else 0)
        hi.append(int(fhi) if fhi < dim else dim)
    return lo, hi


def box_voxels(dest, sub, pose):
    b = box(dest, sub, pose)
    return 0 if b is None else int(np.prod([h - l for l, h in zip(*b)]))


def merged(dest, r):
    """The destination after a merge result r."""
    return dict(dest, S=r["S"], W=r["W"])


def fuse(dest, submaps, poses, **kw):
    """mesh.Submaps.fuse: the destination cleared, then one merge per submap; (destination after, summed stats)."""
    d = dict(dest, S=np.zeros_like(dest["S"]), W=np.zeros_like(dest["W"]))
    stats = np.zeros(4, np.uint64)
    for s, p in zip(submaps, poses):
        r = merge(d, s, p, **kw)
        d = merged(d, r)
        stats += r["stats"]
    return d, stats
