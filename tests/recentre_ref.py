"""The rule of the rolling volumes (include/limovelo_hip.h "Rolling volumes") in numpy: what tests/test_recentre_host.py holds the
host build of lv_grid.hpp's shift functions to and tests/test_gpu_volume_recentre.py the kernels, bit for bit.  A shift is a full
array of "never observed" and ONE slice assignment; the origin is two np.float32 operations; lv_occ_mark is np.add.at."""
import numpy as np

import grid_ref as gr

F = np.float32
LIMIT = 1 << 20
NAN_BITS = 0x7FC00000


def shifted(a, d, fill):
    """a [nz, ny, nx] after a recentre by d = (dx, dy, dz): new voxel (i, j, k) holds old (i + dx, j + dy, k + dz) where that lies
    inside, `fill` elsewhere.  A new array of a's type."""
    a = np.asarray(a)
    out = np.full(a.shape, fill, a.dtype)
    dst, src = [], []
    for n, s in zip(a.shape, (d[2], d[1], d[0])):   # (the array's axes are z, y, x)
        s = int(s)
        lo, hi = max(0, -s), min(n, n - s)          # new indices whose source lies inside
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + s, hi + s))
    out[tuple(dst)] = a[tuple(src)]
    return out


def unknown_bits(shape):
    """An occupancy grid never observed, as its bits (uint32): the values move as bits, so the reference compares bits."""
    return np.full(shape, NAN_BITS, np.uint32)


def shift_logodds(L, d):
    """L (f32 [nz, ny, nx]) after a recentre by d, moved as bits; exposed voxels hold exactly NAN_BITS."""
    return shifted(np.ascontiguousarray(L, F).view(np.uint32), d, NAN_BITS).view(F)


def origin_at(origin0, s, resolution):
    """origin0 + (float)s * resolution per axis in f32, unfused, in that order."""
    with np.errstate(all="ignore"):
        return (np.asarray(origin0, F) + (np.asarray(s, np.int64).astype(F) * F(resolution)).astype(F)).astype(F)


def check(origin0, resolution, s, d):
    """(ok, s_new [3] int64, origin_new [3] f32) of a recentre by d at accumulated shift s; not ok: nothing changes."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    if np.any(np.abs(d) > LIMIT) or np.any(np.abs(s + d) > LIMIT):
        return False, s, origin_at(origin0, s, resolution)
    o = origin_at(origin0, s + d, resolution)
    if not np.all(np.isfinite(o)):
        return False, s, origin_at(origin0, s, resolution)
    return True, s + d, o


def stats(evidence, d):
    """[kept, exposed, left, 0] of a recentre by d of a volume whose boolean `evidence` [nz, ny, nx] says which voxels held any."""
    evidence = np.asarray(evidence, bool)
    inside = shifted(np.ones(evidence.shape, np.int8), d, 0).astype(bool)   # new voxels with a source
    kept_evidence = int(shifted(evidence.astype(np.int8), d, 0).sum())
    return [int(inside.sum()), int((~inside).sum()), int(evidence.sum()) - kept_evidence, 0]


def clip_box(dims, lo, hi):
    """(lo, hi) clipped to the grid (dims = nx, ny, nz), or None when nothing is left."""
    clo = [max(int(lo[a]), 0) for a in range(3)]
    chi = [min(int(hi[a]), dims[a] - 1) for a in range(3)]
    return (clo, chi) if all(clo[a] <= chi[a] for a in range(3)) else None


def mark(prm, L, pts, lo, hi, min_points, only_unknown, l_mark):
    """(L after lv_occ_mark, stats [4]) from L [nz, ny, nx] f32, caller points [n, 3], the box lo..hi and the parameters; prm: the
    dict of tests/occupancy_ref.py at the grid's CURRENT origin."""
    dims = (prm["nx"], prm["ny"], prm["nz"])
    L = np.array(L, F)
    box = clip_box(dims, lo, hi)
    if box is None:
        return L, [0, 0, 0, 0]
    (x0, y0, z0), (x1, y1, z1) = box
    pts = np.asarray(pts, F).reshape(-1, 3)
    ok, cell = gr.cell_of(prm["origin"], prm["resolution"], dims, False, pts)
    ok = ok & np.all((cell >= np.array([x0, y0, z0])) & (cell <= np.array([x1, y1, z1])), axis=1)
    count = np.zeros(L.shape, np.int64)
    np.add.at(count, (cell[ok, 2], cell[ok, 1], cell[ok, 0]), 1)
    candidate = count >= int(min_points)
    unknown = np.isnan(L)
    lm, lmin, lmax = F(l_mark), F(prm["l_min"]), F(prm["l_max"])
    with np.errstate(all="ignore"):
        if only_unknown:
            write = candidate & unknown
            L[write] = np.minimum(np.maximum(lm, lmin), lmax)
            left = candidate & ~unknown
        else:
            write = candidate
            base = np.where(unknown[write], F(0), L[write]).astype(F)
            L[write] = np.minimum(np.maximum((base + lm).astype(F), lmin), lmax)
            left = np.zeros(L.shape, bool)
    return L, [int(ok.sum()), int(candidate.sum()), int(write.sum()), int(left.sum())]


GRIDS = [(33, 5, 3), (1, 5, 1), (1, 1, 1), (70, 37, 9)]   # nx, ny, nz
ALIGNED_GRIDS = [(36, 5, 3), (72, 37, 9)]                 # nx % 4 == 0: the grids on which a shift with d_x % 4 == 0 loads 16 bytes


def shift_list(dims):
    """The shifts the tests run on a grid: per axis 0, +-1, +-(n - 1), +-n, +-(n + 5); 31 / 32 / 33 (and 4, a multiple of four) in x;
    and combinations of them over the axes.  On a grid with nx % 4 == 0 also d_x in 0, +-4, 8, +-32, +-(nx - 4), nx, -(nx + 4), each
    alone and with non-zero d_y and d_z."""
    out = [(0, 0, 0)]
    for a in range(3):
        n = dims[a]
        for v in (1, n - 1, n, n + 5):
            for sgn in (1, -1):
                d = [0, 0, 0]
                d[a] = sgn * v
                out.append(tuple(d))
    out += [(31, 0, 0), (32, 0, 0), (33, 0, 0), (-32, 0, 0), (4, 0, 0), (-4, 1, 0)]
    nx, ny, nz = dims
    out += [(1, 1, 1), (-1, -1, -1), (1, -1, 0), (nx - 1, -(ny - 1), nz - 1), (-(nx - 1), ny - 1, -(nz - 1)), (3, -2, 0), (-2, 0, 1),
            (nx, 1, 0), (1, ny + 5, -1), (0, -1, nz), (4, -2, 1)]
    if nx % 4 == 0:   # rows of whole 16-byte groups: with d_x % 4 == 0 the kernel's aligned path, which these hold to the rule
        for dx in (0, 4, -4, 8, 32, -32, nx - 4, -(nx - 4), nx, -(nx + 4)):
            out += [(dx, 1, -1), (dx, -2, 1), (dx, ny - 1, 0), (dx, 0, -(nz - 1)), (dx, 0, 0)]
    return list(dict.fromkeys(out))
