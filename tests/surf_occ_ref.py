"""The rule of lv_occ_from_surface (include/limovelo_hip.h "Occupancy from the surface") in numpy, written from the header's text and
independent of the C++: the yardstick of tests/test_surf_occ_host.py (the rule functions of lv_surf_occ.hpp under g++) and of
tests/test_gpu_surf_occ.py (the kernels), both by equality on every bit of the grid and on all four stats.

One f32 step (the centre of an occupancy voxel and its quantisation in the volume, every operation a single float32 operation in
the order the header gives), integers after it.  Arrays are [nz, ny, nx]; a geometry is a dict(origin=[3], resolution, shape=(nz,
ny, nx)) at the volume's CURRENT origin (origin_at() gives that of a shifted volume)."""
import numpy as np

F = np.float32
NAN_BITS = np.uint32(0x7FC00000)
FILL, OVERWRITE, REPLACE, ACCUMULATE = 0, 1, 2, 3
NONE, FREE, OCCUPIED = 0, 1, 2


def origin_at(origin0, shift, resolution):
    """origin0 + (float)shift * resolution per axis, f32, unfused ("Rolling volumes")"""
    return [F(F(o) + F(F(s) * F(resolution))) for o, s in zip(origin0, shift)]


def geometry(origin, resolution, shape):
    return dict(origin=[F(v) for v in origin], resolution=F(resolution), shape=tuple(int(n) for n in shape))


def centres(origin, resolution, n):
    """[n] f32: origin + (((float)v + 0.5f) * resolution)"""
    v = np.arange(n).astype(F)
    return (F(origin) + ((v + F(0.5)) * F(resolution)).astype(F)).astype(F)


def quantise(p, origin, resolution):
    """occ_quant of "Occupancy grid": (ok, q) with q = floorf(((p - origin) / resolution) * 256) where |q| < 2^24"""
    with np.errstate(all="ignore"):
        f = np.floor((((p.astype(F) - F(origin)).astype(F) / F(resolution)).astype(F) * F(256)).astype(F))
        ok = np.abs(f) < F(16777216.0)
    return ok, np.where(ok, f, 0).astype(np.int64)


def voxel_of(grid, vol):
    """Per axis a (x, y, z order): (inside [n_a] bool, u [n_a] int64): the TSDF voxel index the occupancy voxels' centres fall into
    along that axis and whether it quantises and lies in the volume."""
    out = []
    for a in range(3):
        n_g, n_v = grid["shape"][2 - a], vol["shape"][2 - a]
        ok, q = quantise(centres(grid["origin"][a], grid["resolution"], n_g), vol["origin"][a], vol["resolution"])
        u = q >> 8
        out.append((ok & (u >= 0) & (u < n_v), u))
    return out


def voxel_classes(S, W, min_weight, band):
    """(solid, open) bool arrays of the volume"""
    S, W = np.asarray(S, np.int64), np.asarray(W, np.int64)
    known = W >= int(min_weight)
    solid = known & (S <= int(band) * W)
    return solid, known & ~solid


def dilate(solid, reach):
    """OR over the cube of Chebyshev radius reach, voxels outside the volume contributing nothing"""
    r = int(reach)
    out = solid.copy()
    if r == 0:
        return out
    nz, ny, nx = solid.shape
    pad = np.zeros((nz + 2 * r, ny + 2 * r, nx + 2 * r), bool)
    pad[r:r + nz, r:r + ny, r:r + nx] = solid
    for dk in range(2 * r + 1):
        for dj in range(2 * r + 1):
            for di in range(2 * r + 1):
                out |= pad[dk:dk + nz, dj:dj + ny, di:di + nx]
    return out


def classify(grid, vol, S, W, min_weight=1, band=0, reach=0):
    """(cls [nz, ny, nx] int8 of NONE / FREE / OCCUPIED, outside [nz, ny, nx] bool) of every voxel of the occupancy grid"""
    solid, opn = voxel_classes(S, W, min_weight, band)
    grown = dilate(solid, reach)
    (ix, ux), (iy, uy), (iz, uz) = voxel_of(grid, vol)
    inside = iz[:, None, None] & iy[None, :, None] & ix[None, None, :]
    kk = np.where(iz, uz, 0)[:, None, None]
    jj = np.where(iy, uy, 0)[None, :, None]
    ii = np.where(ix, ux, 0)[None, None, :]
    g, o = grown[kk, jj, ii] & inside, opn[kk, jj, ii] & inside
    cls = np.where(g, OCCUPIED, np.where(o, FREE, NONE)).astype(np.int8)
    return cls, ~inside


def clip_box(shape, lo, hi):
    """the inclusive box lo..hi (x, y, z) clipped to the grid as slices (z, y, x), or None when nothing is left"""
    sl = []
    for a in range(3):
        n = shape[2 - a]
        l, h = max(int(lo[a]), 0), min(int(hi[a]), n - 1)
        if l > h:
            return None
        sl.append(slice(l, h + 1))
    return (sl[2], sl[1], sl[0])


def update(L, delta, l_min, l_max):
    """occ_update: fminf(fmaxf((isnan(L) ? 0 : L) + delta, l_min), l_max) in f32"""
    base = np.where(np.isnan(L), F(0), L).astype(F)
    return np.minimum(np.maximum((base + F(delta)).astype(F), F(l_min)), F(l_max)).astype(F)


def from_surface(L, grid, vol, S, W, l_min=-2.0, l_max=3.5, lo=(0, 0, 0), hi=(1 << 30,) * 3, min_weight=1, band=0, reach=0, mode=FILL,
                 l_solid=3.5, l_open=-2.0):
    """(L' [nz, ny, nx] f32, stats [4] uint64) of one lv_occ_from_surface on the grid L; L itself is left unchanged"""
    L = np.asarray(L, F)
    out = L.copy()
    stats = np.zeros(4, np.uint64)
    box = clip_box(grid["shape"], lo, hi)
    if box is None:
        return out, stats
    cls, outside = classify(grid, vol, S, W, min_weight, band, reach)
    c, old = cls[box], L[box]
    a = np.minimum(np.maximum(F(l_solid), F(l_min)), F(l_max))
    b = np.minimum(np.maximum(F(l_open), F(l_min)), F(l_max))
    new = old.copy()
    occ, fre, non = c == OCCUPIED, c == FREE, c == NONE
    if mode == ACCUMULATE:
        new[occ] = update(old[occ], l_solid, l_min, l_max)
        new[fre] = update(old[fre], l_open, l_min, l_max)
    else:
        where = np.isnan(old) if mode == FILL else np.ones(old.shape, bool)
        new[occ & where] = a
        new[fre & where] = b
        if mode == REPLACE:
            new[non] = NAN_BITS.view(F)
    out[box] = new
    stats[:] = [occ.sum(), fre.sum(), (new.view(np.uint32) != old.view(np.uint32)).sum(), outside[box].sum()]
    return out, stats
