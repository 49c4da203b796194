"""The scene tests/test_surf_occ_ref.py, tests/test_surf_occ_host.py and tests/test_gpu_surf_occ.py share.  It is loaded with
lv_tsdf_load, so no integrator is involved: a volume of 70 x 21 x 9 voxels that holds a slanted wall and a ball, with weights
that leave every fourth voxel unknown, and three occupancy grids over it: the volume's own geometry, a coarser one that sticks out
on every side, and a finer one over the wall.  The wall's solid voxels span i = 28..35, across the 31 | 32 boundary of a bitmap
word; nx = 70 leaves a ragged last word.  tests/test_surf_occ_ref.py holds that every combination reaches every class."""
import numpy as np

import surf_occ_ref as sr

F = np.float32

NX, NY, NZ = 70, 21, 9
RES = 0.25
ORIGIN = (-1.0, -2.0, -0.5)
TRUNC_CELLS = 2
T = 256 * TRUNC_CELLS
MAX_WEIGHT = 10000

GRIDS = {
    "same": dict(origin=ORIGIN, resolution=RES, shape=(NZ, NY, NX)),
    "coarse": dict(origin=(-2.1, -2.9, -0.9), resolution=0.4, shape=(8, 17, 50)),
    "fine": dict(origin=(5.33, -1.05, 0.02), resolution=0.1, shape=(11, 33, 110)),
}
WEIGHT_BANDS = [(1, -64), (1, 0), (2, 128)]
REACHES = [0, 1, 3]
L_MIN, L_MAX = -2.0, 3.5   # lv_default_occupancy_params


def volume():
    """(S, W) int32 [NZ, NY, NX]"""
    k, j, i = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    x, y, z = i + 0.5, j + 0.5, k + 0.5
    wall = (34.0 - x - 0.3 * y) / np.sqrt(1.09)
    ball = np.sqrt((x - 8.0) ** 2 + (y - 10.0) ** 2 + (z - 4.0) ** 2) - 2.6
    s = np.rint(256.0 * np.minimum(wall, ball)).astype(np.int64)
    W = (7 * i + 3 * j + 5 * k) % 4
    W[W == 3] = 5
    W[s < -T] = 0
    s = np.clip(s, -T, T)
    return (s * W).astype(np.int32), W.astype(np.int32)


def vol_geometry(shift=(0, 0, 0)):
    return sr.geometry(sr.origin_at(ORIGIN, shift, RES), RES, (NZ, NY, NX))


def grid_geometry(name, shift=(0, 0, 0)):
    g = GRIDS[name]
    return sr.geometry(sr.origin_at(g["origin"], shift, g["resolution"]), g["resolution"], g["shape"])


def combinations():
    """the 27: (grid name, min_weight, band, reach)"""
    return [(n, mw, band, r) for n in GRIDS for mw, band in WEIGHT_BANDS for r in REACHES]


def random_grid(shape, seed):
    """[nz, ny, nx] f32: a third never observed, the rest spread over [L_MIN, L_MAX] with both clamps present"""
    rng = np.random.default_rng(seed)
    L = rng.uniform(L_MIN, L_MAX, shape).astype(F)
    pick = rng.integers(0, 6, shape)
    L[pick == 0] = F(L_MIN)
    L[pick == 1] = F(L_MAX)
    L[pick >= 4] = sr.NAN_BITS.view(F)
    return np.clip(L, F(L_MIN), F(L_MAX))
