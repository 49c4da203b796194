"""The ray-cast occupancy grid on top of the lv_occ_* calls (include/limovelo_hip.h "Occupancy grid"): what OctoMap and
octomap_server's projected map hand to navigation.  integrate() takes any number of sweeps, occupancy_grid() gives the 2-D map in
the shape of nav_msgs/OccupancyGrid, save_grid / load_grid keep a grid as an .npz next to prelocalise.save_map's map, and
map_point_states() tells which points of the device map lie in space that the accumulated evidence says is free."""
from __future__ import annotations

import math

import numpy as np

from . import capi

MAX_VIEWS = 32   # views per lv_occ_integrate

_FIELDS = [f for f, _ in capi.OccupancyParams._fields_]


def integrate(ctx, views) -> np.ndarray:
    """lv_occ_integrate over views = [(R, t, points)] of any length, in chunks of 32 in order; the stats [4] uint64 summed."""
    stats = np.zeros(4, np.uint64)
    views = list(views)
    for c0 in range(0, len(views), MAX_VIEWS):
        stats += ctx.occ_integrate(views[c0:c0 + MAX_VIEWS])
    return stats


def layers(params, z_lo: float, z_hi: float):
    """(k_lo, k_hi): the layers whose voxel CENTRE origin_z + (k + 0.5) resolution lies in [z_lo, z_hi] (not clipped to the grid;
    k_lo > k_hi when there is none)."""
    oz, res = float(params.origin[2]), float(params.resolution)
    return int(math.ceil((z_lo - oz) / res - 0.5)), int(math.floor((z_hi - oz) / res - 0.5))


def occupancy_grid(ctx, z_lo: float, z_hi: float) -> dict:
    """The projection of the height band [z_lo, z_hi] shaped like nav_msgs/OccupancyGrid: resolution, width (cells along x), height
    (cells along y), origin (x, y, z of the low corner of cell (0, 0)) and data (int8 [height * width], row-major: 100 occupied, 0
    free, -1 unknown)."""
    p = ctx.occ_params()
    k_lo, k_hi = layers(p, z_lo, z_hi)
    if k_lo > k_hi:
        data = np.full(p.nx * p.ny, -1, np.int8)
    else:
        data = ctx.occ_project(k_lo, k_hi).reshape(-1)
    return dict(resolution=float(p.resolution), width=int(p.nx), height=int(p.ny),
                origin=(float(p.origin[0]), float(p.origin[1]), float(z_lo)), data=data)


def params_dict(p) -> dict:
    return {f: ([float(v) for v in p.origin] if f == "origin" else getattr(p, f)) for f in _FIELDS}


def save_grid(ctx, path: str):
    """The parameters and the log-odds ([nz, ny, nx] f32, NaN = never observed) as an .npz."""
    d = params_dict(ctx.occ_params())
    np.savez_compressed(path, logodds=ctx.occ_fetch(), **{"p_" + k: np.asarray(v) for k, v in d.items()})


def load_grid(ctx, path: str):
    """Configures ctx's grid from a file of save_grid and loads its log-odds; returns the parameters."""
    with np.load(path) as z:
        kw = {}
        for f, t in capi.OccupancyParams._fields_:
            v = z["p_" + f]
            kw[f] = [float(x) for x in v] if f == "origin" else (int(v) if t is capi.C.c_int else float(v))
        L = z["logodds"]
    p = capi.default_occupancy_params(**kw)
    ctx.occ_configure(p)
    ctx.occ_load(L)
    return p


def map_point_states(ctx) -> np.ndarray:
    """[map_size] f32: the log-odds of the voxel each point of the device map lies in (occ_query of map_fetch(); NaN outside the
    grid / never observed).  Values <= l_free mark map points in space the sweeps saw through."""
    m = ctx.map_fetch()
    if len(m) == 0:
        return np.zeros(0, np.float32)
    return ctx.occ_query(np.ascontiguousarray(m[:, :3], np.float32))
