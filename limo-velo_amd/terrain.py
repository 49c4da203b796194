"""The elevation map and the traversability of the ground on top of the lv_elev_* calls (include/limovelo_hip.h "Elevation map"):
what elevation_mapping / traversability_estimation, points2costmap and grid_map's terrain layer hand to a ground robot's planner.
params_from_metres() turns metres and degrees into the integer thresholds, like_occupancy() takes the geometry from the configured
occupancy grid, elevation() returns every layer, traversability() the int8 class grid (merged with the occupancy projection over
a height band if asked), distance_field() builds the planar distance field from such a grid (lv_occ_distance_build_cells), after
which occupancy.plan / routes / clearance work unchanged, and ground_points() puts goals and starts on the ground."""
from __future__ import annotations

import math

import numpy as np

from . import capi, occupancy

SUB = 256   # sub-units per cell


def sub_units(metres: float, resolution: float) -> int:
    """floor(metres / resolution * 256): a height threshold in the rule's integer sub-units.  In f32, as the grid's resolution is
    held: 1.5 m over 0.2 m cells is 1920 whether the 0.2 comes from Python or out of lv_occupancy_params."""
    F = np.float32
    return int(math.floor(F(metres) / F(resolution) * F(SUB)))


def slope2_of(max_slope_deg: float) -> int:
    """floor((512 tan slope)^2), at most 2^31 - 1: the rule's slope threshold."""
    if not 0.0 <= float(max_slope_deg) < 90.0:
        raise ValueError("max_slope_deg: 0 <= slope < 90")
    return int(min(math.floor((2 * SUB * math.tan(math.radians(float(max_slope_deg)))) ** 2), 2 ** 31 - 1))


def params_from_metres(origin=(-51.2, -51.2, -3.2), resolution=0.2, nx=512, ny=512, robot_height=1.5, max_step=0.10, max_span=0.12,
                       max_slope_deg=20.0, min_points=3) -> capi.ElevationParams:
    """lv_elevation_params from a grid (origin of its low corner and of the height scale, cell size, cells) and the robot: what
    hangs more than robot_height above a cell's lowest point is ignored; a cell is lethal when its body band is taller than
    max_span, when its ground differs from a neighbour's by more than max_step, or when the ground is steeper than max_slope_deg."""
    return capi.default_elevation_params(origin=[float(v) for v in origin], resolution=float(resolution), nx=int(nx), ny=int(ny),
                                         min_points=int(min_points), head=sub_units(robot_height, resolution),
                                         max_span=sub_units(max_span, resolution), max_step=sub_units(max_step, resolution),
                                         max_slope2=slope2_of(max_slope_deg))


def like_occupancy(ctx, **kw) -> capi.ElevationParams:
    """params_from_metres over the footprint of ctx's configured occupancy grid (its origin, resolution, nx and ny)."""
    p = ctx.occ_params()
    return params_from_metres(origin=[float(v) for v in p.origin], resolution=float(p.resolution), nx=int(p.nx), ny=int(p.ny), **kw)


def elevation(ctx, params=None, points=None) -> dict:
    """Builds the elevation map (points [n, 3]; None: the living points of the device map) and returns every layer as a [ny, nx]
    array under its name in capi.ELEV_LAYERS (lo, top, span, step, slope2, count, band_count, cls, height), plus `stats`
    (uint64 [4]: points used, overhang points, known cells, lethal cells) and `params`."""
    p = params if params is not None else capi.default_elevation_params()
    stats = ctx.elev_build(p, points)
    out = {name: ctx.elev_fetch(layer) for layer, (name, _) in enumerate(capi.ELEV_LAYERS)}
    out["stats"] = stats
    out["params"] = p
    return out


def traversability(ctx, params=None, points=None, z_band=None) -> np.ndarray:
    """Builds the elevation map and returns its class grid, int8 [ny, nx]: 100 lethal, 0 free, -1 unknown.  With z_band = (z_lo, z_hi)
    it is merged with the occupancy grid's projection over that height band (occupancy.layers; the elevation grid must have the
    occupancy grid's nx and ny): lethal where either is lethal, the terrain class elsewhere."""
    p = params if params is not None else capi.default_elevation_params()
    ctx.elev_build(p, points)
    cls = ctx.elev_fetch(capi.LV_ELEV_CLASS)
    if z_band is not None:
        o = ctx.occ_params()
        if (o.nx, o.ny) != (p.nx, p.ny):
            raise ValueError("traversability: z_band needs an elevation grid of the occupancy grid's nx and ny")
        k_lo, k_hi = occupancy.layers(o, float(z_band[0]), float(z_band[1]))
        if k_lo <= k_hi:
            cls = np.where(ctx.occ_project(k_lo, k_hi) == 100, np.int8(100), cls).astype(np.int8)
    return cls


def distance_field(ctx, cells, max_dist=None, signed=False, unknown="free") -> np.ndarray:
    """occupancy.distance_field over a class grid instead of the projected occupancy: builds the planar distance field from cells
    (int8 [ny, nx] of the configured occupancy grid: 100 an obstacle, negative unknown) and returns it in metres, [ny, nx] f32.
    max_dist, signed and unknown ("free" or "obstacle") as there.  occupancy.plan / routes / clearance then run on it."""
    if unknown not in ("free", "obstacle"):
        raise ValueError('unknown: "free" or "obstacle"')
    p = ctx.occ_params()
    kw = dict(planar=1, signed_field=int(bool(signed)), unknown_is_obstacle=int(unknown == "obstacle"))
    if max_dist is not None:
        n = int(math.floor(float(max_dist) / float(p.resolution)))
        if n < 1:
            raise ValueError("max_dist: at least one cell")
        kw["max_cells"] = min(n, 1024)
    ctx.occ_distance_build_cells(cells, capi.default_distance_params(**kw))
    return ctx.occ_distance_fetch(s2=False)[1]


def ground_points(ctx, xy) -> np.ndarray:
    """[n, 3] f32: the points xy ([n, 2], or [n, 3] whose z is ignored) with z set to the ground height of their cell in the
    elevation map last built (NaN outside the grid and in cells that are not known)."""
    a = np.atleast_2d(np.asarray(xy, np.float32))
    pts = np.zeros((len(a), 3), np.float32)
    pts[:, :2] = a[:, :2]
    pts[:, 2] = ctx.elev_query(pts)[0]
    return pts
