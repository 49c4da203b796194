"""The ray-cast occupancy grid on top of the lv_occ_* calls (include/limovelo_hip.h "Occupancy grid"): what OctoMap and
octomap_server's projected map hand to navigation.  integrate() takes any number of sweeps, occupancy_grid() gives the 2-D map in
the shape of nav_msgs/OccupancyGrid, save_grid / load_grid keep a grid as an .npz next to prelocalise.save_map's map, and
map_point_states() tells which points of the device map lie in space that the accumulated evidence says is free.
distance_field() / clearance() give the Euclidean distance to the nearest obstacle (lv_occ_distance_*, "Distance field") and
costmap_from_distance() costmap_2d's inflation costs from it.  plan() / routes() build the cost-to-go to a set of goals over that
field and walk routes down it (lv_occ_plan_*, "Planner": navfn / global_planner), with inflation_cost_table() and min_clear_s2()
turning costmap_2d's parameters into the planner's integer ones.  frontiers() labels the boundary between free and unknown space into
clusters (lv_occ_frontier_*, "Frontiers": explore_lite / frontier_exploration) and explore() ranks them by the planner's cost from
the robot and hands back targets with their routes.  raycast() / line_of_sight() / simulate_scan() ask what a sensor would see
from a place and view_gain() how much unknown space a pose would uncover (lv_occ_raycast, lv_occ_view_gain, "Ray casting"); with a
gain_pattern explore() reports that gain at every target.  recentre() / follow() move the grid's box with the robot by whole
voxels (lv_volume_recentre, "Rolling volumes"), exposed_boxes() names the strips a shift uncovered and mark_from_map() fills them
from the device map's points (lv_occ_mark).  from_surface() fills the grid from the TSDF volume (lv_occ_from_surface, "Occupancy
from the surface") and surface_costmap() projects the result: the costmap of a robot that fuses depth images."""
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


def distance_field(ctx, max_dist=None, signed=False, unknown="free", z_band=None) -> np.ndarray:
    """Builds the distance field of ctx's grid and returns it in metres: [nz, ny, nx] f32, or [ny, nx] over the height band
    z_band = (z_lo, z_hi) (the layers of layers(); a band without a layer gives a field without obstacles).  max_dist (metres)
    truncates at floor(max_dist / resolution) cells: farther values are +-inf.  signed: negative inside obstacles.  unknown:
    "free" or "obstacle"."""
    if unknown not in ("free", "obstacle"):
        raise ValueError('unknown: "free" or "obstacle"')
    p = ctx.occ_params()
    kw = dict(signed_field=int(bool(signed)), unknown_is_obstacle=int(unknown == "obstacle"))
    if max_dist is not None:
        cells = int(math.floor(float(max_dist) / float(p.resolution)))
        if cells < 1:
            raise ValueError("max_dist: at least one voxel")
        kw["max_cells"] = min(cells, 1024)
    if z_band is not None:
        k_lo, k_hi = layers(p, float(z_band[0]), float(z_band[1]))
        if k_lo > k_hi:
            k_lo, k_hi = p.nz, p.nz   # (clipped to nothing: every cell unknown)
        kw.update(planar=1, k_lo=k_lo, k_hi=k_hi)
    ctx.occ_distance_build(capi.default_distance_params(**kw))
    return ctx.occ_distance_fetch(s2=False)[1]


def clearance(ctx, pts):
    """(dist [n] f32, grad [n, 3] f32): the distance in metres from each world point's voxel to the nearest obstacle in the field
    last built, and its gradient (central differences over the neighbouring voxels; points away from the obstacles)."""
    return ctx.occ_distance_query(pts, want_grad=True)


def costmap_from_distance(dist_m, inscribed_radius: float, inflation_radius: float, cost_scaling_factor: float = 10.0) -> np.ndarray:
    """costmap_2d's inflation costs (uint8) from distances in metres: 254 (lethal) at distance 0, 253 (inscribed) up to
    inscribed_radius, (253 - 1) * exp(-cost_scaling_factor * (d - inscribed_radius)) truncated to an integer out to
    inflation_radius, 0 beyond (and where the distance is inf or NaN).  Negative distances (inside obstacles) are lethal."""
    d = np.asarray(dist_m, np.float64)
    cost = np.zeros(d.shape, np.uint8)
    with np.errstate(all="ignore"):
        mid = (d > inscribed_radius) & (d <= inflation_radius)
        cost[mid] = ((253 - 1) * np.exp(-cost_scaling_factor * (d[mid] - inscribed_radius))).astype(np.uint8)
        cost[(d > 0) & (d <= inscribed_radius)] = 253
        cost[d <= 0] = 254
    return cost


def inflation_cost_table(resolution: float, inscribed_radius: float, inflation_radius: float, cost_scaling_factor: float = 10.0,
                         neutral: int = 50) -> np.ndarray:
    """The planner's cost table (uint8) from costmap_2d's inflation law: entry t is costmap_from_distance at t whole cells
    (t * resolution metres) plus `neutral` (navfn's cost of a free cell), clamped to 1..255.  It runs to the first whole-cell
    distance beyond inflation_radius, whose cost every farther cell shares (at most 1025 entries)."""
    n = min(int(math.floor(float(inflation_radius) / float(resolution))) + 2, 1025) if inflation_radius > 0 else 2
    d = np.arange(max(n, 1), dtype=np.float64) * float(resolution)
    c = costmap_from_distance(d, inscribed_radius, inflation_radius, cost_scaling_factor).astype(np.int64) + int(neutral)
    return np.clip(c, 1, 255).astype(np.uint8)


def min_clear_s2(resolution: float, radius: float) -> int:
    """The smallest integer s2 (>= 1) whose metre value resolution * sqrtf(s2), in f32 as the distance field computes it, is at
    least radius: a cell is traversable iff its clearance reaches radius (and it is no obstacle)."""
    F = np.float32
    limit = 3 * 1023 * 1023
    s = min(max(int(math.ceil((float(radius) / float(resolution)) ** 2)), 1), limit)

    def metres(v):
        return float(F(resolution) * np.sqrt(F(v)))

    while s > 1 and metres(s - 1) >= radius:
        s -= 1
    while s < limit and metres(s) < radius:
        s += 1
    return s


def plan(ctx, goals, robot_radius: float, inflation_radius: float | None = None, cost_scaling_factor: float = 10.0, neutral: int = 50,
         connectivity: int | None = None):
    """Builds the cost-to-go to `goals` ([n, 3] world points) over the distance field last built (distance_field() or
    ctx.occ_distance_build) and returns (info, stats): lv_plan_info, and goals used, traversable cells, reached cells, the
    largest finite potential.  Cells whose clearance is below robot_radius are blocked; the others cost what costmap_2d's
    inflation law gives out to inflation_radius (default: 3 robot radii) plus `neutral`.  connectivity: default 8 on a planar
    field, 26 on a 3-D one."""
    res = float(ctx.occ_params().resolution)
    if inflation_radius is None:
        inflation_radius = 3.0 * robot_radius
    if connectivity is None:
        connectivity = 8 if ctx.occ_distance_info().planar else 26
    table = inflation_cost_table(res, robot_radius, inflation_radius, cost_scaling_factor, neutral)
    prm = capi.default_plan_params(connectivity=int(connectivity), min_clear_s2=min_clear_s2(res, robot_radius))
    stats = ctx.occ_plan_build(goals, table, prm)
    return ctx.occ_plan_info(), stats


def routes(ctx, starts):
    """Per start point (polyline, status, cost): the centres of the path's cells in world coordinates, [n, 3] f32 ([n, 2] in a planar
    plan; empty unless status is 0), the status (0 a route, 1 no route from there, 2 the start is blocked or outside) and the
    route's cost (the potential of the start cell, capi.LV_PLAN_UNREACHED without a route)."""
    status, cost, off, cells = ctx.occ_plan_paths(starts)
    i = ctx.occ_plan_info()
    p = ctx.occ_params()
    res = np.float64(p.resolution)
    c = cells.astype(np.int64)
    idx = [c % i.nx, (c // i.nx) % i.ny] + ([] if i.planar else [c // (i.nx * i.ny)])
    xyz = np.stack([np.float64(p.origin[a]) + (v + 0.5) * res for a, v in enumerate(idx)], axis=1).astype(np.float32)
    return [(xyz[int(off[s]):int(off[s + 1])], int(status[s]), int(cost[s])) for s in range(len(status))]


def _cell_centres(p, info, cells) -> np.ndarray:
    """[n, 3] f32 world coordinates of the centres of linear cell indices of a result with info's nx, ny (a planar result's z is
    the grid's origin z)."""
    c = np.asarray(cells).astype(np.int64)
    return _ijk_centres(p, info, np.stack([c % info.nx, (c // info.nx) % info.ny, c // (info.nx * info.ny)], axis=1))


def _ijk_centres(p, info, ijk) -> np.ndarray:
    res = np.float64(p.resolution)
    xyz = np.array([float(v) for v in p.origin]) + (np.asarray(ijk, np.float64).reshape(-1, 3) + 0.5) * res
    if info.planar:
        xyz[:, 2] = float(p.origin[2])
    return xyz.astype(np.float32)


def _band(p, z_band):
    if z_band is None:
        return {}
    k_lo, k_hi = layers(p, float(z_band[0]), float(z_band[1]))
    if k_lo > k_hi:
        k_lo, k_hi = p.nz, p.nz   # (clipped to nothing: every cell unknown)
    return dict(planar=1, k_lo=k_lo, k_hi=k_hi)


def frontiers(ctx, z_band=None, connectivity=None, min_size=1):
    """Builds the frontier clusters of ctx's grid and returns (labels, clusters).  labels: int32 [nz, ny, nx], or [ny, nx] over the
    height band z_band = (z_lo, z_hi) (the layers of layers()): the cluster's number on its members, -1 elsewhere.  clusters: a
    structured array in label order (largest first) with the fields of lv_frontier_cluster plus rep_xyz and centre_xyz, the world
    coordinates of the centres of those cells.  connectivity: default 8 planar, 26 in 3-D; components below min_size are dropped."""
    p = ctx.occ_params()
    kw = _band(p, z_band)
    kw["connectivity"] = int(connectivity) if connectivity is not None else (8 if kw else 26)
    ctx.occ_frontier_build(capi.default_frontier_params(min_size=int(min_size), **kw))
    return ctx.occ_frontier_fetch(), _with_world(p, ctx.occ_frontier_info(), ctx.occ_frontier_clusters())


def _with_world(p, info, cl, extra=()):
    out = np.zeros(len(cl), np.dtype(capi.FRONTIER_CLUSTER_DTYPE.descr + [("rep_xyz", np.float32, 3), ("centre_xyz", np.float32, 3)] + list(extra)))
    for f in capi.FRONTIER_CLUSTER_DTYPE.names:
        out[f] = cl[f]
    out["rep_xyz"] = _cell_centres(p, info, cl["rep"])
    out["centre_xyz"] = _ijk_centres(p, info, cl["centre"])
    return out


def _sub_units(p, pts) -> np.ndarray:
    """[n, 3] int64: world points quantised as the device does, floorf(((p - origin) / resolution) * 256) in f32 in that order (a
    sensor origin and a return's world point differ in their limits only).  Meaningful for rays that were not ignored."""
    F = np.float32
    with np.errstate(all="ignore"):
        q = np.floor(((np.asarray(pts, F).reshape(-1, 3) - np.array([v for v in p.origin], F)) / F(p.resolution)) * F(256))
    return np.where(np.abs(q) < 2.0 ** 24, q, 0).astype(np.int64)


def raycast(ctx, frm, to, stop_unknown=False):
    """lv_occ_raycast of the rays frm[i] -> to[i] ([n, 3] world points): (results, range_m).  results: the structured array of
    capi.RAY_RESULT_DTYPE (status capi.LV_RAY_IGNORED / CLEAR / STOPPED, the cell that stopped the ray, steps, the axis and the
    fraction num / den at which it was entered, the free and unknown cells passed before).  range_m [n] f64: the distance in
    metres from frm to where a STOPPED ray enters its cell, resolution / 256 * |qe - qs| * num / den over the quantised ends;
    inf for CLEAR rays, NaN for IGNORED ones.  stop_unknown: unknown cells stop a ray as occupied ones do."""
    frm = np.asarray(frm, np.float32).reshape(-1, 3)
    to = np.asarray(to, np.float32).reshape(-1, 3)
    res = ctx.occ_raycast(frm, to, capi.default_ray_params(stop_unknown=int(bool(stop_unknown))))
    p = ctx.occ_params()
    d = (_sub_units(p, to) - _sub_units(p, frm)).astype(np.float64)
    length = np.sqrt((d ** 2).sum(axis=1))
    rng = np.full(len(res), np.nan)
    rng[res["status"] == capi.LV_RAY_CLEAR] = np.inf
    h = res["status"] == capi.LV_RAY_STOPPED
    rng[h] = np.float64(p.resolution) / 256.0 * length[h] * res["num"][h] / res["den"][h]
    return res, rng


def line_of_sight(ctx, a, b) -> np.ndarray:
    """[n] bool: no occupied voxel lies on the segment a[i] -> b[i] (false for rays lv_occ_raycast ignores)."""
    return ctx.occ_raycast(a, b)["status"] == capi.LV_RAY_CLEAR


def scan_pattern(n_az: int, n_el: int, el_lo: float, el_hi: float, max_range: float) -> np.ndarray:
    """[n_el * n_az, 3] f32: the end points, in the sensor frame, of a spinning LiDAR's beams of length max_range: n_az azimuths
    2 pi a / n_az, n_el elevations from el_lo to el_hi (radians, inclusive), elevation-major."""
    az = 2.0 * np.pi * np.arange(int(n_az)) / int(n_az)
    el = np.linspace(float(el_lo), float(el_hi), int(n_el))
    e, a = np.meshgrid(el, az, indexing="ij")
    return (float(max_range) * np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1)).reshape(-1, 3).astype(np.float32)


def simulate_scan(ctx, R, t, pattern) -> np.ndarray:
    """[n] f64 ranges in metres (raycast's range_m) of the beams of `pattern` (sensor frame) from the pose (R, t): inf where a
    beam meets no occupied voxel before its end."""
    R = np.asarray(R, np.float32).reshape(3, 3)
    t = np.asarray(t, np.float32).reshape(3)
    to = (np.asarray(pattern, np.float32).reshape(-1, 3) @ R.T + t).astype(np.float32)
    return raycast(ctx, np.broadcast_to(t, to.shape), to)[1]


def view_gain(ctx, positions, pattern, yaws=None) -> np.ndarray:
    """lv_occ_view_gain of `pattern` (scan_pattern) at each of positions [n, 3], turned about z by yaws [n] (default 0), 32 views
    per call: [n, 4] uint64 — rays used, rays stopped, distinct unknown voxels seen, distinct free voxels seen."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    yaws = np.zeros(len(pos)) if yaws is None else np.asarray(yaws, np.float64).reshape(-1)
    views = [(np.array([[math.cos(y), -math.sin(y), 0.0], [math.sin(y), math.cos(y), 0.0], [0.0, 0.0, 1.0]], np.float32), t, pattern)
             for t, y in zip(pos, yaws)]
    out = np.zeros((len(views), 4), np.uint64)
    for c0 in range(0, len(views), MAX_VIEWS):
        out[c0:c0 + MAX_VIEWS] = ctx.occ_view_gain(views[c0:c0 + MAX_VIEWS])
    return out


def explore(ctx, robot_xyz, robot_radius: float, z_band=None, reach=None, min_size=1, unknown="obstacle", gain_pattern=None):
    """Where to drive next: builds the distance field (3-D, or planar over z_band; unknown space counts as an obstacle unless
    unknown="free"), a plan whose only goal is the robot (the planner's edges are symmetric: it holds the cost from the robot to
    every cell), the frontier clusters, and ranks them (reach: cells round a member in which a reachable cell is looked for;
    default ceil(robot_radius / resolution), at most 8).  Returns (clusters, routes): the clusters of frontiers() ordered by
    best_p, the cheapest first and the unreachable ones last, with their label, best_p, best_cell and target_xyz (the centre of
    best_cell; NaN without one); and per cluster the polyline from the robot's cell to the target (empty without a route).
    gain_pattern (scan_pattern): the clusters also get gain_unknown and gain_free, view_gain() of that pattern at target_xyz (0
    without a target); the order stays by best_p, weighing cost against gain is the caller's."""
    if unknown not in ("free", "obstacle"):
        raise ValueError('unknown: "free" or "obstacle"')
    p = ctx.occ_params()
    band = _band(p, z_band)
    if reach is None:
        reach = min(int(math.ceil(float(robot_radius) / float(p.resolution))), 8)
    ctx.occ_distance_build(capi.default_distance_params(unknown_is_obstacle=int(unknown == "obstacle"), **band))
    plan(ctx, np.asarray(robot_xyz, np.float32).reshape(1, 3), robot_radius)
    ctx.occ_frontier_build(capi.default_frontier_params(connectivity=8 if band else 26, min_size=int(min_size), **band))
    info = ctx.occ_frontier_info()
    best_p, best_cell = ctx.occ_frontier_rank(int(reach))
    order = np.lexsort((np.arange(len(best_p)), best_p))
    cl = _with_world(p, info, ctx.occ_frontier_clusters()[order],
                     extra=[("label", np.int32), ("best_p", np.uint32), ("best_cell", np.int32), ("target_xyz", np.float32, 3)] +
                     ([("gain_unknown", np.uint64), ("gain_free", np.uint64)] if gain_pattern is not None else []))
    cl["label"], cl["best_p"], cl["best_cell"] = order, best_p[order], best_cell[order]
    ok = cl["best_cell"] >= 0
    cl["target_xyz"] = np.nan
    cl["target_xyz"][ok] = _cell_centres(p, info, cl["best_cell"][ok])
    lines = [np.zeros((0, 2 if info.planar else 3), np.float32)] * len(cl)
    if gain_pattern is not None and ok.any():
        gain = view_gain(ctx, cl["target_xyz"][ok], gain_pattern)
        cl["gain_unknown"][ok], cl["gain_free"][ok] = gain[:, 2], gain[:, 3]
    if ok.any():
        for c, (line, _, _) in zip(np.flatnonzero(ok), routes(ctx, cl["target_xyz"][ok])):
            lines[c] = line[::-1]   # (walked from the target down to the robot: reversed)
    return cl, lines


def recentre(ctx, shift) -> np.ndarray:
    """lv_volume_recentre of the grid by shift (3 whole voxels): the box moves, the contents stay where they are in the world.
    Returns stats [4] uint64: voxels kept, exposed (now never observed), that held evidence and left the grid, 0."""
    return ctx.volume_recentre(capi.LV_VOLUME_OCC, shift)


def follow_shift(params, position, keep=0.25, step=32, axes=(True, True, False)):
    """The shift follow() would apply to a volume with `params` (origin, resolution, nx, ny, nz) for a robot at `position`: per
    followed axis, 0 while the position's voxel is within keep * n voxels of the centre voxel n // 2, otherwise the multiple of
    `step` nearest to that offset (halves away from zero are rounded up), within the +-2^20 of one recentre."""
    F = np.float32
    if int(step) < 1:
        raise ValueError("step: at least one voxel")
    n = (int(params.nx), int(params.ny), int(params.nz))
    out = [0, 0, 0]
    for a in range(3):
        if not axes[a]:
            continue
        with np.errstate(all="ignore"):
            v = np.floor((F(position[a]) - F(params.origin[a])) / F(params.resolution))   # (f32, as the device quantises)
        if not np.isfinite(v):
            raise ValueError("follow: the position is not finite")
        off = int(v) - n[a] // 2
        if abs(off) > float(keep) * n[a]:
            d = int(step) * int(math.floor(off / int(step) + 0.5))
            out[a] = max(-capi.VOLUME_SHIFT_LIMIT, min(capi.VOLUME_SHIFT_LIMIT, d))
    return tuple(out)


def follow(ctx, position, keep=0.25, step=32, axes=(True, True, False)):
    """Keeps the grid round the robot: when the voxel of `position` is more than keep * n voxels from the grid's centre on a
    followed axis (default x and y), the grid is recentred along that axis by the multiple of `step` voxels that brings the
    position nearest the centre.  Returns the shift applied, (0, 0, 0) when the grid stayed.  The strip it exposed
    (exposed_boxes()) can be filled from the point map (mark_from_map()) or from the TSDF surface (from_surface())."""
    d = follow_shift(ctx.occ_params(), position, keep, step, axes)
    if any(d):
        recentre(ctx, d)
    return d


def exposed_boxes(params, shift):
    """The voxels a recentre by `shift` left never observed, as up to three disjoint inclusive voxel boxes [(lo, hi)] of the
    SHIFTED grid, in the form lv_occ_mark takes: the strip across x, the strip across y of what x kept, the strip across z of
    what x and y kept.  (A shift of a whole grid or more gives the whole grid as one box.)  from_surface() takes the same boxes:
    the exposed voxels can be filled from the TSDF surface as well as by mark_from_map()."""
    n = (int(params.nx), int(params.ny), int(params.nz))
    kept, gone = [], []
    for a in range(3):
        d = max(-n[a], min(n[a], int(shift[a])))
        kept.append((0, n[a] - d - 1) if d >= 0 else (-d, n[a] - 1))
        gone.append((n[a] - d, n[a] - 1) if d > 0 else (0, -d - 1))   # (d == 0: 0..-1, empty)
    full = [(0, n[a] - 1) for a in range(3)]
    boxes = []
    for a in range(3):
        ranges = [kept[b] if b < a else (gone[b] if b == a else full[b]) for b in range(3)]
        if all(lo <= hi for lo, hi in ranges):
            boxes.append((tuple(r[0] for r in ranges), tuple(r[1] for r in ranges)))
    return boxes


def mark_from_map(ctx, box=None, min_points=1, only_unknown=True, l_mark=None) -> np.ndarray:
    """lv_occ_mark from the living points of the device map: a voxel of `box` = (lo, hi) (inclusive voxel indices, default the
    whole grid) that holds at least min_points of them becomes occupied by l_mark (default 0.85; negative marks free space).
    only_unknown: only never observed voxels are written, ray evidence stays.  Returns stats [4] uint64: points used, voxels
    holding >= min_points, voxels marked, voxels left alone because they were observed."""
    kw = dict(min_points=int(min_points), only_unknown=int(bool(only_unknown)))
    if box is not None:
        kw.update(lo=box[0], hi=box[1])
    if l_mark is not None:
        kw["l_mark"] = float(l_mark)
    return ctx.occ_mark(capi.default_occ_mark_params(**kw))


def from_surface(ctx, mode=capi.LV_OCC_SURFACE_FILL, box=None, **kw) -> np.ndarray:
    """lv_occ_from_surface ("Occupancy from the surface"): the voxels of `box` = (lo, hi) (inclusive voxel indices, default the
    whole grid) take what the TSDF volume says of their centres: OCCUPIED where a solid TSDF voxel lies within `reach` voxels,
    FREE where their own TSDF voxel is known and open, nothing otherwise.  mode: capi.LV_OCC_SURFACE_FILL writes only never
    observed voxels (ray evidence stays), _OVERWRITE every classed voxel, _REPLACE also forgets the voxels the volume knows nothing
    of, _ACCUMULATE adds l_solid / l_open to what the voxel holds.  kw: min_weight, band, reach, l_solid, l_open.  Returns stats
    [4] uint64: voxels classed OCCUPIED, classed FREE, voxels changed, voxels outside the volume."""
    kw = dict(kw, mode=int(mode))
    if box is not None:
        kw.update(lo=box[0], hi=box[1])
    return ctx.occ_from_surface(capi.default_occ_surface_params(**kw))


def surface_costmap(ctx, k_lo: int, k_hi: int, **kw) -> np.ndarray:
    """The costmap of a robot that fuses depth images: the whole grid becomes a pure function of the TSDF volume (from_surface in
    mode REPLACE; kw as there), then lv_occ_project over the layers k_lo..k_hi: [ny, nx] int8, 100 occupied, 0 free, -1 unknown."""
    from_surface(ctx, capi.LV_OCC_SURFACE_REPLACE, None, **kw)
    return ctx.occ_project(k_lo, k_hi)
