"""Place recognition for global relocalisation without a pose prior (include/limovelo_hip.h "Place recognition"): where in a saved
map am I?  The context's place database (keyframe scans, lv_place_add_scan, or virtual places built from the map, lv_place_add_map)
returns the places whose Scan Context descriptor is nearest to the current scan's, with the yaw shift that aligns them.  Each hit
seeds a small grid of candidate states that lv_update_batch refines against the map, as prelocalise.prelocalise does around a prior.

Restarting inside a saved map: prelocalise.load_map + load_places + lv_scan_set + global_localise, then lv_filter_set with the
returned state."""
from __future__ import annotations

import math

import numpy as np

from . import prelocalise
from .synth import quat_from_rpy, quat_mul, quat_to_rot


def map_grid_centres(map_xyz, spacing: float, sensor_height: float) -> np.ndarray:
    """[n, 3] f64 place centres on a grid of step `spacing` over the map's xy extent (cell centres, the first half a step in from
    the smallest x and y).  A centre's z is the smallest map z within +-0.5 m of it in x and y, plus sensor_height; grid points
    with no map point that close are skipped."""
    p = np.asarray(map_xyz, np.float64).reshape(-1, 3)
    lo, hi = p[:, :2].min(0), p[:, :2].max(0)
    n = np.maximum(1, np.ceil((hi - lo) / spacing).astype(np.int64))
    g = np.floor((p[:, :2] - lo) / spacing).astype(np.int64)
    g = np.minimum(np.maximum(g, 0), n - 1)
    gc = lo + (g + 0.5) * spacing
    near = np.all(np.abs(p[:, :2] - gc) <= 0.5, axis=1)
    cell = g[near, 1] * n[0] + g[near, 0]
    zmin = np.full(int(n[0] * n[1]), np.inf)
    np.minimum.at(zmin, cell, p[near, 2])
    have = np.nonzero(np.isfinite(zmin))[0]
    iy, ix = np.divmod(have, n[0])
    return np.stack([lo[0] + (ix + 0.5) * spacing, lo[1] + (iy + 0.5) * spacing, zmin[have] + sensor_height], axis=1)


def hit_state(x_query, centre, shift: int, n_sectors: int) -> np.ndarray:
    """The candidate state of one retrieved place: rotation Rz(yaw) R_x with yaw = shift * 2 pi / n_sectors wrapped to (-pi, pi],
    position centre - Rz(yaw) R_x t_off; everything else from x_query."""
    x = np.asarray(x_query, np.float64).reshape(26).copy()
    a = shift * 2.0 * math.pi / n_sectors
    yaw = math.atan2(math.sin(a), math.cos(a))
    if yaw <= -math.pi:
        yaw = math.pi
    q = quat_mul(quat_from_rpy(0.0, 0.0, yaw), x[3:7])
    x[3:7] = q
    x[0:3] = np.asarray(centre, np.float64) - quat_to_rot(q) @ x[11:14]
    return x


def candidates(x_query, ids, shifts, centres, n_sectors: int, *, xy_radius: float = 2.0, xy_step: float = 0.5,
               yaw_span: float | None = None, yaw_step: float | None = None):
    """(states [m, 26], hit [m]): prelocalise.candidate_grid around the state of every hit (hit_state), yaw_span one sector and
    yaw_step half a sector by default; hit[i] = the index into ids of the hit row i grew from."""
    sector = 2.0 * math.pi / n_sectors
    yaw_span = sector if yaw_span is None else yaw_span
    yaw_step = sector / 2 if yaw_step is None else yaw_step
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    out, hit = [], []
    for h, (i, s) in enumerate(zip(ids, shifts)):
        g = prelocalise.candidate_grid(hit_state(x_query, centres[int(i)], int(s), n_sectors), xy_radius, xy_step, yaw_span, yaw_step)
        out.append(g)
        hit.append(np.full(len(g), h, np.int64))
    return np.concatenate(out), np.concatenate(hit)


def global_localise(ctx, x_level, P, k: int = 8, rounds: int = 2, keep: int = 8, **grid):
    """Where is the current scan in the context's map?  x_level: a state whose roll, pitch and extrinsics are the scan's (its
    position and yaw are ignored).  The k nearest places (lv_place_query) seed candidates(..., **grid); lv_update_batch refines
    them, the best `keep` are refined `rounds` more times and ranked by prelocalise.rank.  Returns (best state [26], table): the
    final round best first, dicts {state, passes, n_valid, sum_h2, place, shift, place_dist}."""
    ids, shifts, dist = ctx.place_query(x_level, k)
    n_sectors = int(ctx.place_params().n_sectors)
    xs, hit = candidates(x_level, ids, shifts, ctx.place_centres(), n_sectors, **grid)
    table, origin = prelocalise.refine(ctx, xs, P, rounds, keep)
    for row, o in zip(table, origin):
        h = int(hit[o])
        row.update(place=int(ids[h]), shift=int(shifts[h]), place_dist=float(dist[h]))
    return table[0]["state"].copy(), table


def save_places(ctx, path) -> None:
    """The context's place database to an .npz: params (n_rings, n_sectors, rmin, rmax, z_offset), desc [n, n_rings, n_sectors]
    f32 and centres [n, 3] f64.  Goes beside prelocalise.save_map."""
    p = ctx.place_params()
    desc, centres = ctx.place_fetch()
    np.savez(path, params=np.array([p.n_rings, p.n_sectors, p.rmin, p.rmax, p.z_offset], np.float64), desc=desc, centres=centres)


def load_places(ctx, path) -> None:
    """A database saved by save_places: lv_place_configure with its parameters (which clears the context's database), then
    lv_place_load of its places (ids as saved)."""
    from .capi import default_place_params

    with np.load(path) as z:
        prm, desc, centres = z["params"], z["desc"], z["centres"]
    ctx.place_configure(default_place_params(n_rings=int(prm[0]), n_sectors=int(prm[1]), rmin=float(prm[2]), rmax=float(prm[3]),
                                             z_offset=float(prm[4])))
    if len(centres):
        ctx.place_load(desc, centres)
