"""Euclidean clustering of the device map and removal by cluster (include/limovelo_hip.h "Map clustering"): thin helpers over
Context.map_cluster / Context.map_remove_clusters, the ground mask that turns normals into objects, and per-cluster boxes."""
from __future__ import annotations

import numpy as np

from . import capi


def ground_mask(normals, max_tilt_deg=15.0):
    """The include mask [m] uint8 of the NON-ground points: 0 where the normal is within max_tilt_deg of vertical
    (|nz| >= cos(max_tilt_deg)), 1 elsewhere; points without a normal ((0, 0, 0): too few neighbours) are kept."""
    n = np.asarray(normals, np.float32).reshape(-1, 3)
    ground = np.abs(n[:, 2]) >= np.float32(np.cos(np.deg2rad(float(max_tilt_deg))))
    return (~ground).astype(np.uint8)


def boxes(xyz, labels, n):
    """dict(min [n, 3], max [n, 3], centroid [n, 3] f64, count [n]) of the clusters 0 .. n-1 (host numpy); points with label -1
    belong to none.  A label without a point has min +inf, max -inf and a NaN centroid."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    labels = np.asarray(labels).reshape(-1)
    if len(labels) != len(xyz):
        raise ValueError("labels and xyz differ in length")
    sel = (labels >= 0) & (labels < n)
    lab, pts = labels[sel].astype(np.int64), xyz[sel]
    lo = np.full((n, 3), np.inf)
    hi = np.full((n, 3), -np.inf)
    np.minimum.at(lo, lab, pts)
    np.maximum.at(hi, lab, pts)
    count = np.bincount(lab, minlength=n)
    total = np.stack([np.bincount(lab, weights=pts[:, a], minlength=n) for a in range(3)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        centroid = total / count[:, None]
    return dict(min=lo, max=hi, centroid=centroid, count=count)


def remove_debris(ctx, radius=0.5, min_size=10, mask=None, dry_run=False):
    """dict(flags, n_removed): every connected blob of fewer than min_size points leaves the map (what lv_map_remove_outliers
    keeps because the blob supports itself)."""
    p = capi.default_cluster_params(radius=float(radius), min_size=int(min_size))
    return ctx.map_remove_clusters(p, mask=mask, dry_run=dry_run)


def remove_dynamic_objects(ctx, views, vis_params=None, radius=0.5, max_size=20_000, mask=None):
    """dict(n_removed, n_clusters, n_points, hits): the points a later sweep saw through (map_remove_dynamic) grown to their
    whole connected objects.  1. a dry run of map_remove_dynamic gives the hits; 2. map_remove_clusters with the hits as seeds
    takes every object of at most max_size points that holds one, whole (max_size keeps a hit on a wall from removing the
    wall); 3. the plain map_remove_dynamic then takes the seen-through points that lay in no removable cluster.
    n_clusters: points removed by step 2, n_points: by step 3; hits in map order as the map stood at the start."""
    _, hits = ctx.map_remove_dynamic(views, vis_params, dry_run=True)
    n_obj = 0
    if hits.any():
        p = capi.default_cluster_params(radius=float(radius), min_size=1, max_size=int(max_size))
        n_obj = ctx.map_remove_clusters(p, mask=mask, seeds=hits != 0)["n_removed"]
    n_pts, _ = ctx.map_remove_dynamic(views, vis_params)
    return dict(n_removed=n_obj + n_pts, n_clusters=n_obj, n_points=n_pts, hits=hits)
