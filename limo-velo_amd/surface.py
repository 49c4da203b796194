"""Surface normals and outlier removal on the device map (include/limovelo_hip.h "Surface normals and outlier removal"): thin
helpers over Context.map_normals / Context.map_remove_outliers, and a PLY writer that carries the normals."""
from __future__ import annotations

import numpy as np

from . import capi


def estimate(ctx, k=10, max_dist=2.0, min_neighbours=5, viewpoint=None):
    """dict(normals [m, 3], curvature [m], mean_dist [m], n_used [m]) in map order (the order of ctx.map_fetch()).  viewpoint: the
    normals face it (e.g. the sensor's position); None: the component of largest magnitude is positive."""
    p = capi.default_surface_params(k=int(k), max_dist=float(max_dist), min_neighbours=int(min_neighbours))
    if viewpoint is not None:
        p.orient = 1
        p.viewpoint[:] = [float(v) for v in viewpoint]
    return ctx.map_normals(p)


def clean(ctx, mode="statistical", k=10, std_mul=2.0, max_dist=2.0, radius=0.5, min_neighbours=5, dry_run=False):
    """(n_removed, flags [m] uint8 in map order as the map stood before, stats (mu, sigma, threshold)): the points without support
    leave the map.  mode "statistical": mean distance to the k nearest others above mu + std_mul sigma (or fewer than k others
    within max_dist); "radius": fewer than min_neighbours others within radius."""
    modes = {"statistical": 0, "radius": 1}
    if mode not in modes:
        raise ValueError(f"mode {mode!r}: 'statistical' or 'radius'")
    p = capi.default_outlier_params(mode=modes[mode], k=int(k), std_mul=float(std_mul), max_dist=float(max_dist), radius=float(radius),
                                    min_neighbours=int(min_neighbours))
    return ctx.map_remove_outliers(p, dry_run=dry_run)


def save_ply(path, xyz, normals=None, rgb=None):
    """A binary little-endian PLY of the points xyz [m, 3], with nx ny nz (float) when normals [m, 3] are given and red green blue
    (uchar, rounded from 0..255) when rgb [m, 3] is."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError("normals and xyz differ in length")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if rgb is not None:
        rgb = np.asarray(rgb, np.float64).reshape(-1, 3)
        if len(rgb) != len(xyz):
            raise ValueError("rgb and xyz differ in length")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(len(xyz), dtype=fields)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if rgb is not None:
        c = np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    head = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {len(rec)}\n" + "\n".join(props) + "\nend_header\n"
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())
