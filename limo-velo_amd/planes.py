"""RANSAC plane segmentation of the device map (include/limovelo_hip.h "Plane segmentation"; PCL's SACSegmentation with
SACMODEL_PLANE and its axis-constrained forms): thin helpers over Context.map_planes.

The floor as a plane, not as "normals close to vertical": a table top or a car roof passes cluster.ground_mask's 15 degree test,
a rough or sloped floor fails it.  ground() finds the one dominant plane whose normal is within max_angle_deg of `up` and returns
its members, which is the mask a clustering of the objects on that floor wants:

    ground_mask, floor = planes.ground(ctx)                                  # [m] bool in map order, the plane's record
    cluster.remove_dynamic_objects(ctx, views, mask=~ground_mask)             # objects do not link through the floor
    out = ctx.map_cluster(capi.default_cluster_params(radius=0.3), mask=~ground_mask)

walls() does the same for the planes that contain `up`; segment() is the plain call with keyword parameters."""
from __future__ import annotations

import numpy as np

from . import capi

# label -> colour of save_ply: -1 grey, then a fixed cycle
PALETTE = np.array([[230, 25, 75], [60, 180, 75], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240], [240, 50, 230],
                    [210, 245, 60], [250, 190, 190], [0, 128, 128], [230, 190, 255], [170, 110, 40], [255, 250, 200], [128, 0, 0],
                    [170, 255, 195], [128, 128, 0]], np.uint8)
GREY = np.array([128, 128, 128], np.uint8)


def segment(ctx, mask=None, **params) -> dict:
    """dict(labels [m] int32 in map order, planes [P] records (capi.PLANE_DTYPE), n_planes): lv_map_planes with the defaults
    overridden by keyword (distance, iterations, max_planes, min_inliers, seed, constraint, axis, max_angle [rad], refine)."""
    return ctx.map_planes(capi.default_plane_params(**params), mask=mask)


def ground(ctx, up=(0.0, 0.0, 1.0), max_angle_deg=10.0, mask=None, **params):
    """(mask [m] bool in map order, plane record or None): the members of the dominant plane whose normal lies within
    max_angle_deg of `up`.  No such plane with min_inliers points: an all-False mask and None."""
    out = segment(ctx, mask=mask, **{**params, "max_planes": 1, "constraint": 1, "axis": up, "max_angle": float(np.deg2rad(max_angle_deg))})
    return out["labels"] == 0, (out["planes"][0] if out["n_planes"] else None)


def walls(ctx, up=(0.0, 0.0, 1.0), max_angle_deg=10.0, max_planes=8, mask=None, **params) -> dict:
    """segment() restricted to planes that contain `up` to within max_angle_deg (the normal within that angle of the plane
    perpendicular to `up`), up to max_planes of them, largest support first as RANSAC finds them."""
    return segment(ctx, mask=mask, **{**params, "max_planes": int(max_planes), "constraint": 2, "axis": up,
                                      "max_angle": float(np.deg2rad(max_angle_deg))})


def signed_distance(plane, xyz) -> np.ndarray:
    """[n] f32: s of the rule's inlier test for the points xyz [n, 3] against a plane record, (normal . (p - anchor)) in f32 as
    the library forms it; |s| <= distance is membership."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    n, a = np.asarray(plane["normal"], np.float32), np.asarray(plane["anchor"], np.float32)
    q = p - a[None, :]
    return (n[0] * q[:, 0] + n[1] * q[:, 1]) + n[2] * q[:, 2]


def save_ply(path, xyz, labels) -> None:
    """A binary little-endian PLY of the points coloured by label (-1 grey)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    labels = np.asarray(labels).reshape(-1)
    if len(labels) != len(xyz):
        raise ValueError("labels and xyz differ in length")
    rgb = np.where((labels >= 0)[:, None], PALETTE[np.maximum(labels, 0) % len(PALETTE)], GREY[None, :]).astype(np.uint8)
    rec = np.empty(len(xyz), np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    rec["xyz"], rec["rgb"] = xyz, rgb
    header = ("ply\nformat binary_little_endian 1.0\n" f"element vertex {len(xyz)}\n"
              "property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
