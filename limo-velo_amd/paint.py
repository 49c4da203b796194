"""The vision buffer: colours for the device map's points from camera frames (include/limovelo_hip.h "Map painting").

VisionBuffer keeps the latest frames; paint() colours the map as it stands from any number of them, calling lv_map_paint in
chunks of at most 32 views and merging the chunks; save_ply() writes the painted map.  Colours are not carried with the points
across later inserts, evictions or rebuilds: paint right before export.

A frame is a dict: stamp, image ([h, w, 3] or [h, w] uint8), format (capi.LV_IMAGE_*), fx, fy, cx, cy, dist (k1, k2, p1, p2, k3),
R [3, 3] and t [3], the camera -> world pose (capi.camera_pose forms it from a filter state and the camera -> IMU extrinsic)."""
from __future__ import annotations

import collections

import numpy as np

from . import capi

MAX_VIEWS = 32   # views per lv_map_paint call


class VisionBuffer:
    """The latest `capacity` frames, oldest first."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.capacity = int(capacity)
        self._frames = collections.deque(maxlen=self.capacity)

    def add(self, stamp, image, R, t, fx, fy, cx, cy, *, fmt=None, dist=None):
        img = np.asarray(image)
        if fmt is None:
            fmt = capi.LV_IMAGE_MONO8 if img.ndim == 2 else capi.LV_IMAGE_RGB8
        self._frames.append(dict(stamp=float(stamp), image=img, format=int(fmt), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy),
                                 dist=np.zeros(5, np.float32) if dist is None else np.asarray(dist, np.float32).ravel(),
                                 R=np.asarray(R, np.float32).reshape(3, 3), t=np.asarray(t, np.float32).ravel()))

    def frames(self):
        return list(self._frames)

    def clear(self):
        self._frames.clear()

    def __len__(self):
        return len(self._frames)

    def __iter__(self):
        return iter(list(self._frames))


def merge(parts, blend: int):
    """(rgb [m, 3] f32, depth [m] f32, n_seen [m] int32) from the per-chunk results [(rgb, depth, n_seen)], chunks in view order.
    blend 0: the chunks' means weighted by their counts; blend 1: the chunk with the smallest depth (ties: the earlier chunk)."""
    rgb0, depth0, seen0 = parts[0]
    m = len(depth0)
    n = np.zeros(m, np.int64)
    depth = np.full(m, np.inf, np.float32)
    if blend == 0:
        acc = np.zeros((m, 3), np.float64)
        for rgb, d, s in parts:
            s = np.asarray(s, np.int64)
            acc += np.asarray(rgb, np.float64) * s[:, None]
            n += s
            depth = np.minimum(depth, d)
        out = np.zeros((m, 3), np.float32)
        ok = n > 0
        out[ok] = (acc[ok] / n[ok, None]).astype(np.float32)
    else:
        out = np.zeros((m, 3), np.float32)
        for rgb, d, s in parts:
            take = np.asarray(d) < depth
            out[take] = rgb[take]
            depth = np.where(take, d, depth).astype(np.float32)
            n += np.asarray(s, np.int64)
    return out, depth, n.astype(np.int32)


def paint(ctx, buffer_or_frames, params=None):
    """(rgb [m, 3] f32, depth [m] f32, n_seen [m] int32) for the current map of `ctx` in map order (lv_map_fetch's), from a
    VisionBuffer or a list of frames: lv_map_paint over chunks of at most 32 views, merged (merge)."""
    frames = list(buffer_or_frames)
    if not frames:
        raise ValueError("no frames to paint from")
    p = params if params is not None else capi.default_paint_params()
    parts = [ctx.map_paint(frames[i:i + MAX_VIEWS], p) for i in range(0, len(frames), MAX_VIEWS)]
    if len(parts) == 1:
        rgb, depth, seen = parts[0]
        return rgb, depth, seen.astype(np.int32)
    return merge(parts, int(p.blend))


def save_ply(path, xyz, rgb, mask=None):
    """A binary little-endian PLY of the points xyz [m, 3] with colours rgb [m, 3] (0..255, rounded to uchar); mask [m] bool: only
    those points (e.g. n_seen > 0)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.float64).reshape(-1, 3)
    if mask is not None:
        mask = np.asarray(mask, bool)
        xyz, rgb = xyz[mask], rgb[mask]
    rec = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c = np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
    rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(rec)}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())


def load_ply(path):
    """(xyz [n, 3] f32, rgb [n, 3] uint8) of a PLY written by save_ply."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if head[0] != "ply" or head[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    n = int(next(h for h in head if h.startswith("element vertex")).split()[2])
    rec = np.frombuffer(data[end:], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")], count=n)
    return np.stack([rec["x"], rec["y"], rec["z"]], axis=1), np.stack([rec["red"], rec["green"], rec["blue"]], axis=1)
