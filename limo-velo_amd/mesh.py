"""TSDF fusion and the surface mesh (include/limovelo_hip.h "TSDF and mesh"): thin helpers over Context.tsdf_*.  like_occupancy()
gives a volume the footprint of an occupancy grid, integrate() fuses sweeps of any number, distance() reads the field in metres,
build() returns the triangle mesh of the zero surface, save_ply() writes it (ASCII or binary little-endian), save() / load()
keep the volume as an .npz next to occupancy.save_grid's grid, and recentre() / follow() move the volume's box with the robot
(lv_volume_recentre, "Rolling volumes").  paint() colours the volume from camera frames ("Colour layer"), colour_params_for()
picks its occlusion parameters for a camera, build(colours=True) and save_ply(colours=...) carry the vertex colours.  raycast()
casts rays at the surface ("Surface ray casting"), simulate_scan() a whole scan pattern from a pose, camera_pattern() and render()
a pinhole camera's depth, normal and colour images.  integrate_depth() fuses depth-camera frames ("Depth fusion"), depth_frame()
makes one, render_frame() renders one from the surface.  sample() reads the interpolated distance and its gradient ("Surface
registration"), align() registers a cloud against the surface from any number of guesses, align_params_for() picks the gate and
the Huber width from the volume, frame_points() back-projects a depth frame, track_depth() refines a camera pose against the
volume, loop_measurement() turns a result into a pose-graph edge.  to_occupancy() fills the occupancy grid from the volume
("Occupancy from the surface"), configuring one like the volume where there is none.  submap() takes the live volume as a submap,
merge() resamples a submap into the volume under a rigid pose ("Submap merging"), and Submaps keeps a run's submaps with their
poses, saves and loads them, and rebuilds the volume from them at the poses a pose graph has optimised."""
from __future__ import annotations

import numpy as np

from . import capi, ndt
from .synth import quat_to_rot
from .occupancy import follow_shift

MAX_VIEWS = 32   # views per lv_tsdf_integrate

_SHARED = ("origin", "resolution", "nx", "ny", "nz", "min_range", "max_range")


def like_occupancy(params, trunc_cells: int = 3, max_weight: int = 10000, carve: int = 0):
    """lv_tsdf_params with the grid and the ranges of `params` (an lv_occupancy_params, e.g. ctx.occ_params())."""
    kw = {f: ([float(v) for v in params.origin] if f == "origin" else getattr(params, f)) for f in _SHARED}
    return capi.default_tsdf_params(trunc_cells=int(trunc_cells), max_weight=int(max_weight), carve=int(carve), **kw)


def integrate(ctx, sweeps) -> np.ndarray:
    """lv_tsdf_integrate over sweeps = [(R, t, points)] of any length, 32 views per call in order; the stats [4] uint64 summed:
    rays used, rays cut, contributions, voxels touched (a voxel counts once per call that touched it)."""
    stats = np.zeros(4, np.uint64)
    sweeps = list(sweeps)
    for c0 in range(0, len(sweeps), MAX_VIEWS):
        stats += ctx.tsdf_integrate(sweeps[c0:c0 + MAX_VIEWS])
    return stats


def depth_frame(depth, R, t, fx, fy, cx, cy, depth_scale: float = 0.001, dist=None) -> dict:
    """A frame dict as integrate_depth() takes it: depth ([h, w] uint16 in units of depth_scale metres, 0 = no measurement, or
    float32 metres, NaN = none; z along the optical axis), the pose camera -> world (R, t), the pinhole, optional plumb_bob dist."""
    f = dict(depth=np.asarray(depth), R=np.asarray(R, np.float32).reshape(3, 3), t=np.asarray(t, np.float32).reshape(3), fx=float(fx), fy=float(fy),
             cx=float(cx), cy=float(cy), depth_scale=float(depth_scale))
    if dist is not None:
        f["dist"] = np.asarray(dist, np.float32).reshape(5)
    return f


def integrate_depth(ctx, frames, params=None) -> np.ndarray:
    """lv_depth_integrate over depth frames (depth_frame()) of any number, 32 views per call in order; the stats [4] uint64 summed:
    (voxel, view) pairs projected, those with a valid depth, contributions, voxels touched (once per call that touched them).
    Below the volume's max_weight the split over calls does not change the volume."""
    p = params if params is not None else capi.default_depth_params()
    stats = np.zeros(4, np.uint64)
    frames = list(frames)
    for c0 in range(0, len(frames), MAX_VIEWS):
        stats += ctx.tsdf_integrate_depth(frames[c0:c0 + MAX_VIEWS], p)
    return stats


def distance(ctx, pts):
    """(metres [n] f32, weight [n] int32): the signed distance to the fused surface at the voxel of each world point, positive on
    the sensor's side; NaN and 0 where nothing was observed or outside the volume."""
    return ctx.tsdf_query(pts)


def paint(ctx, frames, params=None) -> np.ndarray:
    """lv_colour_integrate over frames (frame dicts as capi.camera_view takes them) of any number, 32 views per call in order; the
    stats [4] uint64 summed: candidates (of every call), pairs projected, pairs seen, voxels coloured (once per call that did)."""
    p = params if params is not None else capi.default_colour_params()
    stats = np.zeros(4, np.uint64)
    frames = list(frames)
    for c0 in range(0, len(frames), MAX_VIEWS):
        stats += ctx.colour_integrate(frames[c0:c0 + MAX_VIEWS], p)
    return stats


def colour_params_for(ctx, frame, nearest: float):
    """lv_colour_params for frames like `frame` whose nearest surface is `nearest` metres away: the occlusion cells' window,
    zbuf_scale * (2 * window + 1) pixels, covers the voxel pitch fx * resolution / nearest there, so that the voxels of a wall
    leave no holes for those behind it to be seen through; margin_abs = 2.5 voxels; band = one voxel."""
    res = float(ctx.tsdf_params().resolution)
    pitch = float(frame["fx"]) * res / float(nearest)
    window, scale = 1, 1
    while scale * (2 * window + 1) < pitch:
        if scale < 16:
            scale += 1
        elif window < 8:
            window, scale = window + 1, 1
        else:
            break
    return capi.default_colour_params(zbuf_scale=scale, window=window, margin_abs=2.5 * res, band=256)


def build(ctx, min_weight: int = 1, colours: bool = False):
    """(vertices [V, 3] f32 metres, triangles [F, 3] uint32, counts [4] uint64) of the volume's zero surface over the voxels with
    weight >= min_weight; counts: vertices, triangles, active cells, edges refused for a missing cell.  Normals (the triangles'
    winding) point towards where the sensor was.  colours: a fourth item, the vertex colours [V, 4] uint8 r, g, b, a (alpha 0: no
    coloured voxel round the vertex), which needs the colour layer (paint())."""
    counts = ctx.tsdf_mesh_build(min_weight)
    m = ctx.tsdf_mesh_fetch(xyz=True, sub=False, tri=True)
    if colours:
        return m["xyz"], m["tri"], counts, ctx.mesh_colours()
    return m["xyz"], m["tri"], counts


def save_ply(path, vertices, triangles, binary: bool = True, colours=None):
    """A PLY of the mesh: vertices [V, 3] (float x y z) and triangles [F, 3] (list uchar int vertex_indices), binary little-endian
    or ASCII.  colours ([V, 3] or [V, 4] uint8): uchar red green blue per vertex behind x y z."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle refers to a vertex that does not exist")
    c = None
    if colours is not None:
        c = np.asarray(colours, np.uint8).reshape(len(v), -1)[:, :3]
    head = ("ply\nformat " + ("binary_little_endian" if binary else "ascii") + f" 1.0\nelement vertex {len(v)}\n"
            "property float x\nproperty float y\nproperty float z\n" +
            ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if c is not None else "") + f"element face {len(t)}\n"
            "property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if binary and c is not None:
            rec = np.empty(len(v), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
            rec["p"] = v
            rec["c"] = c
            f.write(rec.tobytes())
        elif binary:
            f.write(v.astype("<f4").tobytes())
        if binary:
            rec = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)])
            rec["n"] = 3
            rec["i"] = t
            f.write(rec.tobytes())
        else:
            for i, p in enumerate(v):
                tail = "" if c is None else " %d %d %d" % (c[i, 0], c[i, 1], c[i, 2])
                f.write(("%.9g %.9g %.9g%s\n" % (p[0], p[1], p[2], tail)).encode("ascii"))
            for q in t:
                f.write(("3 %d %d %d\n" % (q[0], q[1], q[2])).encode("ascii"))


def params_dict(p) -> dict:
    return {f: ([float(v) for v in p.origin] if f == "origin" else getattr(p, f)) for f, _ in capi.TsdfParams._fields_}


def _npz(path: str) -> str:
    """The file name numpy writes for `path`: np.savez appends .npz to a name that lacks it."""
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"


def save(ctx, path: str):
    """The parameters and the volume (S and W, [nz, ny, nx] int32 each) as an .npz (the extension is added to a path without it;
    load() does the same, so the same path names the file in both)."""
    vol = ctx.tsdf_fetch(S=True, W=True)
    extra = {"colour": ctx.colour_fetch(sums=True)["sums"]} if ctx.colour_info().present else {}   # ([nz, ny, nx, 4] uint32)
    np.savez_compressed(_npz(path), S=vol["S"], W=vol["W"], **extra, **{"p_" + k: np.asarray(v) for k, v in params_dict(ctx.tsdf_params()).items()})


def load(ctx, path: str):
    """Configures ctx's volume from a file of save() and loads it; returns the parameters."""
    with np.load(_npz(path)) as z:
        kw = {}
        for f, t in capi.TsdfParams._fields_:
            v = z["p_" + f]
            kw[f] = [float(x) for x in v] if f == "origin" else (int(v) if t is capi.C.c_int else float(v))
        S, W = z["S"], z["W"]
        colour = z["colour"] if "colour" in z.files else None   # (files written before the colour layer have none)
    p = capi.default_tsdf_params(**kw)
    ctx.tsdf_configure(p)
    ctx.tsdf_load(S, W)
    if colour is not None:
        ctx.colour_load(colour)
    return p


def recentre(ctx, shift) -> np.ndarray:
    """lv_volume_recentre of the TSDF volume by shift (3 whole voxels); a built mesh goes stale (its vertices are metres and stay
    right).  Returns stats [4] uint64: voxels kept, exposed (now unobserved), that had W > 0 and left the volume, 0."""
    return ctx.volume_recentre(capi.LV_VOLUME_SURFACE, shift)


def follow(ctx, position, keep=0.25, step=32, axes=(True, True, False)):
    """occupancy.follow() for the TSDF volume: returns the shift applied, (0, 0, 0) when the volume stayed."""
    d = follow_shift(ctx.tsdf_params(), position, keep, step, axes)
    if any(d):
        recentre(ctx, d)
    return d


def range_metres(resolution, results) -> np.ndarray:
    """[n] f32: resolution * ((float)depth / 256.0f) of HIT and BLOCKED rays, inf for CLEAR ones, NaN for IGNORED ones."""
    m = (np.float32(resolution) * (results["depth"].astype(np.float32) / np.float32(256.0))).astype(np.float32)
    m[results["status"] == capi.LV_SURF_CLEAR] = np.inf
    m[results["status"] == capi.LV_SURF_IGNORED] = np.nan
    return m


def raycast(ctx, frm, to, min_weight: int = 1, normals: bool = False, colours: bool = False):
    """lv_surf_raycast of the rays frm[i] -> to[i] ([n, 3] world points; frm may be one point for all): (results [n] of
    capi.TSDF_RAY_RESULT_DTYPE, ranges [n] f32 metres) and, where asked for, the normals [n, 3] f32 and the colours [n, 4] uint8
    behind them.  The range is that of the surface for a HIT (status LV_SURF_HIT), of the cell that stopped the ray for a BLOCKED
    one, inf for CLEAR and NaN for IGNORED."""
    to = np.asarray(to, np.float32).reshape(-1, 3)
    frm = np.ascontiguousarray(np.broadcast_to(np.asarray(frm, np.float32).reshape(-1, 3), to.shape))
    res, nrm, col = ctx.tsdf_raycast(frm, to, capi.default_tsdf_ray_params(min_weight=int(min_weight)), normals, colours)
    out = (res, range_metres(ctx.tsdf_params().resolution, res))
    return out + ((nrm,) if normals else ()) + ((col,) if colours else ())


def _cast_view(ctx, R, t, pattern, min_weight, normals, colours):
    pattern = np.asarray(pattern, np.float32).reshape(-1, 3)
    res, nrm, col, _ = ctx.tsdf_raycast_views([(np.asarray(R, np.float32).reshape(3, 3), np.asarray(t, np.float32).reshape(3), pattern)],
                                              capi.default_tsdf_ray_params(min_weight=int(min_weight)), normals, colours)
    rng = range_metres(ctx.tsdf_params().resolution, res)
    rng[res["status"] == capi.LV_SURF_BLOCKED] = np.inf   # (no surface seen: what stopped the ray is its back, or unobserved space)
    with np.errstate(all="ignore"):
        unit = pattern.astype(np.float64) / np.linalg.norm(pattern.astype(np.float64), axis=1)[:, None]
    return res, rng, unit, nrm, col


def simulate_scan(ctx, R, t, pattern, min_weight: int = 1):
    """What a LiDAR at the pose (R, t) would measure of the surface: lv_surf_raycast_views of the beams of `pattern`
    (occupancy.scan_pattern's end points, sensor frame), which are the rays lv_tsdf_integrate would walk for those returns.
    Returns (ranges [n] f32 metres, points [n, 3] f64 in the sensor frame): the range of a beam that HITs the surface, inf where it
    meets none (CLEAR, or BLOCKED: it met the surface from behind or out of unobserved space), NaN where the return is ignored; the
    points are NaN where the range is not finite."""
    _, rng, unit, _, _ = _cast_view(ctx, R, t, pattern, min_weight, False, False)
    pts = unit * np.where(np.isfinite(rng), rng, np.nan).astype(np.float64)[:, None]
    return rng, pts


def camera_pattern(fx, fy, cx, cy, width, height, max_range) -> np.ndarray:
    """[height * width, 3] f32: the end points, in the camera frame (z forward, x right, y down), of the rays of length max_range
    through the pixel centres of a pinhole camera without distortion, row-major."""
    v, u = np.meshgrid(np.arange(int(height), dtype=np.float64), np.arange(int(width), dtype=np.float64), indexing="ij")
    d = np.stack([(u - float(cx)) / float(fx), (v - float(cy)) / float(fy), np.ones_like(u)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (float(max_range) * d).astype(np.float32)


def render(ctx, R, t, fx, fy, cx, cy, width, height, max_range=None, min_weight: int = 1):
    """The surface as a pinhole camera at the pose (R, t) (camera to world) sees it: (depth [height, width] f32, normals [height,
    width, 3] f32 in the world frame, rgba [height, width, 4] uint8).  depth is the z-depth, the range times the z component of the
    pixel's unit ray, NaN where the ray does not HIT the surface; normals and colours are zeros there.  max_range: the rays'
    length (default: the volume's max_range).  No distortion."""
    if max_range is None:
        max_range = ctx.tsdf_params().max_range
    pattern = camera_pattern(fx, fy, cx, cy, width, height, max_range)
    res, rng, unit, nrm, col = _cast_view(ctx, R, t, pattern, min_weight, True, True)
    depth = np.where(res["status"] == capi.LV_SURF_HIT, rng.astype(np.float64) * unit[:, 2], np.nan).astype(np.float32)
    shape = (int(height), int(width))
    return depth.reshape(shape), nrm.reshape(shape + (3,)), col.reshape(shape + (4,))


def render_frame(ctx, R, t, fx, fy, cx, cy, width, height, max_range=None, min_weight: int = 1) -> dict:
    """render()'s depth as a depth frame (float32 metres, NaN where no ray HITs): what a depth camera at the pose would hand to
    integrate_depth() of another context."""
    depth, _, _ = render(ctx, R, t, fx, fy, cx, cy, width, height, max_range, min_weight)
    return depth_frame(depth, R, t, fx, fy, cx, cy)


def sample(ctx, pts, min_weight: int = 1):
    """lv_surf_sample at world points [n, 3]: (d [n] f64 metres, n [n, 3] f64, status [n] uint8): the trilinear distance to the
    surface, positive on the sensor's side, and the exact gradient of that interpolant (about unit length inside the band, zero
    where the field is clamped); zeros where status is not capi.SURF_SAMPLE_KNOWN (outside the volume, or next to a voxel below
    min_weight)."""
    return ctx.surf_sample(pts, min_weight)


def align_params_for(ctx, **kw):
    """lv_surf_align_params for ctx's volume: max_dist = (trunc_cells - 1) * resolution, inside which the fused distances are not
    clamped, and huber = resolution / 2; kw overrides any field (a volume with trunc_cells = 1 needs its own max_dist)."""
    p = ctx.tsdf_params()
    res = float(p.resolution)
    return capi.default_surf_align_params(**dict(dict(max_dist=(p.trunc_cells - 1) * res, huber=res / 2), **kw))


def align(ctx, points, guesses, **kw):
    """lv_surf_align of points [n, 3] (sensor frame) against the surface from guesses [K, 7] (t, q = x y z w, sensor -> world) with
    align_params_for(ctx, **kw): (results [K] of capi.SURF_ALIGN_RESULT_DTYPE, best = (index, n_in) or (-1, -1))."""
    return ctx.surf_align(points, guesses, align_params_for(ctx, **kw))


def frame_points(frame, stride: int = 1) -> np.ndarray:
    """[n, 3] f32: the pixels of a depth_frame() with a valid depth (finite and > 0), every stride-th row and column, as points in
    the camera frame (z forward, x right, y down; pixel centres at whole u, v as in camera_pattern()).  Pinhole only."""
    if "dist" in frame and np.any(np.asarray(frame["dist"]) != 0):
        raise ValueError("frame_points: a distorted frame is not supported (dist must be zero)")
    d = np.asarray(frame["depth"])
    z = d.astype(np.float64) * (float(frame.get("depth_scale", 0.001)) if d.dtype.kind in "ui" else 1.0)
    s = int(stride)
    if s < 1:
        raise ValueError("frame_points: stride >= 1")
    v, u = np.meshgrid(np.arange(0, d.shape[0], s, dtype=np.float64), np.arange(0, d.shape[1], s, dtype=np.float64), indexing="ij")
    z = z[::s, ::s]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z > 0)
    z, u, v = z[ok], u[ok], v[ok]
    return np.stack([(u - float(frame["cx"])) / float(frame["fx"]) * z, (v - float(frame["cy"])) / float(frame["fy"]) * z, z], axis=1).astype(np.float32)


def _quat_of(R) -> np.ndarray:
    """x, y, z, w of a rotation matrix (Shepperd's branches)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    k = int(np.argmax([R[0, 0], R[1, 1], R[2, 2], np.trace(R)]))
    if k == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + np.trace(R)])
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q = np.zeros(4)
        q[i] = 1.0 + R[i, i] - R[j, j] - R[l, l]
        q[j] = R[j, i] + R[i, j]
        q[l] = R[l, i] + R[i, l]
        q[3] = R[l, j] - R[j, l]
    return q / np.linalg.norm(q)


def track_depth(ctx, frame, guess=None, stride: int = 4, **kw):
    """The pose of a depth camera against the volume: frame_points(frame, stride) aligned from guess = (R, t) camera -> world (None:
    the frame's own pose).  Returns (R [3, 3] f64, t [3] f64, result): the refined pose and its capi.SURF_ALIGN_RESULT_DTYPE record
    (status capi.SURF_ALIGN_NO_OVERLAP: the guess, untouched)."""
    R0, t0 = (frame["R"], frame["t"]) if guess is None else guess
    g = np.concatenate([np.asarray(t0, np.float64).reshape(3), _quat_of(R0)])
    res, _ = align(ctx, frame_points(frame, stride), g[None], **kw)
    return quat_to_rot(res[0]["q"]), res[0]["t"].copy(), res[0]


def loop_measurement(x_i, result):
    """ndt.loop_measurement for a surface registration: (t, q, info) of T_i^-1 T_j for PoseGraph.add_registration, where the volume
    is in the frame keyframe i's pose x_i is given in."""
    return ndt.loop_measurement(x_i, result)


def to_occupancy(ctx, **kw) -> np.ndarray:
    """The occupancy grid filled from the volume (occupancy.from_surface; kw as there, mode included).  Where no grid is configured
    one is configured like the volume first: its origin, resolution, shape and ranges, the log-odds constants at their defaults
    (the inverse of like_occupancy()).  Returns from_surface's stats."""
    from . import occupancy

    try:
        ctx.occ_params()
    except capi.LvError as e:
        if "no occupancy grid" not in str(e):
            raise
        t = ctx.tsdf_params()
        p = capi.default_occupancy_params()
        for f in _SHARED:
            if f == "origin":
                p.origin[:] = [float(v) for v in t.origin]
            else:
                setattr(p, f, getattr(t, f))
        ctx.occ_configure(p)
    return occupancy.from_surface(ctx, **kw)


def submap(ctx) -> dict:
    """The live volume as a submap: dict(origin [3], resolution, trunc_cells, S, W [nz, ny, nx] int32), what merge() takes."""
    p = ctx.tsdf_params()
    vol = ctx.tsdf_fetch(S=True, W=True)
    return dict(origin=np.array([float(v) for v in p.origin], np.float32), resolution=np.float32(p.resolution), trunc_cells=int(p.trunc_cells),
                S=vol["S"], W=vol["W"])


def pose7(pose) -> np.ndarray:
    """[7] f64 (t, q = x y z w) of a pose given as that, as (t [3], q [4]) or as a 4 x 4 matrix."""
    a = pose if isinstance(pose, np.ndarray) else None
    if a is None and len(pose) == 2:
        return np.concatenate([np.asarray(pose[0], np.float64).reshape(3), np.asarray(pose[1], np.float64).reshape(4)])
    a = np.asarray(pose, np.float64)
    if a.shape == (4, 4):
        return np.concatenate([a[:3, 3], _quat_of(a[:3, :3])])
    return a.reshape(7).copy()


def merge(ctx, submap, pose, min_weight: int = 1, nearest: bool = False) -> np.ndarray:
    """lv_surf_merge: the submap (submap()'s dict) resampled into ctx's volume at pose (submap -> world: (t, q), [7] or 4 x 4) and
    folded in as evidence; a built mesh goes stale.  Returns stats [4] uint64: destination voxels not OUTSIDE the submap, voxels
    that took evidence, the sum of their dW, voxels DROPPED behind the volume's band."""
    m, keep = capi.surf_submap(submap["origin"], submap["resolution"], submap["trunc_cells"], submap["S"], submap["W"])
    prm = capi.default_surf_merge_params(min_weight=int(min_weight), interp=capi.LV_MERGE_NEAREST if nearest else capi.LV_MERGE_TRILINEAR)
    stats = ctx.surf_merge(m, pose7(pose), prm)
    del keep
    return stats


class Submaps:
    """A run kept as submaps: volumes as submap() gives them, each with the pose (submap -> world) of its pose-graph node.  fuse()
    rebuilds ctx's volume from all of them, e.g. at the poses graph.PoseGraph has optimised."""

    def __init__(self):
        self.submaps = []
        self.poses = []

    def __len__(self):
        return len(self.submaps)

    def add(self, submap, pose) -> int:
        """Keeps a submap with its pose; returns its index."""
        self.submaps.append(dict(submap))
        self.poses.append(pose7(pose))
        return len(self.submaps) - 1

    def save(self, path: str):
        """All submaps and poses as one .npz (the extension is added to a path without it)."""
        z = {"n": np.asarray(len(self)), "poses": np.asarray(self.poses, np.float64).reshape(-1, 7)}
        for k, m in enumerate(self.submaps):
            z[f"S{k}"], z[f"W{k}"] = np.asarray(m["S"], np.int32), np.asarray(m["W"], np.int32)
            z[f"g{k}"] = np.array([*(float(v) for v in m["origin"]), float(m["resolution"]), float(m["trunc_cells"])], np.float32)
        np.savez_compressed(_npz(path), **z)

    @classmethod
    def load(cls, path: str):
        out = cls()
        with np.load(_npz(path)) as z:
            for k in range(int(z["n"])):
                g = z[f"g{k}"]
                out.add(dict(origin=g[:3].copy(), resolution=np.float32(g[3]), trunc_cells=int(g[4]), S=z[f"S{k}"], W=z[f"W{k}"]), z["poses"][k])
        return out

    def fuse(self, ctx, poses=None, min_weight: int = 1, nearest: bool = False) -> np.ndarray:
        """lv_tsdf_clear, then one merge per submap in order, at `poses` (one per submap; default: the poses kept).  Returns the summed
        stats."""
        use = self.poses if poses is None else [pose7(p) for p in poses]
        if len(use) != len(self.submaps):
            raise ValueError("Submaps.fuse: one pose per submap")
        ctx.tsdf_clear()
        stats = np.zeros(4, np.uint64)
        for m, p in zip(self.submaps, use):
            stats += merge(ctx, m, p, min_weight=min_weight, nearest=nearest)
        return stats
