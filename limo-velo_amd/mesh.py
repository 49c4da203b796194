"""TSDF fusion and the surface mesh (include/limovelo_hip.h "TSDF and mesh"): thin helpers over Context.tsdf_*.  like_occupancy()
gives a volume the footprint of an occupancy grid, integrate() fuses sweeps of any number, distance() reads the field in metres,
build() returns the triangle mesh of the zero surface, save_ply() writes it (ASCII or binary little-endian), save() / load()
keep the volume as an .npz next to occupancy.save_grid's grid, and recentre() / follow() move the volume's box with the robot
(lv_volume_recentre, "Rolling volumes")."""
from __future__ import annotations

import numpy as np

from . import capi
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


def distance(ctx, pts):
    """(metres [n] f32, weight [n] int32): the signed distance to the fused surface at the voxel of each world point, positive on
    the sensor's side; NaN and 0 where nothing was observed or outside the volume."""
    return ctx.tsdf_query(pts)


def build(ctx, min_weight: int = 1):
    """(vertices [V, 3] f32 metres, triangles [F, 3] uint32, counts [4] uint64) of the volume's zero surface over the voxels with
    weight >= min_weight; counts: vertices, triangles, active cells, edges refused for a missing cell.  Normals (the triangles'
    winding) point towards where the sensor was."""
    counts = ctx.tsdf_mesh_build(min_weight)
    m = ctx.tsdf_mesh_fetch(xyz=True, sub=False, tri=True)
    return m["xyz"], m["tri"], counts


def save_ply(path, vertices, triangles, binary: bool = True):
    """A PLY of the mesh: vertices [V, 3] (float x y z) and triangles [F, 3] (list uchar int vertex_indices), binary little-endian
    or ASCII."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle refers to a vertex that does not exist")
    head = ("ply\nformat " + ("binary_little_endian" if binary else "ascii") + f" 1.0\nelement vertex {len(v)}\n"
            "property float x\nproperty float y\nproperty float z\n" + f"element face {len(t)}\n"
            "property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if binary:
            f.write(v.astype("<f4").tobytes())
            rec = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)])
            rec["n"] = 3
            rec["i"] = t
            f.write(rec.tobytes())
        else:
            for p in v:
                f.write(("%.9g %.9g %.9g\n" % (p[0], p[1], p[2])).encode("ascii"))
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
    np.savez_compressed(_npz(path), S=vol["S"], W=vol["W"], **{"p_" + k: np.asarray(v) for k, v in params_dict(ctx.tsdf_params()).items()})


def load(ctx, path: str):
    """Configures ctx's volume from a file of save() and loads it; returns the parameters."""
    with np.load(_npz(path)) as z:
        kw = {}
        for f, t in capi.TsdfParams._fields_:
            v = z["p_" + f]
            kw[f] = [float(x) for x in v] if f == "origin" else (int(v) if t is capi.C.c_int else float(v))
        S, W = z["S"], z["W"]
    p = capi.default_tsdf_params(**kw)
    ctx.tsdf_configure(p)
    ctx.tsdf_load(S, W)
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
