"""NDT registration on top of lv_ndt_* (include/limovelo_hip.h "NDT registration"): cloud-to-cloud alignment from several guesses,
and the measurement a pose graph takes from its result (graph.PoseGraph.add_registration).

Plumbing only: the voxel Gaussians, the score and the Levenberg-Marquardt loop are the library's."""
from __future__ import annotations

import math

import numpy as np

from . import capi
from .synth import quat_mul, quat_to_rot

_TRIU = np.triu_indices(6)


def gauss_d2(resolution: float = 1.0, outlier_ratio: float = 0.55) -> float:
    """Magnusson's d2 for voxels of `resolution` metres (what PCL computes as gauss_d2_): 0.433 for 1 m and 0.55."""
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / resolution ** 3
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    return -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)


def grid_for(points, resolution: float = 1.0, margin: float = 1.0, **kw) -> capi.NdtParams:
    """lv_ndt_params whose grid covers the finite points with `margin` metres to spare on every side; the origin is a whole
    multiple of the resolution, so two clouds of one place share their voxel faces."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[np.all(np.isfinite(p), axis=1)]
    if not len(p):
        raise ValueError("no finite point")
    lo = np.floor((p.min(axis=0) - margin) / resolution)
    n = np.floor((p.max(axis=0) + margin) / resolution) - lo + 1
    if np.any(n > 1024) or np.prod(n) > (1 << 22):
        raise ValueError(f"{n.astype(int)} voxels: more than lv_ndt_build takes (coarsen the resolution)")
    return capi.default_ndt_params(origin=lo * resolution, resolution=float(resolution), nx=int(n[0]), ny=int(n[1]), nz=int(n[2]), **kw)


def yaw_guesses(pose, n: int) -> np.ndarray:
    """[n, 7]: pose turned about its own z axis by 2 pi k / n, k = 0..n-1 (k = 0 is the pose itself, bit for bit)"""
    x = np.asarray(pose, np.float64)[:7]
    out = np.tile(x, (n, 1))
    for k in range(1, n):
        a = math.pi * k / n
        q = quat_mul(x[3:7], np.array([0.0, 0.0, math.sin(a), math.cos(a)]))
        out[k, 3:] = q / np.linalg.norm(q)
    return out


def register(ctx, target_points, source_points, guesses, resolution: float = 1.0, margin: float = 1.0, min_points: int = 5, reg: float = 0.01,
             **align):
    """Builds the target's Gaussians from target_points (None: the device map, over the default grid) and aligns source_points
    from guesses [K, 7].  align: fields of lv_ndt_align_params; d2 defaults to gauss_d2(resolution).  Returns (the best result as
    a record of capi.NDT_RESULT_DTYPE or None, all results, best index)."""
    if target_points is None:
        ctx.ndt_build(capi.default_ndt_params(min_points=min_points, reg=reg), None)
    else:
        ctx.ndt_build(grid_for(target_points, resolution, margin, min_points=min_points, reg=reg), target_points)
    align.setdefault("d2", gauss_d2(resolution))
    res, best = ctx.ndt_align(source_points, np.asarray(guesses, np.float64).reshape(-1, 7), **align)
    return (res[best[0]] if best[0] >= 0 else None), res, best[0]


def loop_measurement(x_i, result):
    """(t [3], q [4], info [6, 6]) of T_i^-1 T_j for PoseGraph.add_registration: keyframe j's cloud was aligned to a target in the
    frame keyframe i's pose x_i is given in, and stands at result's pose.  info is H at that pose, carried from the increment of
    T_j to the edge's residual: the translation rows and columns turn by R_i (the residual's translation lives in frame i; its
    rotation in frame j, where H's already is)."""
    xi = np.asarray(x_i, np.float64)
    qi = xi[3:7] / np.linalg.norm(xi[3:7])
    tj, qj = np.asarray(result["t"], np.float64), np.asarray(result["q"], np.float64)
    Ri = quat_to_rot(qi)
    t = Ri.T @ (tj - xi[:3])
    q = quat_mul(np.array([-qi[0], -qi[1], -qi[2], qi[3]]), qj)
    H = np.zeros((6, 6))
    H[_TRIU] = np.asarray(result["info"], np.float64)
    H = H + np.triu(H, 1).T
    B = np.eye(6)
    B[:3, :3] = Ri          # d t_j = Ri d r_t
    return t, q / np.linalg.norm(q), B.T @ H @ B
