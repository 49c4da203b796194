"""A pose graph over keyframes on top of lv_graph_* (include/limovelo_hip.h "Pose graph"): it collects keyframes with the odometry
edges between consecutive ones, loop edges (what places.candidates + Context.update_batch deliver: the refined state at a revisit)
and GPS priors (positions in the map frame, through aiding.to_map), solves on the device, vets loop closures by their chi-square
and regenerates the device map from body-frame keyframe clouds moved by the correction, the way LIO-SAM rebuilds its map.

Plumbing only: residuals, the solver and the warp of the points are the library's."""
from __future__ import annotations

import numpy as np

from . import capi
from .synth import quat_mul, quat_to_rot


def _pose(state) -> np.ndarray:
    s = np.asarray(state, np.float64)
    q = s[3:7] / np.linalg.norm(s[3:7])
    return np.concatenate([s[0:3], q])


def relative(xa, xb):
    """T_a^-1 T_b of two states (or poses [7]): (t [3], q [4], x y z w)."""
    a, b = _pose(xa), _pose(xb)
    t = quat_to_rot(a[3:]).T @ (b[:3] - a[:3])
    q = quat_mul(np.array([-a[3], -a[4], -a[5], a[6]]), b[3:])
    return t, q / np.linalg.norm(q)


def info_from_sigmas(sigma_t, sigma_r) -> np.ndarray:
    """diag(1 / sigma^2) of a 6-dof measurement; scalars or 3-vectors"""
    st, sr = np.broadcast_to(np.asarray(sigma_t, np.float64), 3), np.broadcast_to(np.asarray(sigma_r, np.float64), 3)
    return np.diag(np.concatenate([1.0 / st ** 2, 1.0 / sr ** 2]))


_TRIU = np.triu_indices(6)


class PoseGraph:
    def __init__(self):
        self.states: list[np.ndarray] = []
        self.fixed: list[bool] = []
        self.edges: list[np.ndarray] = []     # odometry and loop edges in the order given
        self.is_loop: list[bool] = []
        self.priors: list[np.ndarray] = []
        self.poses: np.ndarray | None = None  # [n, 7] after optimise

    def __len__(self):
        return len(self.states)

    def _edge(self, i, j, t, q, info, huber, loop):
        e = np.zeros((), capi.GRAPH_EDGE_DTYPE)
        e["i"], e["j"], e["t"], e["q"], e["info"], e["huber"] = i, j, t, q, np.asarray(info, np.float64)[_TRIU], huber
        self.edges.append(e)
        self.is_loop.append(loop)

    def add_keyframe(self, state, sigma_t=0.05, sigma_r=0.01, info=None, huber=0.0, fixed=False) -> int:
        """Appends a keyframe at `state` (26 doubles); from the second on, an odometry edge from the one before with the relative
        pose of the two states as measurement.  Returns its id."""
        k = len(self.states)
        self.states.append(np.array(state, np.float64))
        self.fixed.append(bool(fixed))
        if k:
            t, q = relative(self.states[k - 1], self.states[k])
            self._edge(k - 1, k, t, q, info_from_sigmas(sigma_t, sigma_r) if info is None else info, huber, False)
        return k

    def add_loop(self, i, j, x_i, x_refined_j, info=None, sigma_t=0.05, sigma_r=0.01, huber=0.0):
        """A loop edge i -> j: keyframe j's scan, refined against the map round keyframe i, stood at x_refined_j while keyframe i
        stood at x_i; the measurement is T_i^-1 T_j of those two."""
        t, q = relative(x_i, x_refined_j)
        self._edge(int(i), int(j), t, q, info_from_sigmas(sigma_t, sigma_r) if info is None else info, huber, True)

    def add_registration(self, i, j, t, q, info, huber=0.0):
        """A loop edge i -> j from a cloud-to-cloud registration (ndt.loop_measurement of lv_ndt_align's result): the measurement
        T_i^-1 T_j as (t, q) with its 6 x 6 information."""
        self._edge(int(i), int(j), np.asarray(t, np.float64), np.asarray(q, np.float64), info, huber, True)

    def add_gps(self, k, position, sigma=(0.2, 0.2, 0.5), lever=(0.0, 0.0, 0.0), huber=0.0):
        """A position prior on keyframe k: the antenna (at `lever` in the body frame) at `position` in the map frame
        (aiding.to_map of an ENU fix)."""
        p = np.zeros((), capi.GRAPH_PRIOR_DTYPE)
        W = np.zeros((6, 6))
        W[:3, :3] = np.diag(1.0 / np.broadcast_to(np.asarray(sigma, np.float64), 3) ** 2)
        p["i"], p["t"], p["q"], p["lever"], p["info"], p["huber"] = int(k), position, (0, 0, 0, 1), lever, W[_TRIU], huber
        self.priors.append(p)

    def records(self):
        """(poses [n, 7], fixed [n], edges, priors) as lv_graph_set takes them.  With nothing fixed and no prior, keyframe 0 is fixed."""
        poses = np.array([_pose(s) for s in self.states])
        fixed = np.array(self.fixed, bool)
        if not fixed.any() and not self.priors:
            fixed[0] = True
        return poses, fixed, np.array(self.edges, capi.GRAPH_EDGE_DTYPE), np.array(self.priors, capi.GRAPH_PRIOR_DTYPE)

    def optimise(self, ctx, **params) -> dict:
        """lv_graph_set + lv_graph_optimise (params: fields of lv_graph_params); keeps the corrected poses.  Returns the info record."""
        ctx.graph_set(*self.records())
        info = ctx.graph_optimise(**params)
        self.poses = ctx.graph_fetch()
        return info

    def vet(self, ctx, threshold: float, **params):
        """Drops the loop edges whose chi-square at the current solution (lv_graph_chi2) exceeds threshold and solves again.
        Returns (ids of the dropped edges in the order they were added, the new info record or None when nothing was dropped)."""
        if self.poses is None:
            self.optimise(ctx, **params)
        es, _ = ctx.graph_chi2()
        drop = [k for k in range(len(self.edges)) if self.is_loop[k] and es[k] > threshold]
        if not drop:
            return [], None
        keep = [k for k in range(len(self.edges)) if k not in set(drop)]
        self.edges, self.is_loop = [self.edges[k] for k in keep], [self.is_loop[k] for k in keep]
        return drop, self.optimise(ctx, **params)

    def corrected_states(self) -> list[np.ndarray]:
        """The keyframe states with position and rotation replaced by the solution."""
        if self.poses is None:
            raise RuntimeError("optimise first")
        out = []
        for s, p in zip(self.states, self.poses):
            c = s.copy()
            c[0:7] = p
            out.append(c)
        return out

    def rebuild_map(self, ctx, keyframe_scans) -> np.ndarray:
        """keyframe_scans: {keyframe id: [m, 3] points in that keyframe's body frame}.  Every cloud is placed at its keyframe's
        original pose (f64, rounded to f32), moved by the node's correction with lv_graph_warp_points, and the whole is handed to
        lv_map_build.  Returns the [M, 3] f32 points given to the map.  The graph set by optimise must still be the context's."""
        pts, keys = [], []
        for k in sorted(keyframe_scans):
            p0 = _pose(self.states[k])
            body = np.asarray(keyframe_scans[k], np.float64).reshape(-1, 3)
            pts.append((body @ quat_to_rot(p0[3:]).T + p0[:3]).astype(np.float32))
            keys.append(np.full(len(body), k, np.uint32))
        world = ctx.graph_warp_points(np.concatenate(pts), np.concatenate(keys))
        ctx.map_build(world)
        return world
