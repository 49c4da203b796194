"""Offline mapping on top of lv_traj_* (include/limovelo_hip.h "Trajectory"): record the filter's stamped states (and the raw
sweeps) during a run, turn them into a trajectory on the device, spread a solved pose graph's corrections over it, smooth it, and
register every raw point again at the pose of its own time stamp: the map is rebuilt without the step a rigid, per-keyframe
placement leaves at every keyframe boundary.

Plumbing only: interpolation, smoothing, correction and registration are the library's.

The whole pass (ctx: capi.Context; G: graph.PoseGraph whose keyframes were added at keyframe_times; loops found with
places.candidates and refined with ndt.loop_measurement or Context.update_batch):

    rec = offline.Recorder(keep_sweeps=True)
    for sweep in run:                                    # sweep: POINT_DTYPE records, raw, in the LiDAR frame
        ...                                              # the online pipeline: predict, de-skew, update
        rec.add_state(t_end, ctx.filter_get()[0])
        rec.add_sweep(sweep)
    G.add_loop(i, j, x_i, x_refined_j)                   # loop edges
    G.optimise(ctx)                                      # lv_graph_set + lv_graph_optimise
    ctx.traj_set(rec.trajectory())
    ctx.traj_correct(offline.corrections(G, keyframe_times))
    ctx.traj_smooth(sigma=0.05, half_window=8, iterations=2)
    world = offline.remap(ctx, rec.sweeps, offline.extrinsic_of(rec.states[-1]))
"""
from __future__ import annotations

import numpy as np

from . import capi
from .graph import _pose
from .synth import quat_mul, quat_to_rot


def trajectory(states, times) -> np.ndarray:
    """TRAJ_KNOT_DTYPE knots from lv_state arrays (26 doubles each; position and rotation are used) and their times."""
    poses = np.array([_pose(s) for s in states]).reshape(-1, 7)
    times = np.asarray(times, np.float64).reshape(-1)
    if len(times) != len(poses):
        raise ValueError("one time per state")
    return capi.traj_knots(times, poses)


def extrinsic_of(state) -> np.ndarray:
    """(t [3], q [4]) of the LiDAR in the body from a state: offset_T_L_I, offset_R_L_I."""
    s = np.asarray(state, np.float64)
    q = s[7:11] / np.linalg.norm(s[7:11])
    return np.concatenate([s[11:14], q])


class Recorder:
    """Collects the stamped states of a run and, optionally, its raw sweeps."""

    def __init__(self, keep_sweeps: bool = False):
        self.times: list[float] = []
        self.states: list[np.ndarray] = []
        self.keep_sweeps = keep_sweeps
        self.sweeps: list[np.ndarray] = []

    def add_state(self, time: float, state):
        if self.times and not float(time) > self.times[-1]:
            raise ValueError(f"state at {time!r}: times must ascend (the last is {self.times[-1]!r})")
        self.times.append(float(time))
        self.states.append(np.array(state, np.float64))

    def add_sweep(self, points):
        """points: a structured array with x, y, z f32 first and an f64 field "time" (capi.POINT_DTYPE), in the LiDAR frame."""
        if self.keep_sweeps:
            self.sweeps.append(np.array(points))

    def trajectory(self) -> np.ndarray:
        return trajectory(self.states, self.times)


def corrections(graph, keyframe_times) -> np.ndarray:
    """The records lv_traj_correct takes from a solved graph.PoseGraph: D_k = T_now T_0^-1 of keyframe k (its pose in graph.poses
    against the pose of graph.states[k]) at keyframe_times[k].  A keyframe that has not moved gives the identity exactly."""
    if graph.poses is None:
        raise RuntimeError("optimise first")
    times = np.asarray(keyframe_times, np.float64).reshape(-1)
    if len(times) != len(graph.states):
        raise ValueError("one time per keyframe")
    D = np.zeros((len(times), 7))
    for k, (s, now) in enumerate(zip(graph.states, np.asarray(graph.poses, np.float64))):
        x0 = _pose(s)
        if np.array_equal(now, x0):
            D[k] = [0, 0, 0, 0, 0, 0, 1]
            continue
        q = quat_mul(now[3:], np.array([-x0[3], -x0[4], -x0[5], x0[6]]))
        q /= np.linalg.norm(q)
        D[k, :3] = now[:3] - quat_to_rot(q) @ x0[:3]
        D[k, 3:] = q
    return capi.traj_knots(times, D)


def remap(ctx, sweeps_or_windows, extrinsic=None, chunk: int = 1 << 20, extrapolate: int = capi.TRAJ_REFUSE) -> np.ndarray:
    """Registers every sweep against the context's trajectory and rebuilds the device map from the result.

    sweeps_or_windows: raw sweeps (structured arrays as Recorder.add_sweep takes them), or (t1, t2) windows of the device LiDAR
    buffer (lv_traj_register_cloud: the raw points stay on the device).  extrinsic: (t [3], q [4]) or None for the identity.
    Points the trajectory does not cover are dropped under the default LV_TRAJ_REFUSE, as are non-finite ones.  The first `chunk`
    points go through lv_map_build, the rest through lv_map_add(downsample=1), `chunk` at a time.  Returns the [M, 3] f32 points
    handed over, in order."""
    prm = capi.default_traj_register_params(extrapolate=extrapolate)
    if extrinsic is not None:
        e = np.asarray(extrinsic, np.float64).reshape(7)
        prm = capi.default_traj_register_params(extrapolate=extrapolate, ext_t=e[:3], ext_q=e[3:])
    parts = []
    for s in sweeps_or_windows:
        if isinstance(s, tuple) and len(s) == 2 and np.isscalar(s[0]):
            out, _, _ = ctx.traj_register_cloud(float(s[0]), float(s[1]), prm)
        else:
            out, _, _ = ctx.traj_register(s, prm)
        parts.append(out[np.all(np.isfinite(out), axis=1)])
    world = np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)
    for off in range(0, len(world), chunk):
        piece = world[off:off + chunk]
        if off == 0:
            ctx.map_build(piece)
        else:
            ctx.map_add(piece, downsample=True)
    return world
