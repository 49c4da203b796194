"""Seeded scenes for the NDT tests (TEST INFRASTRUCTURE): the targets, sources, guesses and truths that tests/test_ndt_ref.py,
tests/test_ndt_host.py and tests/test_gpu_ndt.py share, and the reference's answers, computed once per process.

The room: a floor (z = 0) and two walls (x = 0, y = 0) over 6 m x 6 m x 3 m with a 1 m box standing at (3..4, 3..4), sampled with
1 cm of noise; 8 x 8 x 4 voxels of 1 m from (-1, -1, -0.5), so that the surfaces run through the middle of their voxels."""
import functools
import math

import numpy as np

import graph_ref as gr
import ndt_ref as nr

F = np.float32
ROOM = nr.params(origin=(-1.0, -1.0, -0.5), resolution=1.0, nx=8, ny=8, nz=4, min_points=5, reg=0.01)
D2 = 0.43                       # the issue's prototype value
SOLVE = dict(search=7, d2=D2, max_iterations=60, step_tol=1e-7)
TRUTH = np.concatenate([[3.0, 2.5, 1.2], gr.quat_rpy(0.02, -0.03, 0.6)])


def room_points(rng, n, noise=0.01):
    """n points on the room's surfaces, by area"""
    faces = [((0, 0, 0), (6, 0, 0), (0, 6, 0)), ((0, 0, 0), (0, 6, 0), (0, 0, 3)), ((0, 0, 0), (6, 0, 0), (0, 0, 3)),   # floor, walls
             ((3, 3, 1), (1, 0, 0), (0, 1, 0)), ((3, 3, 0), (1, 0, 0), (0, 0, 1)), ((3, 4, 0), (1, 0, 0), (0, 0, 1)),   # box: top, sides
             ((3, 3, 0), (0, 1, 0), (0, 0, 1)), ((4, 3, 0), (0, 1, 0), (0, 0, 1))]
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in faces])
    which = rng.choice(len(faces), size=n, p=area / area.sum())
    o = np.array([faces[k][0] for k in which], float)
    u = np.array([faces[k][1] for k in which], float)
    v = np.array([faces[k][2] for k in which], float)
    return o + rng.uniform(size=(n, 1)) * u + rng.uniform(size=(n, 1)) * v + rng.normal(0, noise, (n, 3))


def to_frame(pose, world):
    """world points in the frame of pose [7]"""
    return (np.asarray(world, float) - pose[:3]) @ gr.rot(pose[3:])


def perturbed(rng, pose, dt, dth):
    """pose moved by a step of exactly |dt| metres and |dth| radians in random directions"""
    a, b = rng.normal(size=3), rng.normal(size=3)
    return gr.retract(pose, np.concatenate([dt * a / np.linalg.norm(a), dth * b / np.linalg.norm(b)]))


@functools.lru_cache(maxsize=None)
def room(seed=0):
    """(target [4000, 3] f32, source [400, 3] f32 in the sensor frame at TRUTH)"""
    rng = np.random.default_rng(seed)
    target = room_points(rng, 4000).astype(F)
    source = to_frame(TRUTH, room_points(rng, 400)).astype(F)
    return target, source


def _guesses(seed, dt, dth, k=8):
    rng = np.random.default_rng(1000 + seed)
    return np.array([perturbed(rng, TRUTH, dt, dth) for _ in range(k)])


def corner_near():
    t, s = room(4)
    return dict(prm=ROOM, target=t, source=s, guesses=_guesses(4, 0.3, math.radians(3.0)), truth=TRUTH, solve=SOLVE)


def corner_far():
    """1 m / 14 degrees off: rejected steps, and guesses that end in a local optimum at MAX_ITERATIONS"""
    t, s = room(1)
    return dict(prm=ROOM, target=t, source=s, guesses=_guesses(1, 1.0, math.radians(14.0)), truth=TRUTH, solve=SOLVE)


def corner_search1():
    t, s = room(5)
    return dict(prm=ROOM, target=t, source=s, guesses=_guesses(5, 0.2, math.radians(2.0)), truth=TRUTH, solve=dict(SOLVE, search=1))


def plane():
    """One plane (the floor alone): z, roll and pitch are observable; x, y and yaw are held by nothing but the voxels' own spread."""
    rng = np.random.default_rng(7)
    w = np.stack([rng.uniform(0, 6, 3000), rng.uniform(0, 6, 3000), rng.normal(0, 0.01, 3000)], axis=1)
    s = np.stack([rng.uniform(1.5, 4.5, 400), rng.uniform(1.5, 4.5, 400), rng.normal(0, 0.01, 400)], axis=1)
    g = np.array([gr.retract(TRUTH, np.array([0, 0, dz, rx, ry, 0.0])) for dz, rx, ry in
                  ((0.1, 0.02, 0.0), (-0.1, 0.0, 0.02), (0.15, -0.02, 0.02), (-0.15, 0.03, 0.0), (0.05, 0.0, -0.03), (0.2, 0.01, 0.01),
                   (-0.2, -0.01, 0.02), (0.12, 0.02, -0.02))])
    return dict(prm=ROOM, target=w.astype(F), source=to_frame(TRUTH, s).astype(F), guesses=g, truth=TRUTH, solve=dict(SOLVE, max_iterations=30))


ALIGN_CASES = {"corner-near": corner_near, "corner-far": corner_far, "corner-search1": corner_search1, "plane": plane}
NEAR = ("corner-near", "corner-search1")   # the cases whose guesses all lie in the basin of the truth


def coincident():
    """min_points coincident points in one voxel, one fewer in another: (prm, points)"""
    p = np.array([[2.3, 3.7, 1.1]] * 5 + [[4.2, 1.1, 0.3]] * 4, F)
    return ROOM, p


def dirty():
    """NaN, infinities, points outside the grid, points exactly on voxel faces and on the grid's own faces"""
    rng = np.random.default_rng(11)
    good = room_points(rng, 500).astype(F)
    faces = np.array([[2.0, 3.0, 0.5], [2.0, 3.0, 0.5], [3.0, 3.0, 1.5], [-1.0, -1.0, -0.5], [7.0, 2.0, 1.0], [2.0, 7.0, 1.0], [2.0, 2.0, 3.5],
                      [np.nextafter(F(7.0), F(0)), 2.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], F)
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e9, 0, 0], [-1.001, 0, 0], [0, 0, 3.6], [3e38, 3e38, 3e38]], F)
    pts = np.concatenate([good, faces, bad])
    return ROOM, pts[np.random.default_rng(12).permutation(len(pts))]


@functools.lru_cache(maxsize=None)
def target(name):
    c = ALIGN_CASES[name]()
    return nr.build(c["prm"], c["target"])


@functools.lru_cache(maxsize=None)
def reference(name, reverse=False):
    """(results, best) of the reference on a case, every guess"""
    c = ALIGN_CASES[name]()
    return nr.align(c["prm"], target(name), c["source"], c["guesses"], reverse=reverse, **c["solve"])
