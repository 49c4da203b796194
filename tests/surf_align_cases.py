"""The scenes of the surface-registration tests (TEST INFRASTRUCTURE): one analytic room corner as a TSDF volume of 48 x 40 x 32
voxels of 0.1 m, 513 source points on its three planes seen from a known pose, and the guesses of every case.  Seeded; nothing is
read from a file.  reference(name) runs tests/surf_align_ref.py once per case and session."""
import functools
import math

import numpy as np

import graph_ref as gr
import surf_align_ref as sr

F = np.float32
PARAMS = dict(origin=(-2.4, -2.0, -1.6), resolution=0.1, nx=48, ny=40, nz=32, min_range=0.1, max_range=20.0, trunc_cells=3, max_weight=10000, carve=0)
BAND = 768                                             # trunc_cells * 256
TRUTH = np.concatenate([[0.3, 0.2, 0.1], gr.qexp(np.array([0.1, -0.2, 0.3]))])
N_PLANE = 171
# max_dist inside the band of 0.3 m, so that the gate and the UNKNOWN corners both occur
SOLVE = dict(max_iterations=50, max_dist=0.25, huber=0.1)


def room_sdf(x, y, z):
    return np.minimum(np.minimum(z + 1.0, x + 1.5), y + 1.2)


def centres():
    """the voxel centres in f64 from the f32 origin and resolution, as [nz, ny, nx] arrays x, y, z"""
    o = np.asarray(PARAMS["origin"], F).astype(np.float64)
    r = float(F(PARAMS["resolution"]))
    k, j, i = np.meshgrid(np.arange(PARAMS["nz"]), np.arange(PARAMS["ny"]), np.arange(PARAMS["nx"]), indexing="ij")
    return o[0] + (i + 0.5) * r, o[1] + (j + 0.5) * r, o[2] + (k + 0.5) * r


@functools.lru_cache(maxsize=None)
def volume(weights=False):
    """the room corner: q = floor(sdf / res * 256) at every voxel centre, W = 1 and S = q where |q| <= 768, W = 0 elsewhere.
    weights: W random in 1..5 (mostly 3..5) with S = q W, so that min_weight = 3 leaves UNKNOWN corners inside the band"""
    x, y, z = centres()
    q = np.floor(room_sdf(x, y, z) / float(F(PARAMS["resolution"])) * 256.0).astype(np.int64)
    seen = np.abs(q) <= BAND
    W = seen.astype(np.int32)
    if weights:
        W = W * np.random.default_rng(5).choice(np.arange(1, 6), size=W.shape, p=[0.02, 0.02, 0.32, 0.32, 0.32]).astype(np.int32)
    S = np.where(seen, q * W, 0).astype(np.int32)
    return dict(origin=PARAMS["origin"], resolution=PARAMS["resolution"], nx=PARAMS["nx"], ny=PARAMS["ny"], nz=PARAMS["nz"], S=S, W=W)


LINEAR = dict(PARAMS, origin=(-3.0, -2.5, -2.0), resolution=0.125)      # binary fractions: a point's u is exact
LINEAR_COEF, LINEAR_OFFSET = (3, -2, 5), -100


def linear_volume():
    """S linear in the voxel index, unclamped (|S| <= 768), W = 1: the interpolant is the field itself"""
    k, j, i = np.meshgrid(np.arange(LINEAR["nz"]), np.arange(LINEAR["ny"]), np.arange(LINEAR["nx"]), indexing="ij")
    S = (LINEAR_COEF[0] * i + LINEAR_COEF[1] * j + LINEAR_COEF[2] * k + LINEAR_OFFSET).astype(np.int32)
    return dict(origin=LINEAR["origin"], resolution=LINEAR["resolution"], nx=LINEAR["nx"], ny=LINEAR["ny"], nz=LINEAR["nz"], S=S, W=np.ones_like(S))


def exact_points(rng, n):
    """(points [n, 3] f32 in LINEAR's box, u [n, 3]): u = i + f with f a multiple of 1/256, a quarter of them with f = 0 (cell
    faces), i in 0 .. n_a - 2; both exact in f32"""
    dims = np.array([LINEAR["nx"], LINEAR["ny"], LINEAR["nz"]])
    i = rng.integers(0, dims - 1, (n, 3))
    f = rng.integers(0, 256, (n, 3)) / 256.0
    f[::4] = 0.0
    u = i + f
    pts = np.asarray(LINEAR["origin"], float) + (u + 0.5) * LINEAR["resolution"]
    assert np.array_equal(pts.astype(F).astype(float), pts)
    return pts.astype(F), u


def plane_points(rng, n):
    """n world points on each of the floor (z = -1), the wall x = -1.5 and the wall y = -1.2, over the whole of each plane inside
    the box.  Near the creases the interpolant of min() is not the plane's distance, and the last half voxel before a box face
    has no eight corners (OUTSIDE: the gate charge), so the cost at the optimum is far from zero: a cost that vanishes cannot
    be held to a relative bound (a pose that moves by 1e-16 moves it by 1e-10 of itself)."""
    floor = np.stack([rng.uniform(-1.5, 2.4, n), rng.uniform(-1.2, 2.0, n), np.full(n, -1.0)], axis=1)
    wall_x = np.stack([np.full(n, -1.5), rng.uniform(-1.2, 2.0, n), rng.uniform(-1.0, 1.6, n)], axis=1)
    wall_y = np.stack([rng.uniform(-1.5, 2.4, n), np.full(n, -1.2), rng.uniform(-1.0, 1.6, n)], axis=1)
    return floor, wall_x, wall_y


def to_frame(pose, world):
    """world points in the sensor frame of `pose`"""
    return (np.asarray(world, float) - pose[:3]) @ gr.rot(pose[3:])


@functools.lru_cache(maxsize=None)
def source():
    """513 source points (f32, sensor frame of TRUTH): the 171 of the floor first"""
    return to_frame(TRUTH, np.concatenate(plane_points(np.random.default_rng(11), N_PLANE))).astype(F)


def offset(dt, dr):
    return gr.compose(TRUTH, np.asarray(dt, float), gr.qexp(np.asarray(dr, float)))


@functools.lru_cache(maxsize=None)
def guesses():
    """the truth, three offsets of up to 0.12 m and 0.08 rad, one guess 50 m away"""
    far = TRUTH.copy()
    far[0] += 50.0
    return np.stack([TRUTH, offset((0.05, -0.03, 0.04), (0.02, 0.01, -0.03)), offset((-0.12, 0.08, -0.06), (-0.05, 0.08, 0.04)),
                     offset((0.08, 0.12, 0.10), (0.08, -0.06, -0.07)), far])


def corner():
    return dict(vol=volume(), source=source(), guesses=guesses(), solve=dict(SOLVE))


def floor():
    return dict(vol=volume(), source=source()[:N_PLANE], guesses=guesses()[:4], solve=dict(SOLVE))


def huber0():
    return dict(vol=volume(), source=source(), guesses=guesses(), solve=dict(SOLVE, huber=0.0))


def weights():
    return dict(vol=volume(True), source=source(), guesses=guesses(), solve=dict(SOLVE, min_weight=3))


CASES = {"corner": corner, "floor": floor, "huber0": huber0, "weights": weights}


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASES[name]()
    return sr.align(c["vol"], c["source"], c["guesses"], **c["solve"])


def check_best(best, results, name):
    """best [2] of an implementation whose `results` (records with cost, n_in, status) it was taken from, against the reference of
    case `name`.  It must be what the rule makes of the implementation's own costs, exactly; and it must be the reference's
    best, unless the reference's least cost is a tie within the 1e-9 relative the costs themselves are held to (guesses that
    reach one optimum end at costs a few ulp apart): then any hypothesis of that tie is right."""
    ref, ref_best = reference(name)
    own = (-1, -1)
    for k, r in enumerate(results):
        if int(r["status"]) != sr.NO_OVERLAP and (own[0] < 0 or r["cost"] < results[own[0]]["cost"]):
            own = (k, int(r["n_in"]))
    assert tuple(best) == own, (best, own)
    live = [k for k, r in enumerate(ref) if r["status"] != sr.NO_OVERLAP]
    least = min(ref[k]["cost"] for k in live)
    tie = [k for k in live if ref[k]["cost"] <= least * (1 + 1e-9)]
    assert (tuple(best) == ref_best) if len(tie) == 1 else (best[0] in tie and best[1] == ref[best[0]]["n_in"]), (best, ref_best, tie)
    return len(tie) == 1


def sample_points(rng, n=4096):
    """[n, 3] f32 world points for the sample: inside the band, on cell faces (f = 0), at i = n - 2 and i = n - 1, outside, NaN and
    inf, next to W = 0 voxels"""
    o = np.asarray(PARAMS["origin"], F).astype(np.float64)
    r = float(F(PARAMS["resolution"]))
    dims = np.array([PARAMS["nx"], PARAMS["ny"], PARAMS["nz"]], float)
    m = n // 8
    floor, wall_x, wall_y = plane_points(rng, m)
    near = np.concatenate([floor, wall_x, wall_y]) + rng.normal(0, 0.12, (3 * m, 3))           # inside the band and at its edge (W = 0 next door)
    faces = o + (np.floor((near[:m] - o) / r - 0.5) + 0.5) * r                                   # voxel centres: f = 0 up to the f32 rounding,
    faces[: m // 2, 1:] += rng.uniform(0, r, (m // 2, 2))                                        # on every axis or on one (exact: exact_points)
    edge = o + rng.uniform(0, 1, (m, 3)) * dims * r
    ax = rng.integers(0, 3, m)
    edge[np.arange(m), ax] = (o + (dims - rng.choice([1.5, 1.0, 0.5, 0.49, 1.51], m)[:, None]) * r)[np.arange(m), ax]   # i = n - 2, n - 1
    low = o + rng.uniform(0, 1, (m, 3)) * dims * r
    low[np.arange(m), ax] = (o + rng.choice([0.5, 0.49, 0.0, 1.0], m)[:, None] * r)[np.arange(m), ax]                  # i = 0 and i = -1
    outside = o + rng.uniform(-0.5, 1.5, (m, 3)) * dims * r
    odd = rng.uniform(-1, 1, (n - 7 * m, 3))
    odd[::4, 0], odd[1::4, 1], odd[2::4, 2], odd[3::4, 0] = math.nan, math.inf, -math.inf, 1e30
    return np.concatenate([near, faces, edge, low, outside, odd]).astype(F)


# ---- the end-to-end scene: a depth camera in the room, looking into the corner
CAMERA = dict(fx=80.0, fy=80.0, cx=47.5, cy=35.5, width=96, height=72)
TRACK_RANGE = 8.0      # the rays' length: the room is 5 m across


def look_at(position, target):
    """(R [3, 3] f32 camera -> world, t [3] f32) of a camera (z forward, x right, y down) at `position` looking at `target`, world z up"""
    z = np.asarray(target, float) - np.asarray(position, float)
    z /= np.linalg.norm(z)
    x = np.cross(z, (0.0, 0.0, 1.0))
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1).astype(F), np.asarray(position, F)


def track_poses():
    """nine camera poses: eight to fuse from, the ninth to track"""
    rng = np.random.default_rng(17)
    return [look_at((1.1, 0.9, 0.5) + rng.uniform(-0.35, 0.35, 3), (-1.0, -0.8, -0.7) + rng.uniform(-0.3, 0.3, 3)) for _ in range(9)]


def track_guess(R, t):
    """(R, t) 0.08 m and 0.05 rad off the pose (R, t)"""
    dr = 0.05 * np.array([0.6, -0.64, 0.48])
    dt = 0.08 * np.array([-0.48, 0.6, 0.64])
    return np.asarray(R, float) @ gr.rot(gr.qexp(dr)), np.asarray(t, float) + dt


def rotation_angle(Ra, Rb):
    c = (np.trace(np.asarray(Ra, float).T @ np.asarray(Rb, float)) - 1.0) / 2.0
    return float(math.acos(min(1.0, max(-1.0, c))))
