"""The shared cases of the elevation map's tests (tests/test_elevation_host.py on the host, tests/test_gpu_elevation.py on the GPU):
small point sets on a 19 x 13 grid of 0.5 m cells with origin (-1, -2, -3), each built to make one clause of the rule of
include/limovelo_hip.h "Elevation map" decide, and a 70 x 37 scene of 0.2 m cells (about 67 k points, fixed seed): a noisy plane, a
12 degree ramp, a 0.15 m kerb, a 3 m wall, a canopy at 3..4 m, a 0.7 m table and a hole.  The answers come from
tests/elevation_ref.py, computed once."""
import functools
import math

import numpy as np

import elevation_ref as er

F = np.float32
ORIGIN, RES, NX, NY = (-1.0, -2.0, -3.0), 0.5, 19, 13


def prm(**kw):
    return er.params(**{**dict(origin=ORIGIN, resolution=RES, nx=NX, ny=NY, min_points=1, head=768, max_span=50, max_step=60, max_slope2=20000), **kw})


def at(i, j, z, fx=0.5, fy=0.5):
    """A world point in cell (i, j) (fx, fy of the way across it) whose height quantises to z sub-units (exact in f32 for the
    small z of these cases: every term is a multiple of 2^-10)."""
    return [ORIGIN[0] + (i + fx) * RES, ORIGIN[1] + (j + fy) * RES, ORIGIN[2] + (z + 0.5) / 256.0 * RES]


def block(cells, z, count=1):
    """`count` points at height z in each of cells [(i, j)]."""
    return [at(i, j, z) for (i, j) in cells for _ in range(count)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (params, points [n, 3] f32)."""
    out = {}
    # points exactly on cell borders, on the grid's low faces (inside) and high faces (outside), corners included
    xs = [ORIGIN[0] + i * RES for i in range(NX + 1)]
    ys = [ORIGIN[1] + j * RES for j in range(NY + 1)]
    out["borders"] = (prm(), np.array([[x, y, ORIGIN[2] + 0.25 * k] for k, (x, y) in enumerate((x, y) for x in xs for y in ys)] +
                                      [[xs[0] - 1e-6, ys[3], 0.0], [xs[3], ys[0] - 1e-6, 0.0], [np.nextafter(F(xs[-1]), F(-100)), ys[2], 0.0],
                                       [xs[2], np.nextafter(F(ys[-1]), F(-100)), 0.0]], F))
    # negative heights: below origin[2]
    out["negative_z"] = (prm(), np.array(block([(3, 3), (4, 3), (3, 4)], -700) + block([(4, 4)], -1) + block([(5, 4)], 0) +
                                         [at(3, 3, -900), at(4, 4, -256 * 40)], F))
    # NaN / inf in each coordinate, a coordinate beyond 2^24 sub-units (32768 m at this resolution), beside points that count
    bad = []
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf, 40000.0, -40000.0):
            p = at(6, 6, 10)
            p[a] = v
            bad.append(p)
    far_ok = at(6, 6, 10)
    far_ok[2] = 32000.0   # (still below 2^24 sub-units: an overhang point)
    out["nonfinite"] = (prm(), np.array(bad + [far_ok] + block([(6, 6), (7, 6)], 10, 2), F))
    # exactly min_points - 1, exactly min_points, and min_points of which one is overhang
    out["min_points"] = (prm(min_points=3), np.array(block([(2, 2)], 5, 2) + block([(3, 2)], 5, 3) + block([(4, 2)], 5, 2) + [at(4, 2, 5 + 769)] +
                                                     block([(2, 3), (3, 3), (4, 3)], 9, 3), F))
    # z - lo exactly head, and head + 1; then head = 0
    pts = block([(8, 8)], 100) + [at(8, 8, 100 + 768)] + block([(9, 8)], 100) + [at(9, 8, 100 + 769)] + block([(10, 8)], 100, 2) + [at(10, 8, 101)]
    out["head"] = (prm(), np.array(pts, F))
    out["head0"] = (prm(head=0), np.array(pts, F))
    # a known cell with no known neighbour (the cells round it hold too few points), one with only +x, one with only -x
    out["neighbours"] = (prm(min_points=2), np.array(block([(3, 9)], 40, 2) + block([(2, 9), (4, 9), (3, 8), (3, 10), (2, 8), (4, 10)], 400, 1) +
                                                     block([(8, 3)], 10, 2) + block([(9, 3)], 31, 2) + [at(9, 3, 33)] + block([(14, 3)], 10, 2) + block([(13, 3)], -20, 2) +
                                                     block([(8, 10)], 10, 2) + block([(8, 11)], 31, 2) + block([(12, 11)], 10, 2) + block([(12, 10)], 55, 2), F))
    # known cells in each corner of the grid, with and without known neighbours
    corners = [(0, 0), (NX - 1, 0), (0, NY - 1), (NX - 1, NY - 1)]
    out["corners"] = (prm(), np.array(block(corners, 20) + block([(1, 0), (1, 1), (NX - 2, NY - 1), (NX - 1, NY - 2), (0, NY - 2)], 45) +
                                      block([(NX - 2, 1)], -30), F))
    # a slope2 that saturates: two cells 2^24 sub-units apart
    lo_z, hi_z = -(2 ** 23) + 5000, 2 ** 23 - 5000
    out["saturate"] = (prm(head=2 ** 25, max_span=2 ** 25, max_step=2 ** 25, max_slope2=2 ** 31 - 1),
                       np.array([at(5, 5, 0), [at(6, 5, 0)[0], at(6, 5, 0)[1], ORIGIN[2] + hi_z / 256.0 * RES],
                                 [at(4, 5, 0)[0], at(4, 5, 0)[1], ORIGIN[2] + lo_z / 256.0 * RES], at(5, 6, 0), at(11, 11, 3)], F))
    # thresholds hit exactly (not lethal), then by one more sub-unit (lethal).  span: cells (1..2, 1); step: (5..8, 1) with the
    # slope's threshold out of the way; slope2 = 100^2 against 100^2 + 1: cells (11..13, 5) and (11..13, 9)
    t = prm(max_span=50, max_step=60, max_slope2=2 ** 31 - 1)
    out["span_step"] = (t, np.array(block([(1, 1)], 0) + [at(1, 1, 50)] + block([(2, 4)], 0) + [at(2, 4, 51)] +
                                    block([(5, 1)], 0) + block([(6, 1)], 60) + block([(8, 4)], 0) + block([(9, 4)], 61), F))
    s = prm(max_span=2 ** 25, max_step=2 ** 25, max_slope2=10000)
    out["slope"] = (s, np.array(block([(11, 5)], 0) + block([(12, 5)], 50) + block([(13, 5)], 100) +
                                block([(11, 9)], 0) + block([(12, 9)], 50) + block([(13, 9)], 100) + block([(12, 10)], 50) + block([(12, 8)], 49) +
                                block([(3, 5)], 0) + block([(4, 5)], 50) + block([(3, 9)], 0) + block([(4, 9)], 51), F))
    # many points everywhere: several per cell at scattered heights, some cells empty, some points outside
    rng = np.random.default_rng(5)
    xy = rng.uniform([ORIGIN[0] - 0.7, ORIGIN[1] - 0.7], [ORIGIN[0] + NX * RES + 0.7, ORIGIN[1] + NY * RES + 0.7], (1500, 2))
    keep = ~((xy[:, 0] > 3.0) & (xy[:, 0] < 4.5) & (xy[:, 1] > 0.0) & (xy[:, 1] < 1.5))
    z = ORIGIN[2] + 0.05 * xy[:, 0] + rng.choice([0.0, 0.0, 0.0, 0.3, 2.5], len(xy)) + rng.normal(0, 0.02, len(xy))
    out["random"] = (prm(min_points=2, head=1024, max_span=80, max_step=40, max_slope2=3000), np.column_stack([xy, z])[keep].astype(F))
    return out


@functools.lru_cache(maxsize=None)
def answers():
    """name -> (layers, stats) of tests/elevation_ref.py."""
    return {name: er.build(p, pts) for name, (p, pts) in cases().items()}


# ---- the scene: 70 x 37 cells of 0.2 m, x in [-7, 7), y in [-3.7, 3.7), heights from -1
SCENE_ORIGIN, SCENE_RES, SCENE_NX, SCENE_NY = (-7.0, -3.7, -1.0), 0.2, 70, 37
WALL_I = 20                      # the wall stands in cell column 20: x in [-3.0, -2.8)
RAMP_X0, RAMP_DEG = 3.0, 12.0    # the ramp rises from x = 3 to the grid's edge over every y below the kerb's strip
KERB = (-2.0, 2.6, 2.4)          # the pavement: x in [-2.0, 2.6), y >= 2.4, raised by 0.15 m
TABLE = (0.6, 1.4, -2.6, -1.8)   # x0, x1, y0, y1: its top at 0.7 m
CANOPY = (1.0, 2.6, 0.6, 2.2)    # leaves at 3..4 m over flat ground
HOLE = (-1.6, -1.0, -2.8, -2.2)  # no points at all


def scene_params(**kw):
    r = SCENE_RES
    return er.params(**{**dict(origin=SCENE_ORIGIN, resolution=r, nx=SCENE_NX, ny=SCENE_NY, min_points=3, head=er.sub_units(1.5, r),
                               max_span=er.sub_units(0.12, r), max_step=er.sub_units(0.10, r),
                               max_slope2=int(math.floor((512 * math.tan(math.radians(20.0))) ** 2))), **kw})


def ground_z(x, y):
    z = np.where(x >= RAMP_X0, (x - RAMP_X0) * math.tan(math.radians(RAMP_DEG)), 0.0)
    return z + np.where((x >= KERB[0]) & (x < KERB[1]) & (y >= KERB[2]), 0.15, 0.0)


def _inside(x, y, box):
    return (x >= box[0]) & (x < box[1]) & (y >= box[2]) & (y < box[3])


@functools.lru_cache(maxsize=None)
def scene():
    """[n, 3] f32, about 67 k points."""
    rng = np.random.default_rng(20)
    x0, y0 = SCENE_ORIGIN[0], SCENE_ORIGIN[1]
    x1, y1 = x0 + SCENE_NX * SCENE_RES, y0 + SCENE_NY * SCENE_RES
    n = 56000
    x, y = rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)
    z = ground_z(x, y) + np.clip(rng.normal(0.0, 0.005, n), -0.015, 0.015)
    parts = [np.column_stack([x, y, z])[~_inside(x, y, HOLE)]]
    m = 3700   # the wall: 100 points per row of cells, from the floor to 3 m
    wy = np.repeat(y0 + (np.arange(SCENE_NY) + 0.5) * SCENE_RES, 100) + rng.uniform(-0.09, 0.09, m)
    parts.append(np.column_stack([rng.uniform(-2.98, -2.82, m), wy, rng.uniform(0.0, 3.0, m)]))
    m = 5000   # the canopy
    parts.append(np.column_stack([rng.uniform(CANOPY[0], CANOPY[1], m), rng.uniform(CANOPY[2], CANOPY[3], m), rng.uniform(3.0, 4.0, m)]))
    m = 2400   # the table top
    parts.append(np.column_stack([rng.uniform(TABLE[0], TABLE[1], m), rng.uniform(TABLE[2], TABLE[3], m), 0.7 + rng.normal(0.0, 0.003, m)]))
    pts = np.vstack(parts)
    return pts[rng.permutation(len(pts))].astype(F)


@functools.lru_cache(maxsize=None)
def scene_answer():
    return er.build(scene_params(), scene())


def scene_cell(x, y):
    return int(math.floor((x - SCENE_ORIGIN[0]) / SCENE_RES)), int(math.floor((y - SCENE_ORIGIN[1]) / SCENE_RES))
