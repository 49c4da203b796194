"""tests/lattice_ref.py against itself and against tests/plan_ref.py: its two solvers (a heapq Dijkstra on the reversed graph, whole-array
sweeps to the fixpoint) agree on random grids and tables, and with one heading and the planner's eight moves as primitives it is the
planner.  Equality, no tolerance."""
import numpy as np
import pytest

import lattice_ref as lr
import occupancy_ref as ocr
import plan_ref as pr

F = np.float32
TABLE6 = np.array([254, 180, 110, 70, 55, 50], np.uint8)


def _cost(rng, shape, density, table=TABLE6):
    return pr.cell_cost(pr.random_s2(rng, shape, density), 1, table)


def _centre(prm, i, j, h):
    return [prm["origin"][0] + (i + 0.5) * prm["resolution"], prm["origin"][1] + (j + 0.5) * prm["resolution"], 0.0, h]


@pytest.mark.parametrize("dims,H,P,reach", [((12, 9), 4, 3, 2), ((23, 17), 8, 5, 3), ((9, 30), 16, 2, 8), ((1, 14), 3, 4, 5), ((1, 1), 2, 2, 1)])
def test_dijkstra_equals_the_sweeps(dims, H, P, reach):
    nx, ny = dims
    rng = np.random.default_rng(nx * 31 + ny + H)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=1)
    seen = 0
    for density in (0.0, 0.1, 0.3):
        c = _cost(rng, (ny, nx), density)
        t = lr.random_table(rng, H, P, reach)
        assert lr.check_table(H, P, t) is None
        goals = lr.poses([_centre(prm, int(rng.integers(nx)), int(rng.integers(ny)), h) for h in (-1, 0, H - 1, H)] + [[np.nan, 0, 0, 0]])
        V, st = lr.build(prm, c, t, goals)
        W, st2 = lr.build(prm, c, t, goals, solver=lr.sweep_fixpoint)
        assert np.array_equal(V, W) and list(st) == list(st2)
        assert np.all(V[:, c == 0] == lr.UNREACHED)
        seen += int(st[2])
        # every reached state walks to a goal at exactly its cost
        starts = lr.poses([_centre(prm, i, j, -1) for j in range(ny) for i in range(nx)])
        status, cost, off, states, taken = lr.paths(prm, c, V, t, starts)
        for s in np.flatnonzero(status == 0):
            row, tk = states[int(off[s]):int(off[s + 1])], taken[int(off[s]):int(off[s + 1])]
            assert V.reshape(-1)[row[-1]] == 0 and tk[-1] == 255 and np.all(tk[:-1] < P) and V.reshape(-1)[row[0]] == cost[s]
    assert seen > 0


@pytest.mark.parametrize("dims", [(12, 9), (33, 5), (1, 6), (34, 34)])
def test_one_heading_and_eight_moves_is_the_planner(dims):
    nx, ny = dims
    rng = np.random.default_rng(nx + 5 * ny)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=1)
    t = lr.neighbour_table()
    for density in (0.0, 0.2, 0.45):
        s2 = pr.random_s2(rng, (ny, nx), density)
        pts = np.array([_centre(prm, int(rng.integers(nx)), int(rng.integers(ny)), 0)[:3] for _ in range(3)], F)
        c, P, st, _ = pr.build(prm, s2, pr.pparams(connectivity=8), TABLE6, pts)
        goals = lr.poses(np.concatenate([pts, np.zeros((3, 1))], axis=1))
        V, lst = lr.build(prm, c, t, goals)
        # (that graph is symmetric: the cost to go equals the cost from)
        assert np.array_equal(V[0], P) and list(lst) == list(st)


def test_the_table_check():
    t = lr.table(2, 2)
    assert lr.check_table(2, 2, t) == (None, "empty")
    t[0, 0] = lr.prim(1, 0, 0, 10)
    assert lr.check_table(2, 2, t) is None and lr.reach_of(t) == 1
    assert lr.check_table(0, 2, t)[1] == "H" and lr.check_table(2, 17, t)[1] == "P" and lr.check_table(2, 3, t)[1] == "n_prims"
    for field, value, why in (("di", 9, "di, dj"), ("dj", -9, "di, dj"), ("h_to", 2, "h_to"), ("n_sweep", 11, "n_sweep"), ("reserved", 1, "reserved"),
                              ("penalty", (1 << 24) + 1, "penalty")):
        b = t.copy()
        b[1, 1][field] = value
        assert lr.check_table(2, 2, b) == (3, why), field
    b = t.copy()
    b[1, 0]["sweep"][9] = (0, 1)
    assert lr.check_table(2, 2, b) == (2, "sweep unused")
    b[1, 0]["n_sweep"] = 10
    assert lr.check_table(2, 2, b) is None
    b[1, 0]["sweep"][0] = (-9, 0)
    assert lr.check_table(2, 2, b) == (2, "sweep")
    b = t.copy()
    b[1, 1] = lr.prim(0, 0, 1, 10)
    assert lr.check_table(2, 2, b) == (3, "self loop")
    b[1, 1] = lr.prim(0, 0, 0, 10)   # a turn on the spot
    assert lr.check_table(2, 2, b) is None
    b[1, 1] = lr.prim(0, 0, 1, 0)    # an empty slot is no loop
    assert lr.check_table(2, 2, b) is None
