"""tests/plan_ref.py against itself: the heapq Dijkstra equals the naive relax-until-nothing-changes statement of the rule, a path's
summed edge costs equal the potential of its start, no path cuts a corner, and (where scipy is installed) the potential equals
scipy.sparse.csgraph.dijkstra on the same graph."""
import numpy as np
import pytest

import occupancy_ref as ocr
import plan_ref as pr

F = np.float32
TABLE = np.array([200, 120, 60, 51, 50], np.uint8)
CASES = [((7, 9), 8), ((7, 9), 4), ((1, 6), 8), ((3, 5, 6), 6), ((3, 5, 6), 18), ((3, 5, 6), 26), ((1, 1, 4), 26), ((1, 1), 4)]


def _case(shape, conn, density=0.3, seed=0):
    rng = np.random.default_rng(seed + 11 * len(shape) + conn)
    dims = shape[::-1] + ((1,) if len(shape) == 2 else ())
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=dims[0], ny=dims[1], nz=dims[2])
    s2 = pr.random_s2(rng, shape, density)
    lo = np.array(prm["origin"])
    pts = (lo + rng.uniform(0, 1, (12, 3)) * np.array(dims) * 0.25).astype(F)
    return prm, s2, pr.pparams(connectivity=conn), pts[:3], pts


@pytest.mark.parametrize("shape,conn", CASES)
def test_dijkstra_equals_the_naive_fixpoint(shape, conn):
    for density in (0.0, 0.3, 0.5):
        prm, s2, pp, goals, _ = _case(shape, conn, density)
        c, P, st, adj = pr.build(prm, s2, pp, TABLE, goals)
        ok, v = pr.cells_of(prm, (c[None] if c.ndim == 2 else c).shape, c.ndim == 2, goals)
        c3 = c[None] if c.ndim == 2 else c
        used = [(k * c3.shape[1] + j) * c3.shape[2] + i for (i, j, k), o in zip(v, ok) if o and c3[k, j, i]]
        assert np.array_equal(P.reshape(-1), pr.relax_fixpoint(c.size, adj, used))
        assert st[0] == len(used) and st[1] == np.count_nonzero(c) and st[2] == np.sum(P != pr.UNREACHED)
        assert np.all(P[c == 0] == pr.UNREACHED)


@pytest.mark.parametrize("shape,conn", CASES)
def test_paths_sum_to_the_potential_and_cut_no_corner(shape, conn):
    prm, s2, pp, goals, starts = _case(shape, conn, 0.25, seed=3)
    c, P, _, adj = pr.build(prm, s2, pp, TABLE, goals)
    status, cost, off, cells = pr.paths(prm, c, P, adj, starts)
    c3 = c[None] if c.ndim == 2 else c
    nz, ny, nx = c3.shape
    Pf = P.reshape(-1)
    for s in range(len(starts)):
        row = cells[int(off[s]):int(off[s + 1])]
        if status[s] != 0:
            assert len(row) == 0 and cost[s] == pr.UNREACHED
            continue
        assert Pf[row[0]] == cost[s] and Pf[row[-1]] == 0
        total = 0
        for u, w in zip(row[:-1], row[1:]):
            iu, iw = np.array([u % nx, (u // nx) % ny, u // (nx * ny)]), np.array([w % nx, (w // nx) % ny, w // (nx * ny)])
            d = iw - iu
            m = int(np.count_nonzero(d))
            assert np.all(np.abs(d) <= 1) and 1 <= m <= pr.MAX_M[conn]
            assert pr.allowed(c3, *iu, *d)
            for a in range(3):   # every single-component step of a diagonal lands on a traversable cell
                if d[a] and m > 1:
                    e = iu.copy()
                    e[a] += d[a]
                    assert c3[e[2], e[1], e[0]] != 0
            total += pr.WEIGHT[m] * (int(c3.reshape(-1)[u]) + int(c3.reshape(-1)[w]))
        assert total == cost[s]


def test_cell_cost_rule():
    s2 = np.array([-pr.FAR, -4, 0, 1, 3, 4, 8, 9, 15, 16, 10 ** 6, pr.FAR], np.int32)
    assert list(pr.cell_cost(s2, 1, TABLE)) == [0, 0, 0, 120, 120, 60, 60, 51, 51, 50, 50, 50]
    assert list(pr.cell_cost(s2, 5, TABLE)) == [0, 0, 0, 0, 0, 0, 60, 51, 51, 50, 50, 50]
    assert list(pr.cell_cost(s2, 1, TABLE[:1])) == [0, 0, 0] + [200] * 9


def test_overflow_is_dropped():
    # a corridor of 255-cost cells long enough to pass 2^32: not buildable here, so the rule is held on a hand-made graph
    adj = {0: [(1, 0xFFFFFFF0)], 1: [(0, 0xFFFFFFF0), (2, 14), (3, 15)], 2: [(1, 14)], 3: [(1, 15)]}
    P = pr.dijkstra(4, adj, [0])
    assert list(P) == [0, 0xFFFFFFF0, 0xFFFFFFFE, pr.UNREACHED] and list(pr.relax_fixpoint(4, adj, [0])) == list(P)


@pytest.mark.parametrize("shape,conn", CASES)
def test_against_scipy(shape, conn):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra

    prm, s2, pp, goals, _ = _case(shape, conn, 0.3, seed=5)
    c, P, _, adj = pr.build(prm, s2, pp, TABLE, goals)
    goal_cells = np.nonzero(P.reshape(-1) == 0)[0]
    if len(goal_cells) == 0:
        assert np.all(P == pr.UNREACHED)
        return
    rows = [u for u, lst in adj.items() for _ in lst]
    cols = [v for lst in adj.values() for v, _ in lst]
    w = [e for lst in adj.values() for _, e in lst]
    g = sp.csr_matrix((np.array(w, np.float64), (rows, cols)), shape=(c.size, c.size))
    d = dijkstra(g, directed=True, indices=goal_cells, min_only=True)
    want = np.where(np.isfinite(d), d, pr.UNREACHED).astype(np.uint32)
    assert np.array_equal(P.reshape(-1), want)
