"""The planner's rule (include/limovelo_hip.h "Planner") in numpy and plain Python: what tests/test_plan_host.py holds the host
build of lv_plan.hpp to and tests/test_gpu_occ_plan.py the kernels, cell for cell.

  cell cost   s = s2(v).  Blocked (c = 0) iff s < min_clear_s2.  Otherwise t = n_cost - 1 if s == FAR else min(isqrt(s), n_cost - 1)
              and c = table[t] (uint8, every entry 1..255); isqrt the exact integer floor square root.
  moves       offsets (dx, dy, dz) in {-1, 0, 1}^3 without 0, m non-zero components; connectivity 4 / 6: m = 1, 8 / 18: m <= 2,
              26: m <= 3; planar fields take 4 or 8 (dz = 0), 3-D fields 6, 18 or 26.  u -> v is allowed iff u, v and every cell
              u + (a proper non-empty subset of the move's non-zero components) are in the field and traversable.
  edge        w(m) * (c(u) + c(v)), w = 10, 14, 17.
  potential   P(v) = least total edge cost from any goal cell, 0 on goal cells, as uint32; UNREACHED = 0xFFFFFFFF for blocked and
              disconnected cells and for a cost that would reach 0xFFFFFFFF.
  goals       world points quantised as lv_occ_query does (occupancy_ref.quant_f, then >> 8; planar: z unused); non-finite ones,
              ones outside the field and ones in blocked cells are ignored.  goals used counts the points that are not.
  path        status 2: start non-finite, outside or blocked; 1: P unreached; 0: the cells from the start to a cell with P = 0, the
              next cell being the first v (lexicographic in (dz, dy, dx), each -1, 0, 1) with u -> v allowed and
              P(v) + edge(u, v) == P(u).
Everything is integer arithmetic and is compared by equality.  A heapq Dijkstra gives P; relax_fixpoint is the naive statement."""
import heapq
import math

import numpy as np

import occupancy_ref as ocr

F = np.float32
FAR = 2147483647
UNREACHED = 0xFFFFFFFF
WEIGHT = {1: 10, 2: 14, 3: 17}
MAX_M = {4: 1, 6: 1, 8: 2, 18: 2, 26: 3}
MAX_CLEAR = 3 * 1023 * 1023


def pparams(**kw):
    """A plain dict of lv_plan_params (the defaults, overridden by kw)."""
    p = dict(connectivity=8, min_clear_s2=1)
    p.update(kw)
    return p


def cell_cost(s2, min_clear_s2, table):
    """uint8, the shape of s2: the cost byte per cell, 0 = blocked."""
    s = np.asarray(s2, np.int64)
    table = np.asarray(table, np.uint8)
    n = len(table)
    r = np.array([math.isqrt(int(v)) if 0 <= v < FAR else 0 for v in s.reshape(-1)], np.int64).reshape(s.shape)
    t = np.where(s == FAR, n - 1, np.minimum(r, n - 1))
    return np.where(s < min_clear_s2, 0, table[t]).astype(np.uint8)


def moves(connectivity, planar):
    """[(dx, dy, dz, m)] in lexicographic order of (dz, dy, dx)."""
    out = []
    for dz in ((0,) if planar else (-1, 0, 1)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m = (dx != 0) + (dy != 0) + (dz != 0)
                if 0 < m <= MAX_M[connectivity]:
                    out.append((dx, dy, dz, m))
    return out


def _trav(c, i, j, k):
    nz, ny, nx = c.shape
    return 0 <= i < nx and 0 <= j < ny and 0 <= k < nz and c[k, j, i] != 0


def allowed(c, i, j, k, dx, dy, dz):
    """The move (i, j, k) -> (i + dx, j + dy, k + dz) on the cost array c [nz, ny, nx]."""
    if not (_trav(c, i, j, k) and _trav(c, i + dx, j + dy, k + dz)):
        return False
    for sx in ((0, dx) if dx else (0,)):
        for sy in ((0, dy) if dy else (0,)):
            for sz in ((0, dz) if dz else (0,)):
                if not _trav(c, i + sx, j + sy, k + sz):   # (the empty and the full subset are the ends, tested above)
                    return False
    return True


def edges(c, connectivity, planar):
    """{u: [(v, cost)]} over linear indices, u's moves in their lexicographic order."""
    nz, ny, nx = c.shape
    mv = moves(connectivity, planar)
    out = {}
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                if not c[k, j, i]:
                    continue
                lst = []
                for dx, dy, dz, m in mv:
                    if allowed(c, i, j, k, dx, dy, dz):
                        lst.append((((k + dz) * ny + j + dy) * nx + i + dx, WEIGHT[m] * (int(c[k, j, i]) + int(c[k + dz, j + dy, i + dx]))))
                out[(k * ny + j) * nx + i] = lst
    return out


def dijkstra(n_cells, adj, goal_cells):
    """P [n_cells] uint32 by heapq."""
    D = [UNREACHED] * n_cells
    heap = []
    for g in set(goal_cells):
        D[g] = 0
        heap.append((0, g))
    heapq.heapify(heap)
    while heap:
        d, u = heapq.heappop(heap)
        if d > D[u]:
            continue
        for v, w in adj.get(u, ()):
            s = d + w
            if s < UNREACHED and s < D[v]:
                D[v] = s
                heapq.heappush(heap, (s, v))
    return np.array(D, np.uint32)


def relax_fixpoint(n_cells, adj, goal_cells):
    """The same P by relaxing every edge until nothing changes."""
    D = [UNREACHED] * n_cells
    for g in goal_cells:
        D[g] = 0
    changed = True
    while changed:
        changed = False
        for u, lst in adj.items():
            if D[u] == UNREACHED:
                continue
            for v, w in lst:
                s = D[u] + w
                if s < UNREACHED and s < D[v]:
                    D[v] = s
                    changed = True
    return np.array(D, np.uint32)


def cells_of(prm, shape, planar, pts):
    """(ok [n] bool, ijk [n, 3] int64) of world points against a field of shape [nz, ny, nx]."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    qf = ocr.quant_f(pts, prm["origin"], prm["resolution"])
    if planar:
        qf[:, 2] = 0
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < ocr.Q_LIMIT, axis=1)
    v = np.where(ok[:, None], qf, 0).astype(np.int64) >> 8
    ok &= np.all((v >= 0) & (v < np.array(shape[::-1])), axis=1)
    return ok, v


def build(prm, s2, pp, table, goals):
    """(cost uint8, P uint32, stats [4] uint64, adj) of a distance field s2 ([nz, ny, nx], or [ny, nx]: planar); cost and P in the
    shape of s2."""
    s2 = np.asarray(s2)
    planar = s2.ndim == 2
    c = cell_cost(s2, pp["min_clear_s2"], table)
    c3 = c[None] if planar else c
    nz, ny, nx = c3.shape
    ok, v = cells_of(prm, c3.shape, planar, goals)
    used = [(int(k) * ny + int(j)) * nx + int(i) for (i, j, k), o in zip(v, ok) if o and c3[k, j, i]]
    adj = edges(c3, pp["connectivity"], planar)
    P = dijkstra(c3.size, adj, used)
    reached = P != UNREACHED
    stats = np.array([len(used), np.count_nonzero(c3), reached.sum(), P[reached].max() if reached.any() else 0], np.uint64)
    return c, P.reshape(s2.shape), stats, adj


def paths(prm, c, P, adj, starts):
    """(status [n] int32, cost [n] uint32, offsets [n + 1] uint64, cells int32) of start points on a finished plan."""
    planar = c.ndim == 2
    c3 = c[None] if planar else c
    Pf = np.asarray(P).reshape(-1)
    nz, ny, nx = c3.shape
    ok, v = cells_of(prm, c3.shape, planar, starts)
    status, cost, off, cells = [], [], [0], []
    for (i, j, k), o in zip(v, ok):
        if not o or not c3[k, j, i]:
            status.append(2)
            cost.append(UNREACHED)
        elif Pf[(k * ny + j) * nx + i] == UNREACHED:
            status.append(1)
            cost.append(UNREACHED)
        else:
            u = int((k * ny + j) * nx + i)
            status.append(0)
            cost.append(int(Pf[u]))
            cells.append(u)
            while Pf[u] != 0:
                u = next(w for w, e in adj[u] if Pf[w] != UNREACHED and int(Pf[w]) + e == int(Pf[u]))
                cells.append(u)
        off.append(len(cells))
    return np.array(status, np.int32), np.array(cost, np.uint32), np.array(off, np.uint64), np.array(cells, np.int32)


def random_s2(rng, shape, p_obstacle):
    """A distance field for tests through distance_ref: random obstacles of the given density, unsigned and untruncated; with no
    obstacle every value is FAR."""
    import distance_ref as dr

    mask = rng.uniform(size=shape) < p_obstacle
    s2 = dr.field(mask if len(shape) == 3 else mask[None], dr.dparams())
    return s2 if len(shape) == 3 else s2[0]
