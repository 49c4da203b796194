"""The lattice planner's rule (include/limovelo_hip.h "Lattice planner") in numpy and plain Python: what tests/test_lattice_host.py
holds the host build of lv_lattice.hpp to and tests/test_gpu_occ_lattice.py the kernels, state for state.

  states      (i, j, h) over the cost bytes c [ny, nx] of a planar plan (0 = blocked), h in 0..H-1; linear index (h * ny + j) * nx + i.
  table       H * P records (PRIM_DTYPE), record h * P + p primitive p of heading h; length 0: an empty slot.
  move        p from u = (i, j, h) to v = (i + di, j + dj, h_to): allowed iff start, end and every sweep cell (offsets from the start)
              are inside the grid and traversable.  edge = length * (c(u) + c(v)) + penalty.  Directed.
  goals       records (x, y, z, h): the cell quantised as the planner's goals are (z unused); h = -1: every heading of the cell;
              ignored when non-finite, outside, blocked or h outside -1..H-1.
  V           least total edge cost from the state to any goal state, uint32; UNREACHED = 0xFFFFFFFF for blocked cells, for no
              sequence, and for a cost that would reach 0xFFFFFFFF.
  path        status 2: start non-finite, outside, blocked or h out of range; 1: V unreached; 0: the states from the start to a state
              with V = 0, the next being the successor of the first p that is non-empty, allowed and has edge + V(succ) == V(s).
              h = -1: the heading with the least V at the cell, ties to the smaller h.
Everything is integer arithmetic and is compared by equality.  dijkstra runs heapq on the reversed graph; sweep_fixpoint states the
fixpoint V(s) = min_p (edge + V(succ)) heading by heading on whole arrays."""
import heapq

import numpy as np

import plan_ref as pr

F = np.float32
UNREACHED = 0xFFFFFFFF
REACH, MAX_SWEEP, MAX_PENALTY, MAX_H, MAX_P = 8, 10, 1 << 24, 16, 16
PRIM_DTYPE = np.dtype([("di", np.int8), ("dj", np.int8), ("h_to", np.uint8), ("n_sweep", np.uint8), ("length", np.uint16),
                       ("reserved", np.uint16), ("penalty", np.uint32), ("sweep", np.int8, (MAX_SWEEP, 2))])
POSE_DTYPE = np.dtype([("xyz", F, 3), ("h", np.int32)])
assert PRIM_DTYPE.itemsize == 32 and POSE_DTYPE.itemsize == 16


def table(H, P):
    """An empty table [H, P]."""
    return np.zeros((H, P), PRIM_DTYPE)


def prim(di, dj, h_to, length, penalty=0, sweep=()):
    r = np.zeros((), PRIM_DTYPE)
    r["di"], r["dj"], r["h_to"], r["length"], r["penalty"], r["n_sweep"] = di, dj, h_to, length, penalty, len(sweep)
    for s, (a, b) in enumerate(sweep):
        r["sweep"][s] = (a, b)
    return r


def poses(rows):
    """POSE_DTYPE records from rows (x, y, z, h)."""
    a = np.asarray(rows, np.float64).reshape(-1, 4)
    out = np.zeros(len(a), POSE_DTYPE)
    out["xyz"] = a[:, :3].astype(F)
    out["h"] = a[:, 3].astype(np.int32)
    return out


def neighbour_table():
    """H = 1, the planner's 8 moves in its order: length 10 / 14, a diagonal sweeping its two corner cells."""
    t = table(1, 8)
    moves = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
    for p, (dx, dy) in enumerate(moves):
        t[0, p] = prim(dx, dy, 0, 14 if dx and dy else 10, 0, [(dx, 0), (0, dy)] if dx and dy else [])
    return t


def check_table(H, P, prims):
    """None when the table holds, otherwise (record or None, why)."""
    if not 1 <= H <= MAX_H:
        return None, "H"
    if not 1 <= P <= MAX_P:
        return None, "P"
    t = np.asarray(prims).reshape(-1)
    if t.size != H * P:
        return None, "n_prims"
    for n, r in enumerate(t):
        h = n // P
        if r["reserved"] != 0:
            return n, "reserved"
        if abs(int(r["di"])) > REACH or abs(int(r["dj"])) > REACH:
            return n, "di, dj"
        if r["h_to"] >= H:
            return n, "h_to"
        if r["n_sweep"] > MAX_SWEEP:
            return n, "n_sweep"
        if r["penalty"] > MAX_PENALTY:
            return n, "penalty"
        for s in range(MAX_SWEEP):
            a, b = int(r["sweep"][s][0]), int(r["sweep"][s][1])
            if abs(a) > REACH or abs(b) > REACH:
                return n, "sweep"
            if s >= r["n_sweep"] and (a or b):
                return n, "sweep unused"
        if r["length"] and r["di"] == 0 and r["dj"] == 0 and r["h_to"] == h:
            return n, "self loop"
    if not np.any(t["length"] != 0):
        return None, "empty"
    return None


def reach_of(prims):
    t = np.asarray(prims).reshape(-1)
    out = 0
    for r in t[t["length"] != 0]:
        out = max(out, abs(int(r["di"])), abs(int(r["dj"])), *(abs(int(v)) for v in r["sweep"][:r["n_sweep"]].reshape(-1)), 0)
    return out


def _shift(a, di, dj, fill):
    """b[j, i] = a[j + dj, i + di], `fill` where that is outside."""
    ny, nx = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dj, ny), slice(0, ny - dj)) if dj >= 0 else (slice(0, ny + dj), slice(-dj, ny))
    xs, xd = (slice(di, nx), slice(0, nx - di)) if di >= 0 else (slice(0, nx + di), slice(-di, nx))
    if abs(di) < nx and abs(dj) < ny:
        b[yd, xd] = a[ys, xs]
    return b


def _moves(c, prims):
    """Per non-empty record (h, p, r, allowed [ny, nx] bool, edge [ny, nx] int64)."""
    c64 = np.asarray(c, np.int64)
    H, P = prims.shape
    out = []
    for h in range(H):
        for p in range(P):
            r = prims[h, p]
            if not r["length"]:
                continue
            cv = _shift(c64, int(r["di"]), int(r["dj"]), 0)
            ok = (c64 != 0) & (cv != 0)
            for s in range(int(r["n_sweep"])):
                ok &= _shift(c64, int(r["sweep"][s][0]), int(r["sweep"][s][1]), 0) != 0
            out.append((h, p, r, ok, int(r["length"]) * (c64 + cv) + int(r["penalty"])))
    return out


def sweep_fixpoint(c, prims, goal_states):
    """V [H, ny, nx] uint32: every state lowered from its successors, whole arrays at a time, until nothing changes."""
    H, _ = prims.shape
    ny, nx = c.shape
    V = np.full((H, ny, nx), UNREACHED, np.int64)
    V.reshape(-1)[list(goal_states)] = 0
    mv = _moves(c, prims)
    changed = True
    while changed:
        changed = False
        for h, p, r, ok, edge in mv:
            succ = _shift(V[int(r["h_to"])], int(r["di"]), int(r["dj"]), UNREACHED)
            cand = np.where(ok & (succ != UNREACHED), succ + edge, UNREACHED)
            cand[cand >= UNREACHED] = UNREACHED
            if np.any(cand < V[h]):
                V[h] = np.minimum(V[h], cand)
                changed = True
    return V.astype(np.uint32)


def dijkstra(c, prims, goal_states):
    """V [H, ny, nx] uint32 by heapq over the reversed graph (as plan_ref.dijkstra does it)."""
    H, _ = prims.shape
    ny, nx = c.shape
    n = H * ny * nx
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    us, vs, ws = [], [], []
    for h, p, r, ok, edge in _moves(c, prims):
        us.append(((h * ny + jj[ok]) * nx + ii[ok]))
        vs.append(((int(r["h_to"]) * ny + jj[ok] + int(r["dj"])) * nx + ii[ok] + int(r["di"])))
        ws.append(edge[ok])
    us, vs, ws = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (us, vs, ws))
    order = np.argsort(vs, kind="stable")
    us, vs, ws = us[order].tolist(), vs[order], ws[order].tolist()
    first = np.searchsorted(vs, np.arange(n + 1)).tolist()   # the edges INTO state v: first[v] .. first[v + 1]
    D = [UNREACHED] * n
    heap = []
    for g in set(goal_states):
        D[g] = 0
        heap.append((0, g))
    heapq.heapify(heap)
    while heap:
        d, v = heapq.heappop(heap)
        if d > D[v]:
            continue
        for e in range(first[v], first[v + 1]):
            s = d + ws[e]
            u = us[e]
            if s < UNREACHED and s < D[u]:
                D[u] = s
                heapq.heappush(heap, (s, u))
    return np.array(D, np.uint32).reshape(H, ny, nx)


def cells_of(prm, shape, recs):
    """(ok [n] bool, ij [n, 2]) of pose records against cost bytes of shape [ny, nx]."""
    ok, v = pr.cells_of(prm, (1,) + tuple(shape), True, recs["xyz"])
    return ok, v[:, :2]


def goal_states(prm, c, H, goals):
    """The goal states, and the number of goal records used."""
    ny, nx = c.shape
    ok, ij = cells_of(prm, c.shape, goals)
    states, used = [], 0
    for (i, j), o, h in zip(ij, ok, goals["h"]):
        if not o or not c[j, i] or not -1 <= h < H:
            continue
        used += 1
        states += [(t * ny + int(j)) * nx + int(i) for t in (range(H) if h < 0 else (int(h),))]
    return states, used


def build(prm, c, prims, goals, solver=dijkstra):
    """(V [H, ny, nx] uint32, stats [4] uint64) over the cost bytes c [ny, nx] of a planar plan."""
    prims = np.asarray(prims)
    H = prims.shape[0]
    gs, used = goal_states(prm, c, H, goals)
    V = solver(c, prims, gs)
    reached = V != UNREACHED
    return V, np.array([used, H * np.count_nonzero(c), reached.sum(), V[reached].max() if reached.any() else 0], np.uint64)


def allowed(c, r, i, j):
    ny, nx = c.shape
    trav = lambda a, b: 0 <= a < nx and 0 <= b < ny and c[b, a] != 0
    return bool(r["length"]) and trav(i, j) and trav(i + int(r["di"]), j + int(r["dj"])) and all(
        trav(i + int(r["sweep"][s][0]), j + int(r["sweep"][s][1])) for s in range(int(r["n_sweep"])))


def paths(prm, c, V, prims, starts):
    """(status [n] int32, cost [n] uint32, offsets [n + 1] uint64, states int32, prims uint8) of start records on a finished V."""
    prims = np.asarray(prims)
    H, P = prims.shape
    ny, nx = c.shape
    ok, ij = cells_of(prm, c.shape, starts)
    status, cost, off, states, taken = [], [], [0], [], []
    for (i, j), o, h in zip(ij, ok, starts["h"]):
        i, j, h = int(i), int(j), int(h)
        if not o or not c[j, i] or not -1 <= h < H:
            status.append(2)
            cost.append(UNREACHED)
        else:
            if h < 0:
                h = int(np.argmin(V[:, j, i]))   # (the first of the least)
            if V[h, j, i] == UNREACHED:
                status.append(1)
                cost.append(UNREACHED)
            else:
                status.append(0)
                cost.append(int(V[h, j, i]))
                while True:
                    states.append((h * ny + j) * nx + i)
                    if V[h, j, i] == 0:
                        taken.append(255)
                        break
                    for p in range(P):
                        r = prims[h, p]
                        if not allowed(c, r, i, j):
                            continue
                        vi, vj, vh = i + int(r["di"]), j + int(r["dj"]), int(r["h_to"])
                        if V[vh, vj, vi] != UNREACHED and int(V[vh, vj, vi]) + int(r["length"]) * (int(c[j, i]) + int(c[vj, vi])) + int(r["penalty"]) == int(V[h, j, i]):
                            break
                    else:
                        raise AssertionError("no successor explains V: not a fixpoint")
                    taken.append(p)
                    i, j, h = vi, vj, vh
        off.append(len(states))
    return np.array(status, np.int32), np.array(cost, np.uint32), np.array(off, np.uint64), np.array(states, np.int32), np.array(taken, np.uint8)


def random_table(rng, H, P, reach, p_empty=0.15, max_penalty=40, sweeps=True):
    """A legal random table: offsets within `reach`, some empty slots, some turns on the spot, sweep cells between the ends."""
    t = table(H, P)
    for h in range(H):
        for p in range(P):
            if rng.uniform() < p_empty:
                continue
            di, dj = (int(v) for v in rng.integers(-reach, reach + 1, 2))
            h_to = int(rng.integers(0, H))
            if di == 0 and dj == 0 and h_to == h:
                if H == 1:
                    di = 1 if reach else 0
                    if not reach:
                        continue
                else:
                    h_to = (h + 1) % H
            n = int(rng.integers(0, 4)) if sweeps and reach else 0
            sw = [(int(rng.integers(min(0, di), max(0, di) + 1)), int(rng.integers(min(0, dj), max(0, dj) + 1))) for _ in range(n)]
            t[h, p] = prim(di, dj, h_to, int(rng.integers(1, 30)), int(rng.integers(0, max_penalty + 1)), sw)
    if not np.any(t["length"]):
        t[0, 0] = prim(1 if reach else 0, 0, 0 if reach else (1 % H), 10)
    return t
