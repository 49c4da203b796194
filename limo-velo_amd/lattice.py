"""The state-lattice planner for car-like robots from Python (include/limovelo_hip.h "Lattice planner"): the lattice's headings,
a generator of motion primitives (the usual SBPL / nav2 construction, on the host in f64), the table check restated, and
plan / routes / polyline over a capi.Context.

The generator's floats are inputs, like the planner's cost table: nothing in the device rule depends on them.  A table from
anywhere else that passes check_primitives serves as well."""
from __future__ import annotations

import math

import numpy as np

from . import capi

REACH, MAX_SWEEP = capi.LV_LATTICE_REACH, capi.LV_LATTICE_MAX_SWEEP
MAX_PENALTY = 1 << 24


def directions(H: int) -> np.ndarray:
    """[H, 2] int: the lattice vectors of the headings, counter-clockwise from +x.  H = 4: the axes; 8: axes and diagonals;
    16: those and the (2, 1) family."""
    if H == 4:
        first = [(1, 0)]
    elif H == 8:
        first = [(1, 0), (1, 1)]
    elif H == 16:
        first = [(1, 0), (2, 1), (1, 1), (1, 2)]
    else:
        raise ValueError(f"H = {H}: the lattice directions are defined for 4, 8 and 16 headings")
    out = []
    for q in range(4):   # quarter turns: (x, y) -> (-y, x)
        for x, y in first:
            for _ in range(q):
                x, y = -y, x
            out.append((x, y))
    return np.array(out, np.int64)


def headings(H: int) -> np.ndarray:
    """[H] f64: the angles of the lattice directions in [0, 2 pi): for 16, those of (1, 0), (2, 1), (1, 1), (1, 2), (0, 1), ..."""
    d = directions(H)
    return np.mod(np.arctan2(d[:, 1], d[:, 0]), 2.0 * math.pi)


def heading_index(th: float, H: int) -> int:
    """The heading bin nearest to angle th (radians); ties to the smaller index."""
    diff = np.abs(np.mod(headings(H) - float(th) + math.pi, 2.0 * math.pi) - math.pi)
    return int(np.argmin(diff))


def _cells_along(points, end) -> list:
    """The cells a densely sampled path passes between its two ends, in order, each once.  Cell centres lie on the integers."""
    seen, out = {(0, 0), tuple(end)}, []
    for x, y in points:
        c = (int(math.floor(x + 0.5)), int(math.floor(y + 0.5)))
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def _sample(th0, th1, a, R, b, step=0.02):
    """Points of straight a, arc of radius R from heading th0 to th1 (the short way), straight b; lengths in cells."""
    pts = []
    x = y = 0.0
    for s in np.arange(0.0, a, step):
        pts.append((x + s * math.cos(th0), y + s * math.sin(th0)))
    x, y = a * math.cos(th0), a * math.sin(th0)
    d = math.remainder(th1 - th0, 2.0 * math.pi)
    sg = 1.0 if d >= 0 else -1.0
    n = max(2, int(abs(d) * R / step) + 1)
    for t in np.linspace(0.0, d, n):
        pts.append((x + sg * R * (math.sin(th0 + t) - math.sin(th0)), y - sg * R * (math.cos(th0 + t) - math.cos(th0))))
    x, y = pts[-1]
    for s in np.arange(0.0, b, step):
        pts.append((x + s * math.cos(th1), y + s * math.sin(th1)))
    return pts


def _arc(th0, th1, R):
    """The nearest lattice cell that a straight - arc (radius R cells) - straight from heading th0 to th1 ends in exactly:
    (di, dj, a, b, length in cells), or None within the reach."""
    d = math.remainder(th1 - th0, 2.0 * math.pi)
    sg = 1.0 if d >= 0 else -1.0
    ax, ay = sg * R * (math.sin(th1) - math.sin(th0)), -sg * R * (math.cos(th1) - math.cos(th0))   # the arc's displacement
    u0, u1 = (math.cos(th0), math.sin(th0)), (math.cos(th1), math.sin(th1))
    det = u0[0] * u1[1] - u0[1] * u1[0]
    best = None
    for dj in range(-REACH, REACH + 1):
        for di in range(-REACH, REACH + 1):
            rx, ry = di - ax, dj - ay
            a = (rx * u1[1] - ry * u1[0]) / det
            b = (u0[0] * ry - u0[1] * rx) / det
            if a < -1e-9 or b < -1e-9:
                continue
            a, b = max(a, 0.0), max(b, 0.0)
            key = (round(a + b + R * abs(d), 9), abs(di) + abs(dj), dj, di)
            if best is None or key < best[0]:
                best = (key, di, dj, a, b)
    if best is None:
        return None
    _, di, dj, a, b = best
    return di, dj, a, b, a + b + R * abs(d)


def _too_far(what):
    return ValueError(f"{what}: a primitive would exceed LV_LATTICE_REACH = {REACH} cells or LV_LATTICE_MAX_SWEEP = {MAX_SWEEP} sweep cells: "
                      "plan on a coarser grid (a larger resolution) or with a smaller min_radius")


def primitives(H: int, min_radius: float, resolution: float, reverse: bool = False, reverse_penalty: int = 200, turn_penalty: int = 0,
               in_place: bool = False) -> np.ndarray:
    """The table [H, P] (capi.LATTICE_PRIM_DTYPE) of a car with turning radius min_radius (metres) on a grid of `resolution`
    metres.  Per heading: a straight step along the heading's lattice vector, then an arc to the heading on the left and one to
    the heading on the right, each straight - arc - straight at min_radius to the nearest lattice cell that admits it (P = 3).
    reverse: the same three driven backwards, each at reverse_penalty more (P = 6).  in_place: two turns on the spot to the
    adjacent headings (2 more).  turn_penalty is added to every primitive that changes heading.  length = round(10 * the path's
    length in cells), at least 1; the sweep cells come from dense sampling of the path."""
    R = float(min_radius) / float(resolution)
    if not (R >= 0.0 and math.isfinite(R)):
        raise ValueError("min_radius / resolution: finite and not negative")
    ang, dirs = headings(H), directions(H)
    P = 3 * (2 if reverse else 1) + (2 if in_place else 0)
    t = np.zeros((H, P), capi.LATTICE_PRIM_DTYPE)

    def fill(h, p, di, dj, h_to, cells_len, penalty, sweep):
        if max(abs(di), abs(dj)) > REACH or len(sweep) > MAX_SWEEP or any(max(abs(a), abs(b)) > REACH for a, b in sweep):
            raise _too_far(f"heading {h}, primitive {p}")
        r = t[h, p]
        r["di"], r["dj"], r["h_to"], r["n_sweep"] = di, dj, h_to, len(sweep)
        r["length"] = max(1, min(65535, int(round(10.0 * cells_len))))
        r["penalty"] = min(int(penalty), MAX_PENALTY)
        for s, (a, b) in enumerate(sweep):
            r["sweep"][s] = (a, b)

    for h in range(H):
        moves = []   # (di, dj, h_to, length in cells, turns, sweep)
        dx, dy = (int(v) for v in dirs[h])
        n = math.hypot(dx, dy)
        moves.append((dx, dy, h, n, False, _cells_along(_sample(ang[h], ang[h], n, 0.0, 0.0), (dx, dy))))
        for h_to in ((h + 1) % H, (h - 1) % H):
            found = _arc(ang[h], ang[h_to], R)
            if found is None:
                raise _too_far(f"heading {h} to heading {h_to}")
            di, dj, a, b, ln = found
            moves.append((di, dj, h_to, ln, True, _cells_along(_sample(ang[h], ang[h_to], a, R, b), (di, dj))))
        p = 0
        for di, dj, h_to, ln, turns, sweep in moves:
            fill(h, p, di, dj, h_to, ln, turn_penalty if turns else 0, sweep)
            p += 1
        if reverse:   # the same paths mirrored in the start point and driven backwards: the heading runs through the same angles
            for di, dj, h_to, ln, turns, sweep in moves:
                fill(h, p, -di, -dj, h_to, ln, reverse_penalty + (turn_penalty if turns else 0), [(-a, -b) for a, b in sweep])
                p += 1
        if in_place:
            for h_to in ((h + 1) % H, (h - 1) % H):
                fill(h, p, 0, 0, h_to, abs(math.remainder(ang[h_to] - ang[h], 2.0 * math.pi)), turn_penalty, [])
                p += 1
    check_primitives(t)
    return t


def check_primitives(prims) -> None:
    """The C check of the table restated: raises ValueError naming the record (h * P + p) that lv_occ_lattice_build would refuse."""
    t = np.asarray(prims)
    if t.dtype != capi.LATTICE_PRIM_DTYPE or t.ndim != 2:
        raise ValueError("a table is an array [H, P] of capi.LATTICE_PRIM_DTYPE records")
    H, P = t.shape
    if not (1 <= H <= 16 and 1 <= P <= 16):
        raise ValueError(f"H = {H}, P = {P}: each 1..16")
    for n, r in enumerate(t.reshape(-1)):
        h = n // P
        sw = r["sweep"].astype(np.int64)
        why = None
        if r["reserved"] != 0:
            why = "reserved must be 0"
        elif max(abs(int(r["di"])), abs(int(r["dj"]))) > REACH:
            why = "di, dj: each within +-LV_LATTICE_REACH"
        elif r["h_to"] >= H:
            why = "h_to: 0..H-1"
        elif r["n_sweep"] > MAX_SWEEP:
            why = "n_sweep: 0..LV_LATTICE_MAX_SWEEP"
        elif r["penalty"] > MAX_PENALTY:
            why = "penalty: at most 2^24"
        elif np.any(np.abs(sw) > REACH):
            why = "sweep: each offset within +-LV_LATTICE_REACH"
        elif np.any(sw[int(r["n_sweep"]):] != 0):
            why = "sweep: unused entries must be 0"
        elif r["length"] and r["di"] == 0 and r["dj"] == 0 and r["h_to"] == h:
            why = "a self loop (di == dj == 0 and h_to == h)"
        if why:
            raise ValueError(f"record {n} (heading {h}, primitive {n % P}): {why}")
    if not np.any(t["length"] != 0):
        raise ValueError("the table has no non-empty record (every length is 0)")


def _records(poses_xyth, H):
    a = np.asarray(poses_xyth, np.float64).reshape(-1, 3)
    rec = np.zeros(len(a), capi.LATTICE_POSE_DTYPE)
    rec["xyz"][:, :2] = a[:, :2].astype(np.float32)
    rec["h"] = [-1 if not math.isfinite(th) else heading_index(th, H) for th in a[:, 2]]
    return rec


def plan(ctx, goals_xyth, prims):
    """Builds the lattice over the planar plan last built (occupancy.plan): goals_xyth [n, 3] rows (x, y, theta in radians; a
    NaN theta: any heading).  Returns (info, stats): lv_lattice_info, and goals used, traversable states, reached states, the
    largest finite V."""
    t = np.asarray(prims)
    check_primitives(t)
    stats = ctx.occ_lattice_build(_records(goals_xyth, t.shape[0]), t)
    return ctx.occ_lattice_info(), stats


def routes(ctx, starts_xyth):
    """Per start (x, y, theta; a NaN theta: the best heading there) a tuple (poses, prims, status, cost): the poses (x, y, theta)
    at the centres of the route's cells, [n, 3] f64 (empty unless status is 0), the primitive taken out of each pose (255 at the
    last), the status (0 a route, 1 no route from there, 2 the start is blocked, outside or its heading out of range) and the
    route's cost (V of the start state)."""
    i = ctx.occ_lattice_info()
    status, cost, off, states, taken = ctx.occ_lattice_paths(_records(starts_xyth, max(i.H, 1)))
    p = ctx.occ_params()
    res = np.float64(p.resolution)
    s = states.astype(np.int64)
    ang = headings(i.H) if i.H in (4, 8, 16) else 2.0 * math.pi * np.arange(max(i.H, 1)) / max(i.H, 1)
    plane = max(i.nx * i.ny, 1)
    poses = np.stack([np.float64(p.origin[0]) + (s % max(i.nx, 1) + 0.5) * res, np.float64(p.origin[1]) + ((s % plane) // max(i.nx, 1) + 0.5) * res,
                      ang[s // plane] if len(s) else np.zeros(0)], axis=1)
    return [(poses[int(off[k]):int(off[k + 1])], taken[int(off[k]):int(off[k + 1])], int(status[k]), int(cost[k])) for k in range(len(status))]


def polyline(route, prims) -> np.ndarray:
    """[m, 2] f64 for display: the route's cell centres with the sweep cells of each primitive taken between them (the cell size
    is read off the route's own steps)."""
    poses, taken = route[0], route[1]
    t = np.asarray(prims)
    H = t.shape[0]
    ang = headings(H) if H in (4, 8, 16) else 2.0 * math.pi * np.arange(H) / H
    recs = [t[int(np.argmin(np.abs(ang - pose[2]))), int(p)] if p != 255 else None for pose, p in zip(poses, taken)]
    res = 0.0
    for k, r in enumerate(recs[:-1]):
        for a, name in ((0, "di"), (1, "dj")):
            if r is not None and r[name] != 0:
                res = (poses[k + 1][a] - poses[k][a]) / float(r[name])
    out = []
    for pose, r in zip(poses, recs):
        out.append((pose[0], pose[1]))
        if r is not None:
            out += [(pose[0] + float(a) * res, pose[1] + float(b) * res) for a, b in r["sweep"][:int(r["n_sweep"])]]
    return np.array(out, np.float64).reshape(-1, 2)
