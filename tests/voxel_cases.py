"""The shared cases of the scan voxel grid (limo-velo_amd/csrc/lv_scan.hip): inputs whose leaves hold MANY points, for each of
the three routes that must produce the same bits (small: window_small_kernel; large: deskew_keys_kernel + window_tail_kernel;
general: vg_* kernels + the library sorts).  tests/test_voxel_cases_ref.py holds the cases to what they claim on the CPU,
tests/test_gpu_voxel_grid.py runs them on the device.

A case is (name, xyz f32 [n,3], leaf, expected route, drop mask or None) plus the entry point it goes through and the
options it runs with.  Inputs are built leaf by leaf:
* populations from POPULATIONS (both sides of the 8-member read-ahead of the centroid loops, of 16, of a wavefront);
* leaves at least 30 m from the origin, on both sides of it (negative coordinates);
* members uniform inside their leaf (f64 uniform -> f32: full mantissas);
* input order: no two members of a leaf are adjacent (the stable sort has to bring them together), except where one leaf
  holds every point.
The de-skew of the deskew / window entries is the identity (states at rest, identity poses): what reaches the voxel grid is
the input, so the populations hold on the device as built.  Dropped points: non-finite coordinates for scan_downsample;
stamps outside the states for the de-skew entries (in a window the buffer is time-ordered, so a dropped point in the MIDDLE
of a window carries an infinite coordinate instead: its de-skewed image is not finite)."""
import functools
import heapq
from typing import NamedTuple, Optional

import numpy as np

import cloud_messages as cm

POPULATIONS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200)
NONE, SMALL, LARGE, GENERAL = 0, 1, 2, 3          # capi.SCAN_ROUTE_*
SMALL_WINDOW, WT_IN, WT_OUT, WT_STAGE = 2048, 16384, 4096, 6144   # the limits of lv_scan.hip
T0, DT = 100.0, 1e-5                              # stamp of input index i: T0 + i * DT


class Case(NamedTuple):
    name: str
    xyz: np.ndarray                 # [n,3] f32, as handed to the entry point (dropped points of scan_downsample: non-finite)
    leaf: float
    route: int                      # the route lv_scan_route must report
    drop: Optional[np.ndarray]      # bool [n]: points that must not reach the voxel grid
    entry: str = "downsample"       # "downsample" | "deskew" | "window"
    options: tuple = ()             # (("small_window", 0), ...) set before the call
    one_leaf: bool = False
    big: int = 0                    # population of the one leaf beyond POPULATIONS (0: none)


# ---- the rule, in numpy ------------------------------------------------------------------------------------------------------
def leaf_order(xyz, leaf):
    """pcl::VoxelGrid's leaf of every point (floor by x * (1/leaf) in f32), the stable order by the mixed-radix leaf index,
    and the leaves' (first sorted position, population)."""
    p = np.ascontiguousarray(xyz, np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(p * inv).astype(np.int64)
    if len(p) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    mn = np.floor(p.min(axis=0) * inv).astype(np.int64)
    mx = np.floor(p.max(axis=0) * inv).astype(np.int64)
    div = mx - mn + 1
    ijk -= mn
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    heads = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    counts = np.diff(np.r_[heads, len(s)])
    return order, heads, counts


def reference(xyz, leaf, how="sequential"):
    """Centroid of every leaf, [leaves,3] f32: the f32 sum of its members in input order, divided by the count.
    how = "sequential" (the contract: one add after the other, never np.sum); "reverse", "pairwise" or "chunks8" (each whole
    chunk of eight members backwards: a slip in a read-ahead loop) — the alternatives a wrong kernel would compute."""
    p = np.ascontiguousarray(xyz, np.float32)
    order, heads, counts = leaf_order(p, leaf)
    s = p[order]
    acc = np.zeros((len(heads), 3), np.float32)
    if how in ("sequential", "reverse", "chunks8"):
        for k in range(int(counts.max()) if len(counts) else 0):     # the k-th add of every leaf that has one
            live = np.flatnonzero(counts > k)
            if how == "sequential":
                at = heads[live] + k
            elif how == "reverse":
                at = heads[live] + counts[live] - 1 - k
            else:                                                      # every whole chunk of eight members backwards
                at = heads[live] + np.where(k < (counts[live] & ~7), (k & ~7) + 7 - (k & 7), k)
            acc[live] = acc[live] + s[at]                              # one f32 add per axis
    elif how == "pairwise":
        for l, (h, c) in enumerate(zip(heads, counts)):
            v = s[h:h + c].copy()
            while len(v) > 1:
                tail = v[len(v) & ~1:]
                v = np.concatenate([v[0:len(v) & ~1:2] + v[1::2], tail])
            acc[l] = np.float32(0.0) + v[0]
    else:
        raise ValueError(how)
    return acc / counts.astype(np.float32)[:, None]


# ---- building blocks ----------------------------------------------------------------------------------------------------------
def _cells(rng, k, leaf):
    """k distinct leaf cells, >= 30 m from the origin along x on either side of it, in voxel-grid order (z, then y, then x)."""
    lo = int(np.ceil(30.0 / leaf)) + 1
    flat = rng.choice(2 * 64 * 80 * 24, size=k, replace=False)
    xs, r = flat % 128, flat // 128
    ys, zs = r % 80 - 40, r // 80 - 12
    cx = np.where(xs < 64, lo + xs, -(lo + xs - 64) - 1)
    c = np.stack([cx, ys, zs], axis=1).astype(np.int64)
    return c[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))]


def _members(rng, cell, leaf, m):
    p = ((cell[None, :] + rng.uniform(0.03, 0.97, (m, 3))) * leaf).astype(np.float32)
    assert np.array_equal(np.floor(p * (np.float32(1.0) / np.float32(leaf))).astype(np.int64), np.broadcast_to(cell, (m, 3)))
    return p


def _interleave(rng, pops):
    """An input order of sum(pops) points, as (leaf, member) per input position, in which no two neighbours share a leaf:
    always the leaf with the most members left that is not the previous one (ties at random)."""
    heap = [(-m, float(rng.random()), l) for l, m in enumerate(pops)]
    heapq.heapify(heap)
    out, prev, taken = [], -1, [0] * len(pops)
    while heap:
        a = heapq.heappop(heap)
        if a[2] == prev:
            if not heap:
                raise ValueError("one leaf holds more than half of the points")
            b = heapq.heappop(heap)
            heapq.heappush(heap, a)
            a = b
        l = a[2]
        out.append((l, taken[l]))
        taken[l] += 1
        prev = l
        if a[0] + 1 < 0:
            heapq.heappush(heap, (a[0] + 1, float(rng.random()), l))
    return out


def build(seed, pops, leaf, extra=None):
    """xyz [n,3] f32 whose leaves, in voxel-grid order, hold pops[0], pops[1], ... members; extra: points appended to the
    input (each alone in a far leaf that sorts behind every other)."""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, len(pops), leaf)
    mem = [_members(rng, cells[l], leaf, m) for l, m in enumerate(pops)]
    if len(pops) == 1:
        xyz = mem[0]
    else:
        xyz = np.stack([mem[l][k] for l, k in _interleave(rng, pops)])
    if extra is not None:
        xyz = np.concatenate([xyz, np.asarray(extra, np.float32).reshape(-1, 3)])
    return np.ascontiguousarray(xyz, np.float32)


def pops_for_total(n, cycle=POPULATIONS):
    """Populations from `cycle`, in turn, that add up to exactly n."""
    out, left, k = [], n, 0
    while left > 0:
        m = cycle[k % len(cycle)]
        if m > left:
            m = max(q for q in POPULATIONS if q <= left)
        out.append(m)
        left -= m
        k += 1
    return out


def order_sensitive(xyz, leaf):
    """Per leaf with >= 8 members: does the reverse / the pairwise / the chunks-of-eight-backwards sum change a bit of its
    centroid?  -> (bool[], bool[], bool[])"""
    _, _, counts = leaf_order(xyz, leaf)
    seq = reference(xyz, leaf).view(np.uint32)
    big = counts >= 8
    return tuple((reference(xyz, leaf, how).view(np.uint32) != seq).any(axis=1)[big] for how in ("reverse", "pairwise", "chunks8"))


def _one_leaf(seed, n, leaf):
    """One leaf holding all n points; the seed is the first from `seed` on at which every alternative summation order changes
    a bit of the centroid (n >= 8: with fewer members the orders may agree, and nothing is claimed)."""
    while True:
        xyz = build(seed, [n], leaf)
        if n < 8 or all(a.all() for a in order_sensitive(xyz, leaf)):
            return xyz
        seed += 1000


SMALL_MIX = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 200, 200, 65, 64, 63, 17, 16, 15, 9, 8, 7, 2, 1,
             200, 200, 200, 200, 65, 17, 16, 15, 1]          # 2048 points; leaves straddle 127|128 and 1023|1024
SHORT_MIX = [9, 1, 64, 2, 17, 8, 200, 7, 65, 16, 63, 15]     # 467 points, heads on even and odd positions
_OFF = (("small_window", 0), ("large_window", 0))


def _with_drops(xyz, where, entry, fill=None):
    """Insert dropped points at the input positions `where` (positions in the RESULT); returns (xyz, drop mask)."""
    n = len(xyz) + len(where)
    drop = np.zeros(n, bool)
    drop[list(where)] = True
    out = np.empty((n, 3), np.float32)
    out[~drop] = xyz
    out[drop] = xyz[0]                      # an ordinary point: the de-skew entries drop it by its stamp
    if entry == "downsample":
        bad = np.float32([np.nan, np.inf, -np.inf])
        for j, i in enumerate(np.flatnonzero(drop)):
            out[i, j % 3] = bad[j % 3]
    elif entry == "window":                 # the middle of a time-ordered window: only the coordinates can drop a point
        kept = np.flatnonzero(~drop)
        for i in np.flatnonzero(drop):
            if kept[0] < i < kept[-1]:
                out[i, 0] = np.inf
    return out, drop


@functools.lru_cache(maxsize=None)
def cases():
    cs = []

    def add(name, xyz, leaf, route, drop=None, entry="downsample", options=(), twin=True, **kw):
        cs.append(Case(name, xyz, leaf, route, drop, entry, tuple(options), **kw))
        if twin and route == SMALL:         # the same input on the general route
            cs.append(Case(name + "/general", xyz, leaf, GENERAL, drop, entry, _OFF, **kw))
            if entry == "window":           # ... and, small_window off, on the large route (it has no lower limit of its own)
                cs.append(Case(name + "/large", xyz, leaf, LARGE, drop, entry, _OFF[:1], **kw))

    # ---- small route (and, as "/general" twins, the same inputs on the general route)
    add("small-mix-2048", build(11, SMALL_MIX, 0.5), 0.5, SMALL, entry="deskew")
    add("small-mix-2048-window", build(12, SMALL_MIX, 0.5), 0.5, SMALL, entry="window")
    add("small-short-mix-leaf0.2", build(13, SHORT_MIX, 0.2), 0.2, SMALL, entry="downsample")
    for n in (1, 2, 7, 8, 9, 64, 65, 2047, 2048):
        add(f"small-one-leaf-{n}", _one_leaf(100 + n, n, 0.5), 0.5, SMALL, entry="deskew" if n in (9, 65, 2047) else "downsample",
            one_leaf=True)
    for m in (7, 8, 9, 16, 17):             # the last leaf's run ends exactly at n
        add(f"small-last-run-{m}", build(200 + m, [2, 15, 1, 8, m], 0.5), 0.5, SMALL, entry="downsample")
    for leaf in (0.5, 0.2):
        add(f"small-faces-leaf{leaf}", faces(leaf), leaf, SMALL, entry="downsample")
    for entry in ("downsample", "deskew", "window"):
        base = build(300, SHORT_MIX, 0.5)
        n = len(base) + 4
        xyz, drop = _with_drops(base, (0, n // 2, n - 2, n - 1), entry)
        add(f"small-dropped-{entry}", xyz, 0.5, SMALL, drop, entry=entry)
        xyz = build(301, [7, 2, 9], 0.5)
        drop = np.ones(len(xyz), bool)
        if entry == "downsample":
            xyz = np.full_like(xyz, np.nan)
        add(f"small-all-dropped-{entry}", xyz, 0.5, SMALL, drop, entry=entry)
    # the leaf grid of the small kernel's packed key overflows: 2e5 cells along every axis, 8e15 in all -> general
    add("small-declines-8e15-cells", build(310, SHORT_MIX, 0.5, extra=[[1e5, 1e5, 1e5]]), 0.5, GENERAL, entry="deskew")

    # ---- large route (always from the LiDAR buffer)
    def large(name, xyz, route=LARGE, drop=None, **kw):
        cs.append(Case(name, xyz, 0.5, route, drop, "window", (), **kw))

    large("large-one-leaf-7000", _one_leaf(400, 7000, 0.5), one_leaf=True)
    p = [200] * 30 + [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 17, 200, 9, 200, 65]      # the 64 lies on 6139..6202
    large("large-leaf-straddles-6144", build(401, p, 0.5))
    p = [200] * 29 + [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 6400, 17, 200, 9, 65, 200, 8]  # the 6400 lies on 6067..12466
    large("large-leaf-spans-a-stage", build(402, p, 0.5), big=6400)
    light = (1, 2, 7, 2, 1, 8, 2, 1)
    large("large-1024-out", build(403, [POPULATIONS[k % 8] for k in range(1024)], 0.5))
    large("large-1025-out", build(404, [POPULATIONS[k % 8] for k in range(1025)], 0.5))
    large("large-4096-out", build(405, [light[k % 8] for k in range(WT_OUT)], 0.5))
    large("large-4097-out-declines", build(406, [light[k % 8] for k in range(WT_OUT + 1)], 0.5), route=GENERAL)
    large("large-16384-in", build(407, pops_for_total(WT_IN), 0.5))
    large("general-16385-in", build(408, pops_for_total(WT_IN + 1), 0.5), route=GENERAL)
    base = build(409, pops_for_total(3000), 0.5)
    n = len(base) + 43
    xyz, drop = _with_drops(base, (0, n // 2) + tuple(range(n - 41, n)), "window")
    large("large-dropped-behind-the-last-leaf", xyz, drop=drop)
    xyz = build(410, pops_for_total(2500), 0.5)
    large("large-all-dropped", xyz, drop=np.ones(len(xyz), bool))
    # a coordinate beyond the 21-bit fields of the large route's sort key: 1.2e6 leaves of 0.5 m -> general
    large("large-declines-6e5-m", build(411, pops_for_total(2600), 0.5, extra=[[6e5, 31.3, 1.2]]), route=GENERAL)

    # ---- general route on its own sizes
    add("general-one-leaf-3000", _one_leaf(500, 3000, 0.5), 0.5, GENERAL, entry="deskew", one_leaf=True)
    add("general-16400-downsample", build(501, pops_for_total(16400), 0.5), 0.5, GENERAL, entry="downsample")
    base = build(502, pops_for_total(2500), 0.5)
    n = len(base) + 3
    xyz, drop = _with_drops(base, (0, n // 2, n - 1), "deskew")
    add("general-dropped-deskew", xyz, 0.5, GENERAL, drop, entry="deskew")
    for m in (7, 8, 9, 16, 17):
        add(f"general-last-run-{m}", build(510 + m, pops_for_total(2100) + [m], 0.5), 0.5, GENERAL, entry="downsample")
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return tuple(cs)


def faces(leaf):
    """Points exactly on leaf faces: every coordinate from k * leaf (k negative, zero, positive; -0.0 beside +0.0) and the
    floats next to two of the faces — all triples of them, in a fixed random order."""
    lf = np.float32(leaf)
    vals = [np.float32(k) * lf for k in (-3, -2, -1, 1, 2, 3)] + [np.float32(-0.0), np.float32(0.0)]
    vals += [np.nextafter(lf, np.float32(0)), np.nextafter(-lf, np.float32(-1e9))]
    v = np.array(vals, np.float32)
    g = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g[np.random.default_rng(7).permutation(len(g))])


# ---- what the entry points are handed ---------------------------------------------------------------------------------------
def kept(case):
    """The points that reach the voxel grid, in input order."""
    return case.xyz if case.drop is None else case.xyz[~case.drop]


def motion(case, oracle):
    """(times f64 [n], states, Xt2) of the de-skew entries: two states at rest with identity poses around the kept points'
    stamps; a dropped point's stamp lies before them (in front of the first kept point), behind them, or — scan_deskew only —
    far behind them in the middle of the input."""
    n = len(case.xyz)
    times = T0 + DT * np.arange(n)
    drop = np.zeros(n, bool) if case.drop is None else case.drop
    k = np.flatnonzero(~drop)
    if len(k):
        ta, tb = times[k[0]], times[k[-1]]
        if case.entry == "deskew":
            mid = drop & (np.arange(n) > k[0]) & (np.arange(n) < k[-1])
            times[mid] = T0 + 50.0
    else:
        ta, tb = T0 - 2.0, T0 - 1.0          # every stamp lies behind the states
    rest = dict(a=(0.0, 0.0, -9.807), g=(0.0, 0.0, -9.807))   # State::propagate_f: v = R a - g = 0
    states = np.concatenate([oracle.motion_state(time=ta, **rest), oracle.motion_state(time=max(tb, ta + DT), **rest)])
    return times, states, states[1:2].copy()


WINDOW_FORMAT = dict(point_step=48, off_x=0, off_y=4, off_z=8, off_time=24, time_type=1, off_intensity=16, intensity_type=2,
                     off_range=0, range_type=0, relative_time=0)
INGEST = (int(T0 * 1e6), 0, 0, 0.1, 1, 0.0)    # every record is kept: no rate down-sampling, no range gate
WINDOW = (T0 - 1.0, T0 + 1.0)


def window_message(case, times):
    """The PointCloud2 payload (absolute f64 stamps) that puts the case's points, in input order, into the LiDAR buffer."""
    dt = cm._fields("hesai", False)
    assert dt.itemsize == WINDOW_FORMAT["point_step"] and dt.fields["timestamp"][1] == WINDOW_FORMAT["off_time"]
    rec = np.zeros(len(case.xyz), dt)
    rec["x"], rec["y"], rec["z"] = case.xyz[:, 0], case.xyz[:, 1], case.xyz[:, 2]
    rec["timestamp"] = times
    rec["intensity"] = np.arange(len(rec)) % 251
    return rec.tobytes()


def format_args():
    f = WINDOW_FORMAT
    return (f["point_step"], f["off_x"], f["off_y"], f["off_z"], f["off_time"], f["time_type"], f["off_intensity"], f["intensity_type"],
            f["off_range"], f["range_type"], f["relative_time"])


@functools.lru_cache(maxsize=None)
def _expected(name):
    import lvoracle as oracle

    oracle.build()
    case = next(c for c in cases() if c.name == name)
    if case.entry == "downsample":
        pts = kept(case)
    else:
        times, states, xt2 = motion(case, oracle)
        if case.entry == "window":
            buf = oracle.cloud_ingest(window_message(case, times), len(case.xyz), oracle.CloudFormat(*format_args()), oracle.IngestParams(*INGEST))
            sel = buf[(buf["time"] >= WINDOW[0]) & (buf["time"] <= WINDOW[1])]
            xyz, t = np.stack([sel["x"], sel["y"], sel["z"]], axis=1), sel["time"]
        else:
            xyz, t = case.xyz, times
        ok = (t >= states["time"][0]) & (t <= states["time"][-1]) & np.isfinite(xyz).all(axis=1)   # dropped points: removed
        pts = oracle.deskew(xyz[ok], t[ok], states, xt2)
    out = oracle.voxelgrid(pts, case.leaf) if len(pts) else np.zeros((0, 3), np.float32)
    out.setflags(write=False)
    pts = np.ascontiguousarray(pts, np.float32)
    pts.setflags(write=False)
    return pts, out


def voxel_input(case):
    """What the oracle's voxel grid is given: the kept points behind the oracle's ingest and de-skew."""
    return _expected(case.name)[0]


def expected(case):
    """oracle.voxelgrid(oracle.deskew(oracle.cloud_ingest(...))) of the case, computed once, read-only."""
    return _expected(case.name)[1]
