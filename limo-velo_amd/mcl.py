"""Monte Carlo localisation in a saved occupancy grid on top of lv_occ_mcl_weigh (include/limovelo_hip.h "Localisation"): what amcl
does in a navigation stack.  The device weighs the particles against a scan by the likelihood field (a lookup of every scan end
point in the distance field last built); everything round that call runs here on the host in numpy, seeded by the caller's
np.random.Generator: the tables, the particle sets, the odometry motion model, an exact integer resampling rule, the estimate, and
the loop.

  likelihood_table()    the cost of an end point by its squared voxel distance to the nearest obstacle (Probabilistic Robotics,
                        table 6.3, as integers)
  weight_table()        the weight of a particle by its score above the best one
  beams_from_scan()     a scan's end points, subsampled
  uniform_particles(), gaussian_particles()   global and local initialisation
  move()                sample_motion_model_odometry (Probabilistic Robotics, table 5.6)
  weigh()               lv_occ_mcl_weigh
  resample(), n_eff(), estimate()
  step(), track()       one cycle, and the loop
  DeviceFilter          the same loop with the particles resident on the device (lv_occ_mcl_filter_*), with the filter's own
                        reproducible noise; motion_sigmas(), estimate_from_stats() serve it

A pose is (x, y, z, th): the robot moves in the plane, z places the scan in a 3-D field.  `ctx` is a capi.Context whose grid holds
the map (occupancy.load_grid) and whose distance field is built (ctx.occ_distance_build)."""
from __future__ import annotations

import math

import numpy as np

from . import capi

NO_SCORE = capi.MCL_NO_SCORE
MAX_COST = 1 << 24     # of a table entry (lv_occ_mcl_weigh)
MAX_WEIGHT = 1 << 20   # of a weight-table entry


def likelihood_table(resolution: float, sigma_hit: float, z_hit: float = 0.95, z_rand: float = 0.05, max_range: float = 30.0,
                     scale: float = 64.0, n_table: int = 1024) -> np.ndarray:
    """[n_table] uint32: entry s2 is round(scale * -ln(z_hit * exp(-s2 resolution^2 / (2 sigma_hit^2)) + z_rand / max_range)) less the
    table's minimum: the negative log-likelihood of an end point s2 squared voxels from the nearest obstacle, in units of 1 / scale
    nats.  The last entry serves every larger distance."""
    if not (1 <= int(n_table) <= 4096):
        raise ValueError("n_table: 1..4096")
    if not (sigma_hit > 0 and resolution > 0 and max_range > 0 and z_hit >= 0 and z_rand >= 0 and z_hit + z_rand > 0):
        raise ValueError("likelihood_table: resolution, sigma_hit, max_range > 0; z_hit, z_rand >= 0 and not both 0")
    s2 = np.arange(int(n_table), dtype=np.float64)
    with np.errstate(divide="ignore"):
        nll = -np.log(z_hit * np.exp(-s2 * float(resolution) ** 2 / (2.0 * float(sigma_hit) ** 2)) + z_rand / float(max_range))
    nll = np.where(np.isfinite(nll), nll, np.finfo(np.float64).max)
    t = np.minimum(np.rint(float(scale) * (nll - nll.min())), float(MAX_COST))
    return t.astype(np.uint32)


def weight_table(scale: float = 64.0, temperature: float = 1.0, n_w: int = 4096, shift: int = 0) -> np.ndarray:
    """[n_w] uint32: entry d is round(2^20 exp(-(d << shift) / (scale temperature))), the weight of a particle whose score lies
    d << shift above the best one.  temperature > 1 flattens the weights (beams are not independent: amcl's squashing)."""
    if not (int(n_w) >= 1 and scale > 0 and temperature > 0 and int(shift) >= 0):
        raise ValueError("weight_table: n_w >= 1, scale > 0, temperature > 0, shift >= 0")
    d = np.arange(int(n_w), dtype=np.float64) * float(1 << int(shift))
    return np.rint(float(MAX_WEIGHT) * np.exp(-d / (float(scale) * float(temperature)))).astype(np.uint32)


def beams_from_scan(points, n_beams: int, max_range: float) -> np.ndarray:
    """[<= n_beams, 3] f32: the returns of a scan (end points [n, 3] in the body frame) that are finite and nearer than max_range,
    subsampled evenly in their order."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = np.sqrt((p ** 2).sum(axis=1))
        p = p[np.isfinite(r) & (r > 0.0) & (r < float(max_range))]
    n = min(int(n_beams), len(p))
    if n < 1:
        return np.zeros((0, 3), np.float32)
    return p[(np.arange(n) * len(p)) // n].astype(np.float32)


def field_of(ctx) -> dict:
    """dict(origin [3], resolution, s2) of the distance field last built: s2 [ny, nx] of a planar field, [nz, ny, nx] of a 3-D one.
    The origin is the one the field was built at (a later lv_volume_recentre moves the grid, not the field)."""
    p = ctx.occ_params()
    sh = ctx.volume_shift_info()
    res = float(p.resolution)
    origin = [float(p.origin[a]) - (int(sh.grid[a]) - int(sh.field[a])) * res for a in range(3)]
    return dict(origin=origin, resolution=res, s2=ctx.occ_distance_fetch(metres=False)[0])


def uniform_particles(ctx, K: int, rng, z: float = 0.0, min_clear_s2: int = 1, field: dict | None = None) -> np.ndarray:
    """[K, 4] f32 poses drawn uniformly over the field's cells with s2 >= min_clear_s2 (in a 3-D field: of the layer that holds
    z), uniformly inside the cell, with a uniform heading.  field: field_of(ctx) when the caller has it already."""
    f = field if field is not None else field_of(ctx)
    s2 = np.asarray(f["s2"])
    res = float(f["resolution"])
    if s2.ndim == 3:
        k = int(math.floor((float(z) - float(f["origin"][2])) / res))
        if not 0 <= k < s2.shape[0]:
            raise ValueError("uniform_particles: z is outside the field")
        s2 = s2[k]
    free = np.flatnonzero(s2.reshape(-1) >= int(min_clear_s2))
    if not len(free):
        raise ValueError("uniform_particles: no cell with s2 >= min_clear_s2")
    c = free[rng.integers(0, len(free), int(K))]
    u = rng.uniform(0.0, 1.0, (int(K), 2))
    nx = s2.shape[1]
    out = np.empty((int(K), 4), np.float64)
    out[:, 0] = float(f["origin"][0]) + ((c % nx) + u[:, 0]) * res
    out[:, 1] = float(f["origin"][1]) + ((c // nx) + u[:, 1]) * res
    out[:, 2] = float(z)
    out[:, 3] = rng.uniform(-math.pi, math.pi, int(K))
    return out.astype(np.float32)


def gaussian_particles(pose, sigma_xy: float, sigma_th: float, K: int, rng) -> np.ndarray:
    """[K, 4] f32 poses round pose = (x, y, z, th): x and y with sigma_xy, th with sigma_th, z as given."""
    x, y, z, th = (float(v) for v in pose)
    out = np.empty((int(K), 4), np.float64)
    out[:, 0] = x + rng.normal(0.0, float(sigma_xy), int(K))
    out[:, 1] = y + rng.normal(0.0, float(sigma_xy), int(K))
    out[:, 2] = z
    out[:, 3] = th + rng.normal(0.0, float(sigma_th), int(K))
    return out.astype(np.float32)


def odometry_delta(prev, cur):
    """(rot1, trans, rot2) that takes the odometry pose prev = (x, y, th) to cur (Probabilistic Robotics, table 5.6, lines 2-4)."""
    dx, dy = float(cur[0]) - float(prev[0]), float(cur[1]) - float(prev[1])
    trans = math.hypot(dx, dy)
    rot1 = math.atan2(dy, dx) - float(prev[2]) if trans > 1e-9 else 0.0
    rot1 = math.atan2(math.sin(rot1), math.cos(rot1))
    rot2 = float(cur[2]) - float(prev[2]) - rot1
    return rot1, trans, math.atan2(math.sin(rot2), math.cos(rot2))


def move(poses, delta, alphas, rng) -> np.ndarray:
    """[K, 4] f32: every pose moved by its own sample of the odometry motion model (Probabilistic Robotics, table 5.6) for the
    odometry step delta = (rot1, trans, rot2) (odometry_delta) with the noise parameters alphas = (a1, a2, a3, a4).  Headings are
    wrapped to [-pi, pi); z stays."""
    x = np.asarray(poses, np.float32).reshape(-1, 4).astype(np.float64)
    rot1, trans, rot2 = (float(v) for v in delta)
    a1, a2, a3, a4 = (float(v) for v in alphas)
    K = len(x)
    r1 = rot1 - rng.normal(0.0, 1.0, K) * math.sqrt(a1 * rot1 ** 2 + a2 * trans ** 2)
    tr = trans - rng.normal(0.0, 1.0, K) * math.sqrt(a3 * trans ** 2 + a4 * rot1 ** 2 + a4 * rot2 ** 2)
    r2 = rot2 - rng.normal(0.0, 1.0, K) * math.sqrt(a1 * rot2 ** 2 + a2 * trans ** 2)
    out = x.copy()
    out[:, 0] += tr * np.cos(x[:, 3] + r1)
    out[:, 1] += tr * np.sin(x[:, 3] + r1)
    th = x[:, 3] + r1 + r2
    out[:, 3] = (th + math.pi) % (2.0 * math.pi) - math.pi
    return out.astype(np.float32)


def weigh(ctx, poses, beams, table, out_cost: int | None = None, min_inside: int = 1, want=("score", "n_in", "best")) -> dict:
    """lv_occ_mcl_weigh of the poses [K, 4] under the beams [B, 3] (beams_from_scan) and the table (likelihood_table): a dict of
    score [K] uint64 (NO_SCORE: not eligible), n_in [K] uint32 and best [2] int64, those of `want`.  out_cost: what an end point
    outside the field costs (default: the table's last entry, the cost of open space); a particle with fewer than min_inside end
    points inside the field is not eligible."""
    t = np.ascontiguousarray(table, np.uint32)
    p = capi.MclParams(int(t[-1]) if out_cost is None else int(out_cost), int(min_inside))
    return ctx.occ_mcl_weigh(poses, beams, t, p, want)


def _weights(score, wtable, shift):
    """(w [K] int64, s_min): resample's w_i and the least eligible score (-1 when there is none)."""
    s = np.asarray(score, np.uint64).reshape(-1)
    wt = np.asarray(wtable, np.uint32).astype(np.int64)
    if wt.max(initial=0) > MAX_WEIGHT:
        raise ValueError("weight-table entries are at most 2^20")
    ok = s != np.uint64(NO_SCORE)
    if not ok.any():
        return np.zeros(len(s), np.int64), -1
    s_min = s[ok].min()
    d = (np.where(ok, s, s_min) - s_min) >> np.uint64(int(shift))
    return np.where(ok, wt[np.minimum(d, np.uint64(len(wt) - 1)).astype(np.int64)], 0), int(s_min)


def weights(score, wtable, shift: int = 0) -> np.ndarray:
    """[K] int64: resample's w_i."""
    return _weights(score, wtable, shift)[0]


def resample(score, wtable, shift: int, draw: int, M: int):
    """The systematic resampling of M particles as an exact integer rule: (ancestors [M] int64, W, sum of w^2, s_min).
    w_i = 0 where score_i is NO_SCORE, else wtable[min((score_i - s_min) >> shift, n_w - 1)] with s_min the least eligible score;
    C = the inclusive prefix sums, W = the total, r = draw mod W, t_j = (j W + r) // M, ancestors[j] = the smallest i with
    C_i > t_j.  With W = 0 every ancestor is -1 (and s_min -1 when no score is eligible)."""
    w, s_min = _weights(score, wtable, shift)
    M = int(M)
    C = np.cumsum(w)
    W = int(C[-1]) if len(C) else 0
    if W == 0:
        return np.full(M, -1, np.int64), 0, 0, s_min
    r = int(draw) % W
    t = (np.arange(M, dtype=np.int64) * W + r) // M   # (below 2^20 * 2^40)
    return np.searchsorted(C, t, side="right").astype(np.int64), W, int((w * w).sum()), s_min


def n_eff(W: int, sum_w2: int) -> float:
    """The effective number of particles W^2 / sum w^2 (0 with no weight)."""
    return float(W) * float(W) / float(sum_w2) if sum_w2 else 0.0


def estimate(poses, w) -> np.ndarray:
    """[4] f64: the weighted mean of x, y, z and the circular mean of th (NaN with no weight)."""
    x = np.asarray(poses, np.float64).reshape(-1, 4)
    w = np.asarray(w, np.float64).reshape(-1)
    tot = w.sum()
    if not tot > 0:
        return np.full(4, np.nan)
    m = (x[:, :3] * w[:, None]).sum(axis=0) / tot
    return np.array([m[0], m[1], m[2], math.atan2((w * np.sin(x[:, 3])).sum(), (w * np.cos(x[:, 3])).sum())])


def step(ctx, poses, acc, delta, beams, table, wtable, rng, alphas=(0.05, 0.05, 0.05, 0.05), shift: int = 0, resample_below: float = 0.5,
         out_cost: int | None = None, min_inside: int = 1) -> dict:
    """One cycle: move the poses by the odometry step delta, weigh them under the scan, add the scores to acc (the particles'
    scores since the last resampling, [K] uint64; NO_SCORE stays), take the estimate, and resample when n_eff falls below
    resample_below * K.  Returns dict(poses, acc) to carry on with, and moved (the poses that were weighed), score, n_in, best,
    estimate, n_eff, resampled."""
    moved = move(poses, delta, alphas, rng)
    out = weigh(ctx, moved, beams, table, out_cost, min_inside)
    score = np.asarray(out["score"], np.uint64)
    acc = np.asarray(acc, np.uint64)
    gone = (score == np.uint64(NO_SCORE)) | (acc == np.uint64(NO_SCORE))
    total = np.where(gone, np.uint64(NO_SCORE), np.where(gone, np.uint64(0), acc) + np.where(gone, np.uint64(0), score))
    K = len(moved)
    anc, W, sw2, _ = resample(total, wtable, shift, int(rng.integers(0, 1 << 62)), K)
    ne = n_eff(W, sw2)
    est = estimate(moved, weights(total, wtable, shift))
    resampled = W > 0 and ne < float(resample_below) * K
    if resampled:
        moved_next, total = moved[anc], np.zeros(K, np.uint64)
    else:
        moved_next = moved
    return dict(poses=moved_next, acc=total, moved=moved, score=score, n_in=out["n_in"], best=out["best"], estimate=est, n_eff=ne,
                resampled=bool(resampled))


def track(ctx, poses, deltas, scans, table, wtable, rng, **kw) -> list:
    """The loop: step() for every (delta, beams) of zip(deltas, scans), starting from poses [K, 4].  Returns the steps' dicts."""
    x = np.asarray(poses, np.float32).reshape(-1, 4)
    acc = np.zeros(len(x), np.uint64)
    history = []
    for delta, beams in zip(deltas, scans):
        s = step(ctx, x, acc, delta, beams, table, wtable, rng, **kw)
        x, acc = s["poses"], s["acc"]
        history.append(s)
    return history


# ---- the resident filter (include/limovelo_hip.h "Resident localisation filter"): the same loop with the particles on the device
def motion_sigmas(delta, alphas) -> np.ndarray:
    """[3] f32: the standard deviations of (rot1, trans, rot2) for the odometry step delta under the noise parameters alphas =
    (a1, a2, a3, a4), as move() takes them (Probabilistic Robotics, table 5.6, lines 5-7)."""
    rot1, trans, rot2 = (float(v) for v in delta)
    a1, a2, a3, a4 = (float(v) for v in alphas)
    return np.array([math.sqrt(a1 * rot1 ** 2 + a2 * trans ** 2), math.sqrt(a3 * trans ** 2 + a4 * rot1 ** 2 + a4 * rot2 ** 2),
                     math.sqrt(a1 * rot2 ** 2 + a2 * trans ** 2)], np.float32)


def estimate_from_stats(stats) -> np.ndarray:
    """[4] f64: the pose of a resampling call's statistics (capi.MclFilterStats): per axis origin + resolution * (S / W + 0.5) / 256,
    the middle of the mean sub-unit, and atan2(S[3], S[4]) (NaN with no weight)."""
    W = int(stats.W)
    if W <= 0:
        return np.full(4, np.nan)
    res = float(stats.resolution)
    xyz = [float(stats.origin[a]) + res * (int(stats.S[a]) / W + 0.5) / 256.0 for a in range(3)]
    return np.array(xyz + [math.atan2(float(int(stats.S[3])), float(int(stats.S[4])))])


def below_fraction(resample_below: float):
    """(below_num, below_den) of lv_mcl_resample_params for the threshold n_eff < resample_below * K: 65536ths, at least one."""
    return min(max(int(round(float(resample_below) * 65536.0)), 1), 65536), 65536


class DeviceFilter:
    """The particle filter with its particles resident on the device.  ctx: a capi.Context whose grid holds the map and whose
    distance field is built; poses [K, 4]; seed: of the filter's own noise (every draw is a function of seed, epoch and particle).
    Only the seven occ_mcl_filter_* calls of the context are used."""

    def __init__(self, ctx, poses, seed: int = 0):
        self.ctx = ctx
        ctx.occ_mcl_filter_set(np.asarray(poses, np.float32).reshape(-1, 4), int(seed))

    def move(self, delta, alphas=(0.05, 0.05, 0.05, 0.05)) -> None:
        self.ctx.occ_mcl_filter_move(np.asarray(delta, np.float32), motion_sigmas(delta, alphas))

    def weigh(self, beams, table, out_cost: int | None = None, min_inside: int = 1, want_best: bool = True):
        """The measurement update; best [2] int64 of this scan (None when not asked for: the call then does not wait)."""
        t = np.ascontiguousarray(table, np.uint32)
        p = capi.MclParams(int(t[-1]) if out_cost is None else int(out_cost), int(min_inside))
        return self.ctx.occ_mcl_filter_weigh(beams, t, p, want_best)

    def resample(self, wtable, shift: int = 0, mode: int = 1, resample_below: float = 0.5, want_ancestors: bool = False):
        """(statistics, ancestors or None) of lv_occ_mcl_filter_resample."""
        num, den = below_fraction(resample_below)
        return self.ctx.occ_mcl_filter_resample(wtable, capi.MclResampleParams(int(shift), int(mode), num, den), want_ancestors)

    def poses(self) -> np.ndarray:
        return self.ctx.occ_mcl_filter_get(("poses",))["poses"]

    def step(self, delta, beams, table, wtable, alphas=(0.05, 0.05, 0.05, 0.05), shift: int = 0, resample_below: float = 0.5,
             out_cost: int | None = None, min_inside: int = 1, mode: int = 1, fetch: bool = True) -> dict:
        """One cycle, as step(): move, weigh, the estimate, and the resampling when n_eff falls below resample_below * K.  Returns
        dict(best, estimate, n_eff, resampled, stats) and with fetch also poses, acc and n_in as they stand after the cycle and
        moved, the poses that were weighed (two downloads a cycle: without fetch nothing of size K leaves the device)."""
        self.move(delta, alphas)
        best = self.weigh(beams, table, out_cost, min_inside)
        out = {}
        if fetch:
            out["moved"] = self.poses()
        stats, _ = self.resample(wtable, shift, mode, resample_below)
        out.update(best=best, estimate=estimate_from_stats(stats), n_eff=n_eff(int(stats.W), int(stats.sum_w2)), resampled=bool(stats.resampled),
                   stats=stats)
        if fetch:
            out.update(self.ctx.occ_mcl_filter_get())
        return out

    def track(self, deltas, scans, table, wtable, **kw) -> list:
        """The loop: step() for every (delta, beams) of zip(deltas, scans).  Returns the steps' dicts."""
        return [self.step(delta, beams, table, wtable, **kw) for delta, beams in zip(deltas, scans)]
