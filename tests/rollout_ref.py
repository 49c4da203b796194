"""The rollouts' rule (include/limovelo_hip.h "Rollouts") in numpy: what tests/test_occ_rollout_host.py holds the host build of
lv_rollout.hpp to and tests/test_gpu_occ_rollout.py the kernel, field for field and bit for bit.

  sincos     its own restatement of lv_sincos.hpp: the f32 argument widened to f64, k = rint(x * 2/pi), three Cody-Waite
             subtractions, the two polynomials in Horner form, the quadrant from int(k) & 3, rounded to f32.  numpy's f64
             operations are IEEE and unfused, so the same sequence gives the same bits.
  motion     np.float32 operations in the stated order: d = v * dt; x + d * cs; y + d * sn; th + w * dt.
  cells      grid_ref.cell_of (planar) with the plan's, respectively the field's, origin and resolution.
Vectorised over the K sequences (and the footprint points); the step loop is the rule's.  A plan is a dict(origin, resolution,
cost [ny, nx] uint8, P [ny, nx] uint32), a field a dict(origin, resolution, s2 [ny, nx] int32) or None; world() builds both through
distance_ref and plan_ref."""
import numpy as np

import distance_ref as dr
import grid_ref as gr
import plan_ref as pr

F = np.float32
CLEAR, STOPPED = 1, 2
UNREACHED = pr.UNREACHED
TH_LIMIT = F(1048576.0)
NAN_BITS = 0x7FC00000
NO_SCORE = 2 ** 64 - 1
RESULT_FIELDS = ("status", "steps", "why", "cell_end", "p_end", "p_min", "s_min", "cost_sum")
RESULT_DTYPE = np.dtype([(f, np.uint32 if f in ("p_end", "p_min", "cost_sum") else np.int32) for f in RESULT_FIELDS])


def rparams(**kw):
    """A plain dict of lv_rollout_params (the defaults of lv_default_rollout_params, overridden by kw)."""
    p = dict(T=32, Tc=1, dt=0.1, fp_clear_s2=1, w_cost=1, w_goal=1, w_stop=0, min_steps=1, goal_mode=0)
    p.update(kw)
    return p


def usable(th):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(th, F)) < TH_LIMIT   # (NaN fails)


def sincos(x):
    """(sn, cs) as f32 of the f32 values x, all usable."""
    x = np.asarray(x, F).astype(np.float64)
    k = np.rint(x * 0.63661977236758134308)
    r = x - k * 1.57079632673412561417e+00
    r = r - k * 6.07710050650619224932e-11
    r = r - k * 2.02226624879595063154e-21
    z = r * r
    ps = 1.58969099521155010221e-10
    ps = ps * z - 2.50507602534068634195e-08
    ps = ps * z + 2.75573137070700676789e-06
    ps = ps * z - 1.98412698298579493134e-04
    ps = ps * z + 8.33333333332248946124e-03
    ps = ps * z - 1.66666666666666324348e-01
    s0 = r + r * z * ps
    pc = -1.13596475577881948265e-11
    pc = pc * z + 2.08757232129817482790e-09
    pc = pc * z - 2.75573143513906633035e-07
    pc = pc * z + 2.48015872894767294178e-05
    pc = pc * z - 1.38888888888741095749e-03
    pc = pc * z + 4.16666666666666019037e-02
    c0 = 1.0 - 0.5 * z + z * z * pc
    q = k.astype(np.int64) & 3
    sd = np.where(q == 0, s0, np.where(q == 1, c0, np.where(q == 2, -s0, -c0)))
    cd = np.where(q == 0, c0, np.where(q == 1, -s0, np.where(q == 2, -c0, s0)))
    return sd.astype(F), cd.astype(F)


def _sincos_where(th, ok):
    return sincos(np.where(ok, th, F(0)))


def _cells(grid, x, y):
    """(ok, linear index; 0 where not ok) of the points (x, y) in grid = dict(origin, resolution, and an [ny, nx] array under key)."""
    ny, nx = grid["shape"]
    pts = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3)
    ok, v = gr.cell_of(grid["origin"], grid["resolution"], (nx, ny, 1), True, pts)
    return ok.reshape(x.shape), (v[:, 1] * nx + v[:, 0]).reshape(x.shape)


def step(pose, v, w, dt):
    """Pose s from pose s - 1 (f32 [3], its heading usable) by the motion rule alone."""
    x, y, th = (F(a) for a in pose)
    sn, cs = sincos(th)
    with np.errstate(all="ignore"):
        d = F(v) * F(dt)
        return np.array([x + d * cs, y + d * sn, th + F(w) * F(dt)], F)


def score_of(rp, res):
    """[K] uint64 from the records."""
    p_sel = (res["p_min"] if rp["goal_mode"] else res["p_end"]).astype(np.uint64)
    eligible = (res["steps"] >= rp["min_steps"]) & (p_sel != UNREACHED)
    s = (np.uint64(rp["w_cost"]) * res["cost_sum"].astype(np.uint64) + np.uint64(rp["w_goal"]) * p_sel
         + np.uint64(rp["w_stop"]) * (rp["T"] - res["steps"]).astype(np.uint64))
    return np.where(eligible, s, np.uint64(NO_SCORE))


def best_of(score):
    """[2] int64: the eligible index with the least (score, index) and its score; -1, -1 if none."""
    e = np.nonzero(score != np.uint64(NO_SCORE))[0]
    if not len(e):
        return np.array([-1, -1], np.int64)
    i = e[np.argmin(score[e])]   # (argmin takes the first of equals)
    return np.array([i, score[i]], np.int64)


def rollout(plan, field, rp, start, controls, footprint=None):
    """dict(results [K] RESULT_DTYPE, poses [K, T + 1, 3] f32, score [K] uint64, best [2] int64) of the sequences controls
    [K, Tc, 2] from the pose start."""
    u = np.asarray(controls, F).reshape(len(controls), -1, 2)
    K, Tc = u.shape[:2]
    T, dt, clear = rp["T"], F(rp["dt"]), rp["fp_clear_s2"]
    fp = np.zeros((0, 2), F) if footprint is None else np.asarray(footprint, F).reshape(-1, 2)
    pg = dict(origin=plan["origin"], resolution=plan["resolution"], shape=plan["cost"].shape)
    cost, P = plan["cost"].reshape(-1), plan["P"].reshape(-1)
    if len(fp):
        fg = dict(origin=field["origin"], resolution=field["resolution"], shape=field["s2"].shape)
        s2 = field["s2"].reshape(-1).astype(np.int64)
    x, y, th = (np.full(K, F(a), F) for a in np.asarray(start, F))
    ok_th = usable(th)
    sn, cs = _sincos_where(th, ok_th)
    res = np.zeros(K, RESULT_DTYPE)
    ok, lin = _cells(pg, x, y)
    res["cell_end"] = np.where(ok, lin, -1)
    res["p_end"] = res["p_min"] = np.where(ok, P[lin], UNREACHED)
    res["s_min"] = np.where(ok, 0, -1)
    poses = np.full((K, T + 1, 3), NAN_BITS, np.uint32).view(F)
    poses[:, 0] = np.stack([x, y, th], axis=1)
    alive = np.ones(K, bool)
    for s in range(1, T + 1):
        if not alive.any():
            break
        v, w = u[:, min(s - 1, Tc - 1), 0], u[:, min(s - 1, Tc - 1), 1]
        with np.errstate(all="ignore"):
            d = v * dt
            xn = x + d * cs
            yn = y + d * sn
            thn = th + w * dt
        ok_n = usable(thn)
        ok, lin = _cells(pg, xn, yn)
        c = np.where(ok, cost[lin], 0)
        bad = np.where(~ok_th, 1, np.where(~ok_n, 2, np.where(~ok, 3, np.where(c == 0, 4, 0))))
        snn, csn = _sincos_where(thn, ok_n)
        if len(fp):
            fx, fy = fp[None, :, 0], fp[None, :, 1]
            with np.errstate(all="ignore"):
                wx = xn[:, None] + (csn[:, None] * fx - snn[:, None] * fy)
                wy = yn[:, None] + (snn[:, None] * fx + csn[:, None] * fy)
            okf, linf = _cells(fg, wx, wy)
            low = okf & (s2[linf] < clear)
            bad = np.where(bad != 0, bad, np.where((~okf).any(axis=1), 5, np.where(low.any(axis=1), 6, 0)))
        stop, good = alive & (bad != 0), alive & (bad == 0)
        res["why"][stop] = bad[stop]
        alive &= ~stop
        x, y, th, sn, cs, ok_th = (np.where(good, n, o) for n, o in ((xn, x), (yn, y), (thn, th), (snn, sn), (csn, cs), (ok_n, ok_th)))
        res["steps"][good] = s
        res["cost_sum"][good] += c[good].astype(np.uint32)
        res["cell_end"][good] = lin[good]
        p = P[lin]
        res["p_end"][good] = p[good]
        lower = good & ((res["s_min"] < 0) | (p < res["p_min"]))
        res["p_min"][lower] = p[lower]
        res["s_min"][lower] = s
        poses[good, s] = np.stack([xn, yn, thn], axis=1)[good]
    res["status"] = np.where(res["why"] == 0, CLEAR, STOPPED)
    score = score_of(rp, res)
    return dict(results=res, poses=poses, score=score, best=best_of(score))


def world(prm, L, dp, pp, table, goals):
    """(plan, field, s2, cost, P) of a grid's log-odds through distance_ref.build and plan_ref.build (dp planar)."""
    s2, _ = dr.build(prm, L, dp)
    cost, P, _, _ = pr.build(prm, s2, pp, table, goals)
    plan = dict(origin=prm["origin"], resolution=prm["resolution"], cost=cost, P=P)
    field = dict(origin=prm["origin"], resolution=prm["resolution"], s2=s2)
    return plan, field


class RefContext:
    """Stands in for capi.Context in limo_velo_amd.local_plan: occ_rollout by this reference."""

    def __init__(self, plan, field):
        self.plan, self.field = plan, field

    def occ_rollout(self, start, controls, params=None, footprint=None, want=("results", "best")):
        rp = rparams() if params is None else {f: getattr(params, f) for f in rparams()}
        u = np.asarray(controls, F)
        rp["Tc"] = u.shape[1]
        out = rollout(self.plan, self.field, rp, start, u, footprint)
        return {k: out[k] for k in want}
