"""Prelocalisation in a prior map: find the starting pose of a scan in a map that already exists (the reference's work in
progress, README.md:64-67, "Prelocalization with a previously saved HD map", and its TODO "Saving and loading HD-Maps",
README.md:117).  A grid of candidate poses around a rough prior is refined by lv_update_batch, the best few are refined again,
and the best one is returned.  save_map / load_map keep a map as a .npy of lv_map_fetch's output (map order = age)."""
from __future__ import annotations

import math

import numpy as np

from .synth import quat_from_rpy, quat_mul


def candidate_grid(prior_state, xy_radius: float, xy_step: float, yaw_span: float, yaw_step: float, z_offsets=(0.0,)) -> np.ndarray:
    """[m, 26] states around prior_state: every xy offset on a square grid of step xy_step within +-xy_radius, every yaw offset
    (radians) within +-yaw_span in steps of yaw_step, every z offset.  The yaw is applied on the world side of the prior's
    rotation, q = quat_mul(q_yaw, q_prior); everything else is the prior's.  Rows are ordered z, then yaw, then x, then y."""
    x0 = np.asarray(prior_state, np.float64).reshape(26)

    def axis(radius, step):
        k = int(math.floor(radius / step + 1e-9)) if step > 0 else 0
        return np.arange(-k, k + 1) * step

    dxy = axis(xy_radius, xy_step)
    dyaw = axis(yaw_span, yaw_step)
    out = []
    for dz in z_offsets:
        for a in dyaw:
            q = quat_mul(quat_from_rpy(0.0, 0.0, float(a)), x0[3:7])
            for dx in dxy:
                for dy in dxy:
                    s = x0.copy()
                    s[0] += dx
                    s[1] += dy
                    s[2] += dz
                    s[3:7] = q
                    out.append(s)
    return np.array(out).reshape(-1, 26)


def rank(passes, last) -> np.ndarray:
    """Order of the hypotheses, best first: more valid matches in the last pass first (n_valid descending), then the smaller mean
    squared residual (sum_h2 / n_valid ascending), then the lower index.  Hypotheses with n_valid == 0 come last, in index order.
    passes is accepted for the table a caller prints; it does not enter the order."""
    del passes
    n = np.array([int(d["n_valid"]) for d in last], np.int64)
    h2 = np.array([float(d["sum_h2"]) for d in last], np.float64)
    mean = np.where(n > 0, h2 / np.maximum(n, 1), np.inf)
    idx = np.arange(len(n))
    return np.array(sorted(idx, key=lambda i: (n[i] == 0, -n[i], mean[i], i)), np.int64)


def prelocalise(ctx, prior_state, P, rounds: int = 2, keep: int = 8, **grid):
    """Batch-update the candidate grid (candidate_grid(prior_state, **grid)) from the context's current scan against its map, keep
    the best `keep`, batch-update those again `rounds` times, and return (best state [26], table): table is a list of dicts
    {state, passes, n_valid, sum_h2} of the final round, best first."""
    table, _ = refine(ctx, candidate_grid(prior_state, **grid), P, rounds, keep)
    return table[0]["state"].copy(), table


def refine(ctx, xs, P, rounds: int = 2, keep: int = 8):
    """Batch-update the hypotheses xs ([m, 26]), keep the best `keep`, batch-update those again `rounds` times.  Returns (table,
    origin): table as prelocalise's, best first; origin[i] = the row of xs that table[i] grew from."""
    xs, _, passes, last = ctx.update_batch(xs, P)
    origin = rank(passes, last)[:keep]
    xs = xs[origin]
    for _ in range(rounds):
        xs, _, passes, last = ctx.update_batch(xs, P)
        order = rank(passes, last)
        xs, passes, last, origin = xs[order], passes[order], [last[i] for i in order], origin[order]
    table = [dict(state=xs[i].copy(), passes=int(passes[i]), n_valid=int(last[i]["n_valid"]), sum_h2=float(last[i]["sum_h2"]))
             for i in range(len(xs))]
    return table, origin


def save_map(ctx, path) -> None:
    """The context's map (lv_map_fetch: living points in map order, oldest first) to a .npy of [m, 3] float32."""
    np.save(path, ctx.map_fetch())


def load_map(ctx, path) -> None:
    """lv_map_build from a map saved by save_map (map order preserved)."""
    ctx.map_build(np.load(path))
