"""The world and the batches that tests/test_occ_rollout_host.py runs through the host build of lv_rollout.hpp and
tests/test_gpu_occ_rollout.py through the kernel, with their answers by tests/rollout_ref.py (computed once per process).

The world is a 45 x 38 x 3 grid of 0.25 m cells, all observed free, with a wall across it (columns 20 and 21) that has a gap of five
rows, and a closed box whose inside is free: traversable cells the goal cannot be reached from (P = UNREACHED).  The planar field
spans the three layers; the plan blocks every cell next to an obstacle (min_clear_s2 2) and has one goal right of the wall."""
import functools

import numpy as np

import distance_ref as dr
import occupancy_ref as ocr
import plan_ref as pr
import rollout_ref as rr

F = np.float32
NX, NY, NZ = 45, 38, 3
PRM = ocr.params(origin=(-2.0, -1.5, -0.1), resolution=0.25, nx=NX, ny=NY, nz=NZ, min_range=0.1, max_range=30.0)
DP = dr.dparams(planar=1, k_lo=0, k_hi=2)
PP = pr.pparams(connectivity=8, min_clear_s2=2)
TABLE = np.array([250, 120, 40, 10, 3, 1], np.uint8)
GOAL = np.array([[7.6, 2.9, 0.0]], F)
GAP_Y = 2.875            # the middle of the gap's middle row (j = 17)
POCKET = (7.1, 6.4)      # inside the box


def centre(i, j):
    return float(PRM["origin"][0]) + (i + 0.5) * 0.25, float(PRM["origin"][1]) + (j + 0.5) * 0.25


def grid():
    L = np.full((NZ, NY, NX), -1.0, F)
    L[:, :, 20:22] = 1.0
    L[:, 15:20, 20:22] = -1.0            # the gap: rows 15..19
    L[:, 27:35, 33:41] = 1.0             # the box ...
    L[:, 28:34, 34:40] = -1.0            # ... and its free inside
    return L


@functools.lru_cache(maxsize=None)
def world():
    """(plan, field) of rollout_ref."""
    return rr.world(PRM, grid(), DP, PP, TABLE, GOAL)


def rect(length, width, n):
    """n points round a rectangle's outline (n >= 1), x forward."""
    t = (np.arange(n) + 0.5) / n * 4.0
    side, u = np.floor(t).astype(int), t - np.floor(t)
    hx, hy = 0.5 * length, 0.5 * width
    x = np.choose(side, [hx - 2 * hx * u, np.full(n, -hx), -hx + 2 * hx * u, np.full(n, hx)])
    y = np.choose(side, [np.full(n, hy), hy - 2 * hy * u, np.full(n, -hy), -hy + 2 * hy * u])
    return np.stack([x, y], axis=1).astype(F)


def random_batch(seed, K, T, Tc, n_fp, **kw):
    """Commands of up to 2 m/s and 2 rad/s from a place left of the wall: with T = 64 some sequences leave the grid, some run into
    the wall, some pass the gap."""
    rng = np.random.default_rng(seed)
    u = np.stack([rng.uniform(-0.5, 2.0, (K, Tc)), rng.uniform(-2.0, 2.0, (K, Tc))], axis=-1).astype(F)
    start = np.array([rng.uniform(-1.0, 2.0), rng.uniform(1.5, 4.5), rng.uniform(-1.0, 1.0)], F)
    return dict(rp=rr.rparams(T=T, Tc=Tc, dt=0.1, fp_clear_s2=2, **kw), start=start, controls=u, fp=rect(0.7, 0.45, n_fp) if n_fp else None)


# (K, T, Tc, n_fp): every K, T, n_fp and both Tc of the issue's lists, every n_fp with Tc = 1 and with Tc = T
SHAPES = ([(1000, 17, 17, n) for n in (0, 1, 2, 3, 5, 33, 64)] + [(65, 64, 1, n) for n in (0, 1, 2, 3, 5, 33, 64)]
          + [(1, 1, 1, 0), (63, 2, 1, 5), (64, 2, 2, 0), (65, 1, 1, 3), (1, 64, 64, 2), (63, 17, 1, 64), (64, 64, 64, 33), (1000, 64, 1, 0)])


def turn_then_go(angles, T, v=2.0, dt=0.1):
    """[K, T, 2]: step 1 turns on the spot by angles[k], the rest drive straight on."""
    u = np.zeros((len(angles), T, 2), F)
    u[:, 0, 1] = np.asarray(angles, np.float64) / dt
    u[:, 1:, 0] = v
    return u


@functools.lru_cache(maxsize=None)
def batches():
    """name -> dict(rp, start, controls [K, Tc, 2], fp or None)."""
    out = {}
    for n, (K, T, Tc, n_fp) in enumerate(SHAPES):
        out[f"random_K{K}_T{T}_Tc{Tc}_fp{n_fp}"] = random_batch(100 + n, K, T, Tc, n_fp, goal_mode=n & 1, w_stop=3 * (n % 3), min_steps=min(T, n % 4))
    left, ahead = centre(0, 10), centre(12, 17)
    # every sequence stops at step 1: from the westmost column heading west, 0.3 m a step
    out["all_stop_at_1"] = dict(rp=rr.rparams(T=17, dt=0.1), start=np.array([left[0], left[1], np.pi], F),
                                controls=np.tile(np.array([[[3.0, 0.0]]], F), (130, 1, 1)), fp=None)
    # one sequence of the wavefront lives to T, the others die in steps 1..6
    u = np.zeros((64, 64, 2), F)
    u[:, :, 0] = 0.2
    u[:, 1:7, 0] = np.where(np.arange(6)[None, :] == (np.arange(64) % 6)[:, None], np.nan, 0.2)
    u[37, :, 0] = 0.2
    out["one_survivor"] = dict(rp=rr.rparams(T=64, Tc=64, dt=0.1), start=np.array([ahead[0], ahead[1], 0.3], F), controls=u, fp=rect(0.5, 0.3, 5))
    # through each border: east (through the gap), north, west, south
    out["borders"] = dict(rp=rr.rparams(T=64, Tc=64, dt=0.1), start=np.array([ahead[0], GAP_Y, 0.0], F),
                          controls=turn_then_go([0.0, np.pi / 2, np.pi, -np.pi / 2], 64), fp=None)
    # a start just outside the grid: standing still, driving in, driving away
    out["start_outside"] = dict(rp=rr.rparams(T=5, dt=0.1), start=np.array([-2.1, 1.0, 0.0], F),
                                controls=np.array([[[0.0, 0.0]], [[2.0, 0.0]], [[-2.0, 0.0]], [[2.0, 1.0]]], F), fp=None)
    # a start in a blocked cell next to the wall, heading west: driving out, standing still, backing into the wall
    wall = centre(19, 8)
    out["start_blocked"] = dict(rp=rr.rparams(T=6, dt=0.1, goal_mode=1), start=np.array([wall[0], wall[1], np.pi], F),
                                controls=np.array([[[2.0, 0.0]], [[0.0, 0.0]], [[-2.0, 0.0]], [[2.0, 0.5]]], F), fp=None)
    # NaN and inf in the middle of a sequence (step 9 of 17), in v and in w
    u = np.tile(np.array([[[0.5, 0.2]]], F), (9, 17, 1))
    for k, (c, val) in enumerate([(0, np.nan), (0, np.inf), (0, -np.inf), (1, np.nan), (1, np.inf), (1, -np.inf), (0, 3e38), (1, 3e38)]):
        u[k, 8, c] = val
    out["nan_inf_mid"] = dict(rp=rr.rparams(T=17, Tc=17, dt=0.1), start=np.array([ahead[0], ahead[1], 0.0], F), controls=u, fp=rect(0.5, 0.3, 3))
    # headings at and beyond the bound (2^20), and one step short of it (f32 spacing there is 1/8: w * dt = 1/8 reaches it)
    two = np.array([[[0.5, 0.0]], [[0.5, 1.25]], [[0.5, -1.25]]], F)
    for name, th in (("th0_at_limit", 1048576.0), ("th0_at_minus_limit", -1048576.0), ("th0_beyond", 2.0e6), ("th0_nan", np.nan),
                     ("th0_inf", np.inf), ("th0_below_limit", 1048575.875), ("th0_above_minus_limit", -1048575.875)):
        out[name] = dict(rp=rr.rparams(T=4, dt=0.1), start=np.array([ahead[0], ahead[1], th], F), controls=two, fp=rect(0.5, 0.3, 2))
    # the centre inside, footprint points outside: a long robot near the south border, turning
    south = centre(10, 1)
    out["fp_outside"] = dict(rp=rr.rparams(T=17, dt=0.1), start=np.array([south[0], south[1], 0.0], F),
                             controls=np.array([[[0.5, 0.0]], [[0.5, 1.5]], [[0.5, -1.5]], [[0.0, 2.0]]], F), fp=rect(1.6, 0.3, 33))
    # reason 5 before reason 6 whatever the points' order: a wide robot three cells from the wall and one from the north border,
    # its outline reversed and begun at the middle of the front, so that front points (too near the wall: 6) come before the ones on its left (outside: 5)
    north = centre(17, 36)
    out["fp_5_before_6"] = dict(rp=rr.rparams(T=17, dt=0.1, fp_clear_s2=9), start=np.array([north[0], north[1], 0.0], F),
                                controls=np.array([[[0.1, 0.0]], [[0.1, 0.3]], [[-0.5, 0.0]]], F), fp=np.roll(rect(0.6, 1.1, 64)[::-1], -8, axis=0).copy())
    # ties: sequences 2 and 5 are the best and equal, 0 and 7 equal too
    u = np.array([[[0.3, 0.1]], [[0.2, 0.0]], [[1.0, 0.05]], [[0.0, 0.0]], [[0.9, 0.0]], [[1.0, 0.05]], [[-0.2, 0.0]], [[0.3, 0.1]]], F)
    out["ties"] = dict(rp=rr.rparams(T=17, dt=0.1, w_cost=0), start=np.array([ahead[0], GAP_Y, 0.0], F), controls=u, fp=None)
    # nobody eligible: in the box every P is UNREACHED; and min_steps nobody meets
    out["none_in_pocket"] = dict(rp=rr.rparams(T=5, dt=0.1), start=np.array([POCKET[0], POCKET[1], 1.0], F),
                                 controls=np.array([[[0.3, 0.0]], [[0.0, 1.0]], [[3.0, 0.0]]], F), fp=None)
    out["none_min_steps"] = dict(out["borders"], rp=rr.rparams(T=64, Tc=64, dt=0.1, min_steps=64))
    return out


@functools.lru_cache(maxsize=None)
def answers():
    """name -> rollout_ref.rollout's dict."""
    plan, field = world()
    return {name: rr.rollout(plan, field, b["rp"], b["start"], b["controls"], b["fp"]) for name, b in batches().items()}


def check_the_cases_do_what_they_are_for():
    """The answers show what each batch was made for (asserted on the reference, so on whatever equals it)."""
    a = {k: v["results"] for k, v in answers().items()}
    plan, _ = world()
    assert (plan["cost"][29:33, 35:39] != 0).all() and (plan["P"][28:34, 34:40] == rr.UNREACHED).all()   # the pocket
    assert np.all(a["all_stop_at_1"]["steps"] == 0) and np.all(a["all_stop_at_1"]["why"] == 3) and answers()["all_stop_at_1"]["best"][0] == -1
    s = a["one_survivor"]
    assert s["status"][37] == rr.CLEAR and s["steps"][37] == 64 and np.all(np.delete(s["steps"], 37) <= 6) and np.all(np.delete(s["why"], 37) == 3)
    b = a["borders"]
    assert np.all(b["why"] == 3) and np.all(b["steps"] > 10)
    i, j = b["cell_end"] % NX, b["cell_end"] // NX
    assert (i[0], j[1], i[2], j[3]) == (NX - 1, NY - 1, 0, 0)
    o = a["start_outside"]
    assert list(o["steps"]) == [0, 5, 0, 5] and list(o["cell_end"][[0, 2]]) == [-1, -1] and list(o["s_min"][[0, 2]]) == [-1, -1] and np.all(o["s_min"][[1, 3]] >= 1)
    k = a["start_blocked"]
    assert list(k["why"]) == [0, 4, 4, 0] and list(k["steps"]) == [6, 0, 0, 6] and k["p_min"][0] < rr.UNREACHED and k["s_min"][0] >= 1 and k["s_min"][1] == 0
    n = a["nan_inf_mid"]
    assert list(n["steps"]) == [8] * 8 + [17] and list(n["why"]) == [3, 3, 3, 2, 2, 2, 3, 2, 0]
    for name in ("th0_at_limit", "th0_at_minus_limit", "th0_beyond", "th0_nan", "th0_inf"):
        assert np.all(a[name]["why"] == 1) and np.all(a[name]["steps"] == 0) and np.all(a[name]["cell_end"] >= 0)
    assert list(a["th0_below_limit"]["why"]) == [0, 2, 0] and list(a["th0_above_minus_limit"]["why"]) == [0, 0, 2]
    assert list(a["th0_below_limit"]["steps"]) == [4, 0, 4]
    assert 5 in a["fp_outside"]["why"] and a["fp_outside"]["why"][0] == 0
    assert np.all(a["fp_5_before_6"]["why"] == 5) and np.all(a["fp_5_before_6"]["steps"] == 0)
    plan_, field = world()
    b5 = batches()["fp_5_before_6"]
    pose1 = rr.step(b5["start"], 0.1, 0.0, 0.1)
    ok, lin = rr._cells(dict(origin=field["origin"], resolution=field["resolution"], shape=field["s2"].shape), pose1[0] + b5["fp"][:, 0],
                        pose1[1] + b5["fp"][:, 1])
    low = ok & (field["s2"].reshape(-1)[lin] < 9)
    assert low.any() and (~ok).any() and np.nonzero(low)[0].min() < np.nonzero(~ok)[0].min()   # a 6 at a lower index than any 5
    t = answers()["ties"]
    assert t["best"][0] == 2 and t["score"][2] == t["score"][5] == t["score"].min() and t["score"][0] == t["score"][7]
    p = answers()["none_in_pocket"]
    assert p["best"][0] == -1 and p["best"][1] == -1 and p["results"]["status"][0] == rr.CLEAR and np.all(p["score"] == np.uint64(rr.NO_SCORE))
    assert answers()["none_min_steps"]["best"][0] == -1
    whys = np.concatenate([v["why"] for v in a.values()])
    assert set(whys) == {0, 1, 2, 3, 4, 5, 6}
    big = a["random_K1000_T64_Tc1_fp0"]
    assert (big["status"] == rr.CLEAR).sum() > 20 and (big["why"] == 3).sum() > 20 and (big["why"] == 4).sum() > 20
