"""tests/rollout_ref.py against what it claims (CPU): its restated sine and cosine against numpy's, a straight run on an empty plan,
the six reasons by hand-made cases, the tie rule of `best`, and the closed loop the GPU test repeats on the device."""
import numpy as np

import plan_ref as pr
import rollout_cases as cases
import rollout_ref as rr

F = np.float32


def empty_plan(nx=20, ny=10, res=0.5, goal_cell=(18, 5)):
    """All cells of cost 1, and P = 20 * (|i - gi| + |j - gj|): a plan by hand."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    P = (20 * (np.abs(i - goal_cell[0]) + np.abs(j - goal_cell[1]))).astype(np.uint32)
    return dict(origin=(0.0, 0.0, 0.0), resolution=res, cost=np.ones((ny, nx), np.uint8), P=P)


def test_restated_sincos_against_numpy():
    """200,000 f32 arguments in [-8, 8): the restated sine and cosine, rounded to f32, equal np.float32(np.sin(np.float64(x))) and the
    same for cos on every one of them (0 differ: asserted).  The device is held to the restatement, not to a libm."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-8.0, 8.0, 199_000).astype(F), np.linspace(-8, 8, 1000, endpoint=False).astype(F)])
    sn, cs = rr.sincos(x)
    n_sin = np.count_nonzero(sn != np.sin(x.astype(np.float64)).astype(F))
    n_cos = np.count_nonzero(cs != np.cos(x.astype(np.float64)).astype(F))
    print("arguments", len(x), "sine differs", n_sin, "cosine differs", n_cos)
    assert len(x) >= 100_000 and n_sin == 0 and n_cos == 0


def test_sincos_quadrants_and_large_arguments():
    for x in (0.0, np.pi / 2, np.pi, -np.pi / 2, 3 * np.pi / 2, 100.0, -1000.5, 1048575.875, -1048575.875):
        sn, cs = rr.sincos(F(x))
        assert abs(float(sn) - np.sin(np.float64(F(x)))) < 1e-6 and abs(float(cs) - np.cos(np.float64(F(x)))) < 1e-6, x
    assert rr.usable(F(1048575.875)) and not rr.usable(F(1048576.0)) and not rr.usable(F(np.nan)) and not rr.usable(F(-np.inf))


def test_a_straight_run_on_an_empty_plan():
    plan = empty_plan()
    rp = rr.rparams(T=12, dt=0.5)
    out = rr.rollout(plan, None, rp, (1.25, 2.75, 0.0), np.array([[[1.0, 0.0]]], F))   # a cell a step, along +x in row 5
    r = out["results"][0]
    assert (r["status"], r["steps"], r["why"]) == (rr.CLEAR, 12, 0)
    assert r["cell_end"] == 5 * 20 + 14 and r["p_end"] == 20 * 4 and r["p_min"] == 20 * 4 and r["s_min"] == 12 and r["cost_sum"] == 12
    assert np.array_equal(out["poses"][0, :, 0], (1.25 + 0.5 * np.arange(13)).astype(F)) and np.all(out["poses"][0, :, 1] == F(2.75))
    assert out["score"][0] == 12 + 80 and list(out["best"]) == [0, 92]
    assert np.array_equal(out["poses"][0, 1], rr.step((1.25, 2.75, 0.0), 1.0, 0.0, 0.5))
    # Tc < T holds the last pair; a turn on the spot moves nothing
    two = rr.rollout(plan, None, dict(rp, T=8), (1.25, 0.25, 0.0), np.array([[[0.0, np.pi]], [[1.0, 0.0]]], F).reshape(1, 2, 2))
    assert two["results"]["steps"][0] == 8 and two["poses"][0, 1, 0] == F(1.25) and two["results"]["cell_end"][0] == 7 * 20 + 2


def test_each_reason_by_hand():
    plan = empty_plan()
    plan["cost"][5, 10] = 0
    field = dict(origin=plan["origin"], resolution=plan["resolution"], s2=np.full((10, 20), 100, np.int32))
    field["s2"][7, 4] = 3
    rp = rr.rparams(T=8, dt=0.5, fp_clear_s2=4)
    go = np.array([[[1.0, 0.0]]], F)

    def one(start, u=go, fp=None, **kw):
        out = rr.rollout(plan, field, dict(rp, **kw), start, u, fp)
        r = out["results"][0]
        return int(r["why"]), int(r["steps"]), out

    assert one((1.25, 2.75, 2.0e6))[:2] == (1, 0)                                         # 1: th0 not usable
    assert one((1.25, 2.75, 1048575.0), np.array([[[1.0, 2.0]]], F))[:2] == (2, 0)          # 2: th0 + 1 reaches 2^20
    assert one((1.25, 1.25, 0.0), np.array([[[0.0, np.nan]]], F))[:2] == (2, 0)
    why, steps, out = one((8.75, 1.25, 0.0))                                               # 3: out through the east border
    assert (why, steps) == (3, 2) and out["results"]["cell_end"][0] == 2 * 20 + 19
    assert one((1.25, 1.25, 0.0), np.array([[[np.inf, 0.0]]], F))[:2] == (3, 0)
    why, steps, out = one((3.75, 2.75, 0.0))                                               # 4: the blocked cell (10, 5)
    assert (why, steps) == (4, 2) and np.all(out["poses"][0, 3:].view(np.uint32) == rr.NAN_BITS) and out["poses"][0, 2, 0] == F(4.75)
    fp = np.array([[0.0, 0.0], [0.0, 1.0], [0.0, -0.6]], F)
    assert one((1.25, 0.25, 0.0), fp=fp)[:2] == (5, 0)                                     # 5: the right-hand point is below y = 0
    assert one((0.75, 2.75, 0.0), fp=fp)[:2] == (6, 2)                                     # 6: the left-hand point meets s2 = 3 at (4, 7)
    assert one((0.75, 2.75, 0.0), fp=fp, fp_clear_s2=3)[:2] == (0, 8)
    # 5 comes before 6 though the point that fails 6 has the lower index
    plan_b = dict(plan)
    field["s2"][0, 3] = 1
    assert one((1.25, 0.25, 0.0), fp=np.array([[0.0, 0.0], [0.0, -0.5]], F))[:2] == (5, 0)
    field["s2"][0, 3] = 100
    # pose 0 is not examined: a start in the blocked cell drives out of it
    why, steps, out = one((5.25, 2.75, 0.0))
    assert (why, steps) == (0, 8) and out["results"]["p_min"][0] < out["results"]["p_end"][0] + 1 and plan_b["cost"][5, 10] == 0


def test_best_takes_the_lower_index_of_equals():
    plan = empty_plan()
    u = np.array([[[0.5, 0.0]], [[1.0, 0.0]], [[0.0, 0.0]], [[1.0, 0.0]], [[np.nan, 0.0]]], F)
    out = rr.rollout(plan, None, rr.rparams(T=6, dt=0.5), (1.25, 2.75, 0.0), u)
    assert out["score"][1] == out["score"][3] < out["score"][0] < out["score"][2] and out["score"][4] == np.uint64(rr.NO_SCORE)
    assert list(out["best"]) == [1, int(out["score"][1])]
    assert list(rr.best_of(np.array([rr.NO_SCORE] * 3, np.uint64))) == [-1, -1]
    assert list(rr.best_of(np.array([7, 5, 5, 9], np.uint64))) == [1, 5]
    # goal_mode 1 scores the least P on the way; min_steps and w_stop
    loop = np.zeros((1, 12, 2), F)
    loop[0, :6, 0], loop[0, 6:, 0] = 2.0, -2.0
    res = rr.rollout(plan, None, rr.rparams(T=12, dt=0.5, goal_mode=1, w_cost=0), (1.25, 2.75, 0.0), loop)
    assert res["results"]["s_min"][0] == 6 and res["score"][0] == res["results"]["p_min"][0] < res["results"]["p_end"][0]
    res = rr.rollout(plan, None, rr.rparams(T=12, dt=0.5, min_steps=3, w_stop=7, w_cost=0, w_goal=0), (8.75, 1.25, 0.0),
                     np.array([[[1.0, 0.0]], [[0.5, 0.0]]], F))
    assert list(res["results"]["steps"]) == [2, 4] and res["score"][0] == np.uint64(rr.NO_SCORE) and res["score"][1] == 7 * 8


def test_the_cases_of_the_host_and_gpu_tests():
    cases.check_the_cases_do_what_they_are_for()


def test_closed_loop_reaches_the_goal_without_standing_in_a_blocked_cell(lv):
    """The loop of tests/test_gpu_occ_rollout.py on the reference alone: local_plan.drive with dwa on RefContext.  Every pose stands in
    a traversable cell, and the goal is reached within two cells in at most 300 iterations."""
    import rollout_loop as loop

    out = loop.run(rr.RefContext(*cases.world()))
    plan, _ = cases.world()
    ok, cell = pr.cells_of(cases.PRM, (1,) + plan["cost"].shape, True, np.c_[out["poses"][:, :2], np.zeros(len(out["poses"]))])
    assert ok.all() and np.all(plan["cost"][cell[:, 1], cell[:, 0]] != 0)
    assert out["reached"] and len(out["cmds"]) <= 300
    assert out["poses"][0, 0] < 3.0 < out["poses"][-1, 0]   # from one side of the wall to the other
    assert np.hypot(*(out["poses"][-1, :2] - cases.GOAL[0, :2])) <= 2 * 0.25
