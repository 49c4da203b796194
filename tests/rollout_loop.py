"""The closed loop that tests/test_rollout_ref.py runs on the reference and tests/test_gpu_occ_rollout.py on the device:
limo_velo_amd.local_plan.drive with dwa in the world of tests/rollout_cases.py, from left of the wall through the gap to the goal.
A 0.4 m x 0.3 m robot (the gap leaves three traversable rows, 0.75 m), commands up to 1 m/s, 0.2 s a step: 0.2 m, under the
0.25 m of a cell."""
import numpy as np

import rollout_cases as cases

START = (-0.9, 6.6, -1.2)
DT = 0.2
LIMITS = dict(v_min=0.0, v_max=1.0, w_min=-1.5, w_max=1.5, acc_v=2.0, acc_w=6.0)
GOAL_TOL = 0.5   # two cells


def run(ctx, n_iter=300):
    from limo_velo_amd import capi, local_plan as lp

    fp = lp.footprint_points(0.4, 0.3, 0.1)
    prm = capi.default_rollout_params(T=8, dt=DT, fp_clear_s2=1, w_cost=1, w_goal=4, w_stop=50, min_steps=2)

    def step_fn(c, pose, vel):
        return lp.dwa(c, pose, vel, LIMITS, nv=5, nw=11, window=0.5, params=prm, footprint=fp)["cmd"]

    return lp.drive(ctx, START, step_fn, n_iter, goal=cases.GOAL[0, :2], goal_tol=GOAL_TOL, dt=DT)
