"""The 23-dof filter algebra on the device (lv_manifold.hpp: hand-written ddiv / dsincos / datan / datan2, FMA-contracted)
beyond the small-angle side of its branches, through the existing C ABI only.

(a) solve_kernel<6 | 12> + solve_prep with injected records: the split form of the multi-GPU path (HipEngine: the sums record
    is a torch tensor) lets a test overwrite what the reduction produced with a record of tests/filter_cases.py before the
    solve reads it.  Final x, P and pass count against the chained oracle.kf_step at the project's 1e-9.
(b) the one-launch pass (pass_kernel's closing part) and the three-kernel route from real scenes that start 2 / 5 / 8 degrees
    off, per pass against oracle.kf_step fed with the device's own sums.
(c) lv_predict, one step per case, |gyro - bg| dt from 0.004 to 9 rad: against oracle.predict at 1e-12, and its state half
    against the 50-digit statement of tests/manifold_mp.py.
The oracle restates the device's formulas in libm arithmetic; tests/test_filter_cases_ref.py anchors it to 50 digits and shows
that every case is conditioned two decades below the bounds used here."""
import numpy as np
import pytest

import filter_cases as fc
import manifold_mp as mm

pytestmark = pytest.mark.gpu

TOL_STATE = 1e-9   # tests/test_gpu_configs.py, tests/test_gpu_parity.py
CASE_NAMES = [f"{n}-ext{ext}" for ext in (0, 1) for n in
              ("rot0.01", "rot0.022", "rot0.0222", "rot0.3", "rot2", "rot3", "rot4", "grav-tilted-3deg", "grav-down-86deg",
               "grav-down-172deg", "grav-antipode", "grav-pole", "grav-beside-pole", "zero-record-first")]


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def table(oracle):
    t = {c["name"]: c for c in fc.cases(oracle)}
    assert sorted(t) == sorted(CASE_NAMES)
    return t


def _unit(q):
    return abs(np.linalg.norm(q) - 1.0)


# ---- (a) injected records ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_solve_with_injected_records(capi, table, scene_small, name):
    import torch

    from limo_velo_amd.distributed import HipEngine

    c, ref = table[name], table[name]["run"]
    recs = [torch.from_numpy(fc.pack_record(r)) for r in c["records"]]
    with capi.Context(capi.default_params(estimate_extrinsics=c["ext"], MAX_NUM_ITERS=len(recs) - 1)) as ctx:
        ctx.map_build(scene_small["map_xyz"])
        ctx.scan_set(scene_small["scan_xyz"][:64])   # every launch is the ordinary one; what it reduces is overwritten
        eng = HipEngine(ctx, torch, multi=True)
        assert eng.max_passes == len(recs)
        with eng.stream_ctx():
            eng.begin(c["x0"], c["P"])
            for rec in recs:
                sums = eng.reduce()                    # the search, the fit, the rank's record — and solve_prep
                sums.copy_(rec)                        # on the engine's stream, between the reduction and the solve
                eng.solve()
            x, P, passes = eng.end()
        ctx.set_sums_buffer(None)
    assert passes == ref["passes"]
    ex = np.abs(x - ref["x"]).max()
    eP = np.abs(P - ref["P"]).max() / max(1.0, np.abs(ref["P"]).max())
    print(f"{name}: |x - x_o| {ex:.3e}, |P - P_o| / max(1, max|P_o|) {eP:.3e}")
    assert ex <= TOL_STATE, (name, ex, np.argmax(np.abs(x - ref["x"])))
    assert eP <= 1e-9, (name, eP)
    assert abs(np.linalg.norm(x[23:26]) - 9.809) <= 1e-9
    assert _unit(x[3:7]) <= 1e-12 and _unit(x[7:11]) <= 1e-12


# ---- (b) real scenes that start far off ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("deg,metres", [(2.0, 0.1), (5.0, 0.3), (8.0, 0.3)])
def test_update_from_far_off_on_both_routes(capi, oracle, scene_small, deg, metres, ext):
    sc = scene_small
    off = np.zeros(23)
    off[0:3] = metres * np.array([0.10, -0.07, 0.05]) / np.linalg.norm([0.10, -0.07, 0.05])
    off[3:6] = np.radians(deg) * np.array([0.5, -0.4, 0.8]) / np.linalg.norm([0.5, -0.4, 0.8])
    x_init, P0 = oracle.boxplus(sc["x_true"], off), sc["P0"]
    prm_o = oracle.default_params(estimate_extrinsics=ext)
    with capi.Context(capi.default_params(estimate_extrinsics=ext)) as ctx:
        ctx.set_option("fused_ext", 1)
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        res = {}
        for fused in (True, False):
            ctx.set_fused_pass(fused)
            res[fused] = ctx.update(x_init, P0)
            assert ctx.last_update_fused() == fused
    for fused, (x, P, passes, tr, sums) in res.items():
        route = "one launch" if fused else "three kernels"
        # reached on the device: its own first rotation increment is past the Taylor bound of cos_sinc_sqrt
        assert np.linalg.norm(tr[0][3:6]) > 0.0221, (route, np.linalg.norm(tr[0][3:6]))
        states = [x_init] + [tr[i][23:49].copy() for i in range(passes - 1)]
        worst = 0.0
        for k in range(passes):   # each pass on its own, from the state and with the sums the DEVICE held
            assert sums[k]["n_valid"] > 1500
            xs, dxs, _, _ = oracle.kf_step(states[k], x_init, P0, sums[k], params=prm_o, finalize=False)
            e = max(np.abs(dxs - tr[k][:23]).max(), np.abs(xs - tr[k][23:49]).max())
            worst = max(worst, e)
            assert e <= TOL_STATE, (route, k, e)
        chain = fc.run_chain(oracle, dict(ext=ext, x0=x_init, P=P0, records=sums), max_num_iters=prm_o.max_num_iters)
        eP = np.abs(P - chain["P"]).max() / max(1.0, np.abs(chain["P"]).max())
        print(f"{deg} deg, ext {ext}, {route}: passes {passes}, first increment {np.linalg.norm(tr[0][3:6]):.4f} rad, "
              f"worst per-pass error {worst:.3e}, P {eP:.3e}")
        assert passes == chain["passes"]
        assert eP <= 1e-9, (route, eP)
        assert np.array_equal(x, tr[passes - 1][23:49])
        assert np.linalg.norm(x[:3] - sc["x_true"][:3]) < 5e-3, route


# ---- (c) lv_predict ---------------------------------------------------------------------------------------------------------
TILTED = np.array([3.0, -4.0, -8.387]) * (fc.S2_LEN / np.linalg.norm([3.0, -4.0, -8.387]))
GRAVITY = dict(down=np.array([0.0, 0.0, -fc.S2_LEN]), tilted=TILTED, pole=np.array([-fc.S2_LEN, 0.0, 0.0]), beside=fc.near_pole(1e-9))
# |gyro - bg| dt, gravity, dt.  The half angle (so3_exp) and the angle (A_matrix) run dsincos through all four of its quadrants
PREDICT_STEPS = [(0.004, "down", 0.005), (0.05, "tilted", 0.005), (1.0, "pole", 0.05), (2.0, "beside", 0.05), (3.5, "tilted", 0.05),
                 (4.5, "pole", 0.005), (6.5, "beside", 0.05), (9.0, "tilted", 0.05)]
GYRO_AXIS = np.array([0.4, -0.7, 0.59]) / np.linalg.norm([0.4, -0.7, 0.59])
ACC = np.array([0.3, -0.1, 9.81])
STATE_HALF = np.r_[0:7, 14:17, 23:26]   # pos, rot, vel, grav


def _quadrant(x):
    return int(np.rint(x * 2 / np.pi)) & 3


def test_predict_steps_cover_the_quadrants():
    assert {_quadrant(a / 2) for a, _, _ in PREDICT_STEPS} == {0, 1, 2, 3}
    assert {_quadrant(a) for a, _, _ in PREDICT_STEPS} == {0, 1, 2, 3}
    assert max(a for a, _, _ in PREDICT_STEPS) > 2 * np.pi
    assert GRAVITY["pole"][0] + fc.S2_LEN <= fc.MTK_TOL < GRAVITY["beside"][0] + fc.S2_LEN < 2e-9


def _gyro(x, angle, dt):
    return x[17:20] + (angle / dt) * GYRO_AXIS


@pytest.fixture(scope="module")
def predict_ctx(capi):
    with capi.Context() as ctx:
        yield ctx


@pytest.mark.parametrize("angle,grav,dt", PREDICT_STEPS)
def test_predict_one_step(predict_ctx, oracle, angle, grav, dt):
    ctx = predict_ctx
    x0 = fc.base_state(grav=GRAVITY[grav], offR=fc.OFF_R)   # non-zero biases, a non-identity offset_R_L_I
    P0 = fc.predicted_P(oracle, x0)
    gyro = _gyro(x0, angle, dt)
    ctx.filter_set(x0, P0)
    ctx.predict(dt, fc.Q, ACC, gyro)
    x, P = ctx.filter_get()
    xo, Po = oracle.predict(x0, P0, dt, fc.Q, ACC, gyro)
    # reached on the device: the rotation it returns is the one asked for
    rel = np.asarray(mm.to_float(mm.quat_mul([-t for t in x0[3:6]] + [x0[6]], list(x[3:7]))))
    assert abs(rel[3] - np.cos(angle / 2)) < 1e-9 and abs(np.linalg.norm(rel[:3]) - abs(np.sin(angle / 2))) < 1e-9
    ex, eP = np.abs(x - xo).max(), np.abs(P - Po).max() / max(1.0, np.abs(Po).max())
    ref = mm.predict_state(x0, dt, ACC, gyro)
    half = [ref[i] for i in STATE_HALF]
    e_dev, e_orc = mm.err(x[STATE_HALF], half), mm.err(xo[STATE_HALF], half)
    msg = f"{angle} rad, gravity {grav}, dt {dt}: |x - x_o| {ex:.3e}, P {eP:.3e}; against 50 digits: device {e_dev:.3e}, oracle {e_orc:.3e}"
    print(msg)
    assert ex <= 1e-12, msg
    assert eP <= 1e-12, msg
    # the device's sin / cos / division are a few ulp and FMA-contracted where the oracle's are libm's: 8 x its error
    assert e_dev <= max(8 * e_orc, 1e-13), msg
    assert np.isfinite(P).all() and abs(np.linalg.norm(x[23:26]) - 9.809) <= 1e-9 and _unit(x[3:7]) <= 1e-12


@pytest.mark.parametrize("grav", ["tilted", "pole", "beside"])
def test_queued_and_single_predictions_are_bit_equal(capi, oracle, grav):
    x0 = fc.base_state(grav=GRAVITY[grav], offR=fc.OFF_R)
    P0 = fc.predicted_P(oracle, x0)
    out = {}
    for batch in (1, 0):
        with capi.Context() as ctx:
            ctx.set_option("batch_predict", batch)
            ctx.filter_set(x0, P0)
            for angle, _, dt in PREDICT_STEPS:   # eight steps: one full queue
                ctx.predict(dt, fc.Q, ACC, _gyro(x0, angle, dt))
            out[batch] = ctx.filter_get()
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
