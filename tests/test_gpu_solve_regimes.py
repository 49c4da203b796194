"""The 23-dof solve of an update pass on the device, in its three copies, outside the one regime the rest of the suite runs it in
(LiDAR_noise = LIMITS = 0.001, default_P0 or five predictions of it, a full-rank H^T H that dominates the prior, an update that
ends by pass count).  The cases, their predicates and the bound are those of tests/solve_regimes.py; tests/test_solve_regimes_ref.py
holds the references to each other on the CPU.

(a) solve_kernel<6 | 12> + solve_prep (lv_solve.hip, lv_solve_dev.hpp) with injected records, as test_gpu_filter_branches.py
    injects them: x, P and the pass count against the 50-digit chain.
(b) the closing part of pass_kernel (lv_pass_dev.hpp) and the three-kernel route from a real scene, and lv_correct, at
    LiDAR_noise {1e-6, 1} x P0 {default, x 1e4} and on a degenerate scan (planes that face one axis only); pass by pass against
    the 50-digit step fed with the device's own sums and the device's state before the pass; then with per-dof LIMITS.
(c) the batched copy (lv_batch.hip): one pass per hypothesis against the 50-digit step fed with the returned sums.  (That every
    hypothesis is lv_update at other LiDAR_noise and LIMITS is asserted by tests/test_gpu_update_batch.py::test_parameters.)

The adjudicator is the 50-digit statement, not the oracle: in the degenerate cases a correct f64 solve is itself 1e-10 .. 1e-2
from the truth.  With e_o and e_f the errors of oracle.kf_step (upstream's two 23 x 23 inverses) and of the device's stated block
form in numpy f64, the device is held, for x and for P / max(1, max|P_mp|), to
    max(8 max(e_o, e_f),  1e-12 max(1, |dx|_inf))
— 8 is what test_predict_one_step gives the device over the oracle's error, 1e-12 is TOL_X of test_gpu_pass_kernel.py — and to
the pass count exactly.

Measured on an MI355X (gfx950), this suite's run; x and P are the device's errors against 50 digits:

(a) injected records          passes  device x   device P   e_o        e_f        bound
    R1e-06-ext0                   2    2.22e-16   2.75e-16   3.82e-16   3.82e-16   1.00e-12
    R1-ext0                       2    4.44e-16   3.21e-16   7.66e-16   3.82e-16   1.00e-12
    R100-ext0                     2    2.22e-16   2.40e-16   5.06e-16   3.80e-16   1.00e-12
    weak-scan-ext0                2    5.55e-17   7.61e-16   7.64e-16   7.64e-16   1.00e-12
    prior-wide-ext0               2    1.11e-16   2.79e-16   3.82e-16   3.82e-16   1.00e-12
    prior-tight-ext0              2    2.22e-16   4.00e-22   3.64e-16   3.64e-16   1.00e-12
    prior-ill-ext0                2    4.26e-14   1.63e-10   1.60e-10   1.54e-10   1.28e-09
    corridor-default-ext0         2    3.82e-11   2.08e-10   8.50e-11   1.71e-10   1.37e-09
    corridor-wide-R1e-6-ext0      2    7.88e-05   4.48e-04   1.89e-03   4.45e-04   1.52e-02
    rows1-ext0                    2    1.92e-12   7.44e-12   1.29e-11   8.05e-12   1.03e-10
    rows3-ext0                    2    8.26e-11   4.06e-11   1.48e-10   1.52e-10   1.22e-09
    rows6-ext0                    2    8.44e-15   1.63e-15   2.27e-14   9.08e-15   1.00e-12
    zero-variance-ext0            2    2.22e-16   4.08e-16   inf        3.82e-16   1.00e-12
    limits-uniform-ext0           2    2.22e-16   2.77e-16   8.05e-16   3.82e-16   1.00e-12
    limits-tight-dof0-ext0        4    4.44e-16   2.54e-16   4.58e-16   3.82e-16   1.00e-12
    limits-tight-dof5-ext0        4    4.44e-16   2.54e-16   4.58e-16   3.82e-16   1.00e-12
    limits-tight-dof8-ext0        4    4.44e-16   7.58e-16   7.58e-16   1.20e-15   1.00e-12
    limits-tight-dof12-ext0       4    4.44e-16   2.54e-16   4.58e-16   3.82e-16   1.00e-12
    limits-tight-dof22-ext0       4    4.44e-16   2.54e-16   4.58e-16   3.82e-16   1.00e-12
    limits-pass1-below-ext0       3    4.44e-16   1.99e-16   3.82e-16   3.82e-16   1.00e-12
    limits-pass1-above-ext0       2    2.22e-16   2.77e-16   8.05e-16   3.82e-16   1.00e-12
    limits-pass2-below-ext0       4    4.44e-16   2.54e-16   4.58e-16   3.82e-16   1.00e-12
    limits-pass2-above-ext0       3    4.44e-16   1.99e-16   3.82e-16   3.82e-16   1.00e-12
    limits-converged-apart-ext0    4    1.78e-15   4.07e-16   1.78e-15   1.78e-15   1.00e-12
    R1e-06-ext1                   2    2.22e-16   3.23e-16   3.82e-16   5.51e-16   1.00e-12
    R1-ext1                       2    4.44e-16   3.66e-16   7.82e-16   3.91e-16   1.00e-12
    R100-ext1                     2    2.22e-16   5.20e-16   6.30e-16   3.92e-16   1.00e-12
    weak-scan-ext1                2    1.11e-16   3.15e-16   1.73e-16   2.78e-16   1.00e-12
    prior-wide-ext1               2    2.22e-16   1.80e-16   7.33e-16   5.51e-16   1.00e-12
    prior-tight-ext1              2    2.22e-16   4.10e-22   3.94e-16   3.78e-16   1.00e-12
    prior-ill-ext1                2    5.68e-14   3.38e-10   2.39e-10   1.64e-10   1.91e-09
    corridor-default-ext1         2    3.83e-11   3.73e-10   3.26e-10   1.14e-10   2.61e-09
    corridor-wide-R1e-6-ext1      2    7.43e-05   6.64e-04   1.16e-02   2.83e-03   9.27e-02
    rows1-ext1                    2    1.60e-11   5.28e-11   1.31e-10   8.18e-11   1.04e-09
    rows3-ext1                    2    2.55e-11   3.88e-11   5.94e-11   8.87e-11   7.10e-10
    rows6-ext1                    2    6.75e-14   4.92e-14   1.17e-13   9.07e-14   1.00e-12
    limits-uniform-ext1           2    1.11e-16   6.04e-16   8.26e-16   3.82e-16   1.00e-12
    limits-tight-dof0-ext1        4    4.44e-16   3.50e-16   4.31e-16   3.82e-16   1.00e-12
    limits-tight-dof5-ext1        4    4.44e-16   3.50e-16   4.31e-16   3.82e-16   1.00e-12
    limits-tight-dof11-ext1       4    4.44e-16   3.50e-16   4.31e-16   3.82e-16   1.00e-12
    limits-tight-dof12-ext1       4    4.44e-16   3.50e-16   4.31e-16   3.82e-16   1.00e-12
    limits-tight-dof22-ext1       4    4.44e-16   3.50e-16   4.31e-16   3.82e-16   1.00e-12
    limits-pass1-below-ext1       3    4.44e-16   2.27e-16   6.88e-16   4.39e-16   1.00e-12
    limits-pass1-above-ext1       2    1.11e-16   6.04e-16   8.26e-16   3.82e-16   1.00e-12
    limits-pass2-below-ext1       4    4.44e-16   3.50e-16   4.31e-16   3.82e-16   1.00e-12
    limits-pass2-above-ext1       3    4.44e-16   2.27e-16   6.88e-16   4.39e-16   1.00e-12
    limits-converged-apart-ext1    4    1.78e-15   4.34e-16   1.78e-15   1.78e-15   1.00e-12
(b) real scene, worst pass    passes  device     e_o        e_f        bound
    scene-R1e-06-P1, one launch            4  7.11e-16   8.19e-15   1.13e-14   1.00e-12
    scene-R1e-06-P1, three kernels         4  9.16e-16   1.14e-14   9.55e-15   1.00e-12
    scene-R1-P1, one launch                4  1.04e-15   1.10e-14   1.00e-14   1.00e-12
    scene-R1-P1, three kernels             4  4.19e-16   1.60e-14   1.12e-14   1.00e-12
    scene-R1e-06-P10000, one launch        4  6.84e-16   9.08e-15   5.65e-15   1.00e-12
    scene-R1e-06-P10000, three kernels     4  6.81e-16   1.11e-14   6.97e-15   1.00e-12
    scene-R1-P10000, one launch            4  9.35e-16   4.80e-15   1.45e-14   1.00e-12
    scene-R1-P10000, three kernels         4  9.35e-16   7.19e-15   2.58e-14   1.00e-12
    scene-walls, one launch                4  2.91e-15   1.18e-13   8.97e-14   1.00e-12
    scene-walls, three kernels             4  1.14e-14   6.05e-14   6.44e-14   1.00e-12
(c) lv_update_batch, one pass, worst of 12 hypotheses: device x 4.44e-16, P 1.38e-15, e_o 2.57e-14, e_f 1.55e-14, bound 1.00e-12
"""
import numpy as np
import pytest

import filter_cases as fc
import solve_regimes as sr

pytestmark = pytest.mark.gpu

TOL_X, TOL_P_REL = 1e-12, 1e-9   # tests/test_gpu_pass_kernel.py: what separates the two routes
DEGENERATE = float(np.sin(np.radians(5.0)) ** 2)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def table(oracle):
    t = {c["name"]: c for c in sr.cases(oracle)}
    assert list(t) == sr.NAMES
    return t


def _unit(q):
    return abs(np.linalg.norm(q) - 1.0)


def _sane(x, P):
    assert np.isfinite(x).all() and np.isfinite(P).all()
    assert abs(np.linalg.norm(x[23:26]) - 9.809) <= 1e-9
    assert _unit(x[3:7]) <= 1e-12 and _unit(x[7:11]) <= 1e-12


def _params(capi, c):
    return capi.default_params(estimate_extrinsics=c["ext"], MAX_NUM_ITERS=c["max_num_iters"], LiDAR_noise=c["R"], LIMITS=list(c["limits"]))


# ---- (a) injected records ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.NAMES)
def test_solve_with_injected_records(capi, table, scene_small, name):
    import torch

    from limo_velo_amd.distributed import HipEngine

    c, ref = table[name], table[name]["mp"]
    recs = [torch.from_numpy(fc.pack_record(r)) for r in c["records"]]
    with capi.Context(_params(capi, c)) as ctx:
        ctx.map_build(scene_small["map_xyz"])
        ctx.scan_set(scene_small["scan_xyz"][:64])   # every launch is the ordinary one; what it reduces is overwritten
        eng = HipEngine(ctx, torch, multi=True)
        assert eng.max_passes == len(recs)
        with eng.stream_ctx():
            eng.begin(c["x0"], c["P"])
            for rec in recs:                           # (passes after the one that ends the update return at once)
                sums = eng.reduce()
                sums.copy_(rec)
                eng.solve()
            x, P, passes = eng.end()
        ctx.set_sums_buffer(None)
    with np.errstate(invalid="ignore"):
        ex = np.abs(x - ref["x"]).max()
        eP = np.abs(P - ref["P"]).max() / max(1.0, np.abs(ref["P"]).max())
    print(f"{name}: passes {passes} ({ref['passes']}), x {ex:.2e}, P {eP:.2e}, e_o {c['e_o']:.2e}, e_f {c['e_f']:.2e}, bound {c['bound']:.2e}")
    assert passes == ref["passes"], (name, passes, ref["passes"])
    _sane(x, P)
    assert ex <= c["bound"], (name, ex, c["bound"], int(np.argmax(np.abs(x - ref["x"]))))
    assert eP <= c["bound"], (name, eP, c["bound"])
    if c["keep"] is not None:   # dofs without variance: untouched, and P keeps its zeros
        out = [i for i in range(23) if i not in c["keep"]]
        assert np.array_equal(x[7:14], c["x0"][7:14]) and not P[out].any() and not P[:, out].any()


# ---- (b) the other copies, from a real scene ---------------------------------------------------------------------------------
def _scene_case(name, sc, P0, R, limits=None, scan=None):
    return dict(name=name, ext=0, x0=sc["x_init"], P=P0, R=R, limits=np.full(23, fc.LIMIT) if limits is None else np.asarray(limits, float),
                max_num_iters=3, keep=None, scan=sc["scan_xyz"] if scan is None else scan, records=[])


def _run_routes(capi, sc, case):
    """lv_update on both routes and lv_correct on both, from the case's state: {(entry, fused): (x, P, passes, trace, sums)}."""
    out = {}
    with capi.Context(_params(capi, case)) as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(case["scan"])
        for fused in (True, False):
            ctx.set_fused_pass(fused)
            out["update", fused] = ctx.update(case["x0"], case["P"])
            assert ctx.last_update_fused() == fused
            ctx.filter_set(case["x0"], case["P"])
            p = ctx.correct()
            assert ctx.last_update_fused() == fused
            out["correct", fused] = ctx.filter_get() + (p,)
        ctx.set_fused_pass(True)
    return out


def _check_passes(oracle, case, res):
    """Every pass of an lv_update on its own, from the state and with the sums the DEVICE held: the device's dx_ and new state (and
    the posterior P on the pass that ends the update) against the 50-digit step, beside the two f64 yardsticks.  Returns the
    largest bound applied."""
    x, P, passes, tr, sums = res
    mp, orc, blk = sr.mp_step(case), sr.oracle_step(oracle, case), sr.block_step(oracle, case)
    states = [case["x0"]] + [tr[i][23:49].copy() for i in range(passes - 1)]
    worst_bound = 0.0
    for k in range(passes):
        assert sums[k]["n_valid"] > 0
        last = k == passes - 1
        ref = mp(states[k], sums[k])
        e_o, e_f = sr.step_error(orc(states[k], sums[k]), ref, last), sr.step_error(blk(states[k], sums[k]), ref, last)
        assert np.isfinite(e_o) and np.isfinite(e_f)
        e_d = sr.step_error(dict(dx=tr[k][:23], x=tr[k][23:49], P=P), ref, last)
        b = sr.bound(e_o, e_f, float(np.abs(ref["dx"]).max()))
        worst_bound = max(worst_bound, b)
        print(f"  pass {k + 1}: n_valid {sums[k]['n_valid']}, device {e_d:.2e}, e_o {e_o:.2e}, e_f {e_f:.2e}, bound {b:.2e}")
        assert e_d <= b, (case["name"], k, e_d, b)
    assert np.array_equal(x, tr[passes - 1][23:49])
    chain = sr.chain(orc, case, records=sums)
    assert passes == chain["passes"], (case["name"], passes, chain["passes"])
    _sane(x, P)
    return worst_bound


def _routes_agree(res, tol_x, tol_P):
    (xf, Pf, pf, _, _), (xt, Pt, pt, _, _) = res["update", True], res["update", False]
    assert pf == pt == res["correct", True][2] == res["correct", False][2]
    for x, P in ((xt, Pt), res["correct", True][:2], res["correct", False][:2]):
        _sane(x, P)
        assert np.abs(x - xf).max() <= tol_x, np.abs(x - xf).max()
        if tol_P is None:   # the existing rule of the routes: relative entry by entry, small entries are differences of larger ones
            np.testing.assert_allclose(P, Pf, rtol=TOL_P_REL, atol=1e-13 * max(1.0, np.abs(Pf).max()))
        else:
            assert np.abs(P - Pf).max() <= tol_P * max(1.0, np.abs(Pf).max())


@pytest.mark.parametrize("R", [1e-6, 1.0])
@pytest.mark.parametrize("p_scale", [1.0, 1e4])
def test_routes_at_other_noise_and_prior(capi, oracle, scene_small, R, p_scale):
    sc = scene_small
    case = _scene_case(f"scene-R{R:g}-P{p_scale:g}", sc, sc["P0"] * p_scale, R)
    res = _run_routes(capi, sc, case)
    for fused in (True, False):
        print(f"{case['name']}, {'one launch' if fused else 'three kernels'}: passes {res['update', fused][2]}")
        _check_passes(oracle, case, res["update", fused])
    _routes_agree(res, TOL_X, None)


@pytest.fixture(scope="module")
def wall_scan(oracle, scene_small):
    """Up to 200 scan points whose plane (the oracle's fit at x_init) has its normal within 5 degrees of the x axis: a scan that
    sees walls of one orientation only.  A plane family holds one translation and two rotations, and a cone of 5 degrees leaves
    up to sin^2(5 deg) = 7.6e-3 of a row's weight on the other directions.  Predicate: at most 3 eigenvalues of the pose block of
    the oracle's H^T H are above sin^2(5 deg) of the largest.  (Measured: 1, 0.20, 6.6e-3, 1.6e-3, 2.0e-5, 1.7e-5 of the largest;
    "above 1e-6 of the largest" is out of reach of planes fitted to points with 1 cm of noise, whatever the cone.)"""
    sc = scene_small
    tree = oracle.KdTree(sc["map_xyz"])
    det = oracle.iterate(sc["x_init"], sc["map_xyz"], sc["scan_xyz"], tree=tree, details=True)
    pick = np.flatnonzero((det["valid"] != 0) & (np.abs(det["abcd"][:, 0]) > np.cos(np.radians(5.0))))[:200]
    assert len(pick) >= 50, len(pick)
    scan = np.ascontiguousarray(sc["scan_xyz"][pick])
    s = oracle.iterate(sc["x_init"], sc["map_xyz"], scan, tree=tree, details=False)
    eig = np.sort(np.linalg.eigvalsh(s["HTH"][:6, :6]))[::-1]
    assert s["n_valid"] >= 50 and (eig > DEGENERATE * eig[0]).sum() <= 3 and eig[5] < 1e-4 * eig[0], (s["n_valid"], eig)
    return scan


def test_routes_on_a_degenerate_scan(capi, oracle, scene_small, wall_scan):
    sc = scene_small
    case = _scene_case("scene-walls", sc, sc["P0"], 1e-3, scan=wall_scan)
    res = _run_routes(capi, sc, case)
    b = 0.0
    for fused in (True, False):
        print(f"{case['name']}, {'one launch' if fused else 'three kernels'}: passes {res['update', fused][2]}")
        b = max(b, _check_passes(oracle, case, res["update", fused]))
        eig = np.sort(np.linalg.eigvalsh(res["update", fused][4][0]["HTH"][:6, :6]))[::-1]
        assert (eig > DEGENERATE * eig[0]).sum() <= 3, eig      # what the DEVICE reduced is degenerate too
    _routes_agree(res, b, b)


def test_routes_with_per_dof_limits(capi, oracle, scene_small):
    """LIMITS 1.0 everywhere against 1.0 but 1e-12 on dof 22 (the last gravity dof, which the prior below ties to the position):
    the pass counts are the oracle chain's on both routes and under lv_correct, and the two settings end differently."""
    sc = scene_small
    u = np.zeros(23)
    u[0], u[22] = 1.0, 1e-3
    P0 = sc["P0"] + np.outer(u, u)
    tight = np.ones(23)
    tight[22] = 1e-12
    passes = {}
    for name, limits in (("uniform", np.ones(23)), ("tight22", tight)):
        case = _scene_case(f"scene-limits-{name}", sc, P0, 1e-3, limits=limits)
        res = _run_routes(capi, sc, case)
        orc = sr.oracle_step(oracle, case)
        for fused in (True, False):
            x, P, p, tr, sums = res["update", fused]
            chain = sr.chain(orc, case, records=sums)
            print(f"{case['name']}, {'one launch' if fused else 'three kernels'}: passes {p}, oracle chain {chain['passes']}, |dx_22| {np.abs(tr[:, 22])}")
            assert p == chain["passes"] == res["correct", fused][2], (name, fused, p, chain["passes"], res["correct", fused][2])
            # dof 22 moves two decades beyond the tight limit on the two passes that decide, every other dof stays below 1.0
            assert np.all(np.abs(chain["dx"][:2, 22]) > 1e-10) and np.abs(chain["dx"]).max() < 1.0
            assert np.abs(x - chain["x"]).max() <= 1e-9
        _routes_agree(res, TOL_X, None)
        passes[name] = res["update", True][2]
    assert passes == dict(uniform=2, tight22=4), passes


# ---- (c) the batched copy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1e-3, 1.0])
def test_batch_single_pass_against_50_digits(capi, oracle, scene_small, R):
    from limo_velo_amd import synth

    sc = scene_small
    rng = np.random.default_rng(11)
    xs = [sc["x_init"], sc["x_true"]]
    far = np.array(sc["x_init"])
    far[:3] += [5000.0, 5000.0, 0.0]
    xs.append(far)                                      # outside the map: a pass without matches
    for _ in range(4):
        x = np.array(sc["x_init"])
        x[3:7] = synth.quat_mul(synth.quat_from_rpy(0.0, 0.0, np.radians(rng.uniform(-10, 10))), x[3:7])
        x[:2] += rng.uniform(-0.5, 0.5, 2)
        xs.append(x)
    xs = np.array(xs)
    P0 = fc.predicted_P(oracle, sc["x_init"])
    with capi.Context(capi.default_params(MAX_NUM_ITERS=0, LiDAR_noise=R)) as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        bx, bP, bp, bl = ctx.update_batch(xs, P0, want_P=True)
    for i, x0 in enumerate(xs):
        assert bp[i] == 1
        if bl[i]["n_valid"] == 0:
            assert i == 2 and np.array_equal(bx[i], x0) and np.array_equal(bP[i], P0)
            continue
        case = dict(name=f"batch-R{R:g}-{i}", ext=0, x0=x0, P=P0, R=R, limits=np.full(23, fc.LIMIT), max_num_iters=0, keep=None)
        ref = sr.mp_step(case)(x0, bl[i])
        e_o = sr.step_error(sr.oracle_step(oracle, case)(x0, bl[i]), ref, True)
        e_f = sr.step_error(sr.block_step(oracle, case)(x0, bl[i]), ref, True)
        b = sr.bound(e_o, e_f, float(np.abs(ref["dx"]).max()))
        ex = np.abs(bx[i] - ref["x"]).max()
        eP = np.abs(bP[i] - ref["P"]).max() / max(1.0, np.abs(ref["P"]).max())
        print(f"hypothesis {i}: n_valid {bl[i]['n_valid']}, x {ex:.2e}, P {eP:.2e}, e_o {e_o:.2e}, e_f {e_f:.2e}, bound {b:.2e}")
        _sane(bx[i], bP[i])
        assert ex <= b and eP <= b, (i, ex, eP, b)
    assert bl[2]["n_valid"] == 0 and sum(d["n_valid"] > 0 for d in bl) == len(xs) - 1


def test_batch_with_per_dof_limits(capi, oracle, scene_small):
    """The batched copy's LIMITS test, dof by dof: with the prior of test_routes_with_per_dof_limits (position tied to dof 22) every
    hypothesis ends on the pass lv_update and the oracle chain end on, after 2 passes under uniform limits of 1.0 and after 4 with
    1e-12 on dof 22.  (Under the diagonal default_P0 dof 22 does not move at all, and a limit on it decides nothing.)"""
    sc = scene_small
    u = np.zeros(23)
    u[0], u[22] = 1.0, 1e-3
    P0 = sc["P0"] + np.outer(u, u)
    xs = np.array([sc["x_init"], sc["x_true"], oracle.boxplus(sc["x_init"], np.r_[0.05, -0.08, 0.02, 0.0, 0.0, 0.01, np.zeros(17)])])
    tight = np.ones(23)
    tight[22] = 1e-12
    passes = {}
    for name, limits in (("uniform", np.ones(23)), ("tight22", tight)):
        case = _scene_case(f"batch-limits-{name}", sc, P0, 1e-3, limits=limits)
        with capi.Context(_params(capi, case)) as ctx:
            ctx.map_build(sc["map_xyz"])
            ctx.scan_set(sc["scan_xyz"])
            bx, bP, bp, _ = ctx.update_batch(xs, P0, want_P=True)
            ctx.set_fused_pass(False)
            singles = [ctx.update(x, P0) for x in xs]
        for i, (x, P, p, tr, sums) in enumerate(singles):
            chain = sr.chain(sr.oracle_step(oracle, dict(case, x0=xs[i])), dict(case, x0=xs[i]), records=sums)
            print(f"{case['name']}, hypothesis {i}: batch {bp[i]}, lv_update {p}, oracle chain {chain['passes']}, |dx_22| {np.abs(tr[:, 22])}")
            assert bp[i] == p == chain["passes"], (name, i, bp[i], p, chain["passes"])
            assert np.all(np.abs(chain["dx"][:2, 22]) > 1e-10) and np.abs(chain["dx"]).max() < 1.0
            assert np.abs(bx[i] - x).max() <= TOL_X
            np.testing.assert_allclose(bP[i], P, rtol=TOL_P_REL, atol=1e-13)
        passes[name] = list(bp)
    assert passes == dict(uniform=[2, 2, 2], tight22=[4, 4, 4]), passes
