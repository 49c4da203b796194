"""The case table of the filter-algebra tests: states, covariances and injected measurement records that drive the 23-dof
algebra through the branches the scene-based tests never take (pure numpy + the oracle, no GPU).

A case is dict(name, ext, x0[26], P[23,23], records=[rec, ...]); a rec is dict(HTH[12,12], HTh[12], n_valid, sum_h2), the
all-reduced sums of one pass.  One pass of the iterated update is  x <- x [+] dx,  dx = K_h + (K_x - I) J (x [-] x_prop),
with K = (HTH + (P/R)^-1)^-1 — so a record with HTh = HTH [d, 0...] and an HTH that dominates the prior moves the observed
dofs by d, and dofs that P correlates with them follow: P = P0 + sum u u^T, u = 30 e_pos_i + k e_grav_j moves gravity
by k d_i 30 / (P0_ii + 900).

Every case names the branch it is there for as predicates on ORACLE quantities of its own run; cases() asserts them, so
that a change of seeds or magnitudes cannot turn a case into one more small-angle test unnoticed.  The chain of oracle.kf_step
calls that runs a case (run_chain) restates esekf's loop (from -1, `continue` on a pass without matches, the posterior P only
on the pass that ends the update); tests/test_filter_cases_ref.py holds it to oracle.update."""
import numpy as np

import lvamd  # noqa: F401  (registers limo_velo_amd)
from limo_velo_amd import synth

S2_LEN = 98090.0 / 10000.0
MTK_TOL = 1e-11
TAYLOR_N_BOUND = 2.0 ** -13           # cos_sinc_sqrt leaves its Taylor branch at (|v| / 2)^2 >= 2^-13, |v| >= 0.0221 rad
LIMIT = 0.001                          # LIMITS of the default parameters, every dof
ROWS, ROW_SCALE = 400, 10.0            # H^T H ~ 4e4 I: the prior of the extrinsic dofs (R / P = 100) holds back 0.25 % of d
Q = np.diag([1e-4] * 3 + [1e-2] * 3 + [1e-5] * 3 + [1e-4] * 3)   # Localizator::propagate with config/params.yaml:39-42

ROT_AXIS = np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62])
EXT_AXIS = np.array([-0.3, 0.8, 0.52]) / np.linalg.norm([-0.3, 0.8, 0.52])
D_POS = np.array([0.3, -0.2, 0.1])
D_EXT_T = np.array([0.02, 0.01, -0.015])
OFF_R = synth.quat_from_rotvec([0.02, -0.03, 0.05])


def pack_record(rec) -> np.ndarray:
    """The device record of include/limovelo_hip.h: [0..77] upper triangle of H^T H row by row, [78..89] H^T h, [90] n_valid,
    [91] sum h^2, [92..95] zero."""
    out = np.zeros(96)
    out[:78] = np.asarray(rec["HTH"])[np.triu_indices(12)]
    out[78:90] = rec["HTh"]
    out[90] = float(rec["n_valid"])
    out[91] = rec["sum_h2"]
    return out


def make_hth(ext: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    H = np.zeros((ROWS, 12))
    n = 12 if ext else 6
    H[:, :n] = rng.normal(size=(ROWS, n)) * ROW_SCALE
    return H.T @ H


def make_record(ext: int, seed: int, d12) -> dict:
    HTH = make_hth(ext, seed)
    d = np.zeros(12)
    d[: 12 if ext else 6] = np.asarray(d12, float)[: 12 if ext else 6]
    HTh = HTH @ d
    return dict(HTH=HTH, HTh=HTh, n_valid=ROWS, sum_h2=float(d @ HTh))


ZERO_RECORD = dict(HTH=np.zeros((12, 12)), HTh=np.zeros(12), n_valid=0, sum_h2=0.0)


def base_state(grav=(0.0, 0.0, -S2_LEN), offR=(0, 0, 0, 1)) -> np.ndarray:
    return synth.make_state([1.5, -2.0, 0.7], synth.quat_from_rotvec([0.3, -0.2, 0.9]), offR, [0.1, -0.05, 0.2], [0.5, -0.3, 0.1],
                            [0.01, -0.02, 0.005], [0.05, 0.02, -0.03], grav)


def predicted_P(oracle, x0) -> np.ndarray:
    """P0 after five IMU predictions from x0: cross terms between pose, velocity, biases and gravity."""
    x, P = x0.copy(), synth.default_P0()
    for _ in range(5):
        x, P = oracle.predict(x, P, 0.005, Q, [0.1, -0.05, 9.81], [0.01, 0.02, -0.01])
    return P


def grav_moving_P(P, d_pos, want) -> np.ndarray:
    """P + sum u u^T with u_j = 30 e_pos_j + k_j e_grav_j, k_j such that a position step d_pos drags gravity by `want`."""
    P = P.copy()
    for j in range(2):
        k = want[j] * (P[j, j] + 900.0) / (30.0 * d_pos[j])
        u = np.zeros(23)
        u[j], u[21 + j] = 30.0, k
        P += np.outer(u, u)
    return P


def near_pole(eps: float) -> np.ndarray:
    """|g| = 9.809 with g[0] + 9.809 = eps: beside the pole of the S2 chart, on the regular side of its branch."""
    g0 = -S2_LEN + eps
    return np.array([g0, np.sqrt((S2_LEN - g0) * (S2_LEN + g0)), 0.0])


def increment(mag: float, ext: int) -> np.ndarray:
    d = np.zeros(12)
    d[0:3], d[3:6] = D_POS, mag * ROT_AXIS
    if ext:
        d[6:9], d[9:12] = 0.5 * mag * EXT_AXIS, D_EXT_T
    return d


def params_for(oracle, case):
    return oracle.default_params(estimate_extrinsics=case["ext"], max_num_iters=len(case["records"]) - 1)


def run_chain(oracle, case, records=None, P=None, max_num_iters=None):
    """The iterated update of a case on the oracle, one kf_step per record, by esekf's loop rule.  Returns dict(x, P, passes,
    dx [passes, 23], xs [passes, 26] (the state after each pass), conv [passes])."""
    records = case["records"] if records is None else records
    P = case["P"] if P is None else P
    maximum_iter = len(records) - 1 if max_num_iters is None else max_num_iters
    prm = oracle.default_params(estimate_extrinsics=case["ext"], max_num_iters=maximum_iter)
    x, x_prop, t = case["x0"].copy(), case["x0"], 0
    out = dict(x=x, P=np.asarray(P, float).copy(), passes=0, dx=[], xs=[], conv=[])
    for i, rec in zip(range(-1, maximum_iter), records):
        out["passes"] += 1
        if rec["n_valid"] == 0:   # dyn_share.valid = false: `continue`
            out["dx"].append(np.zeros(23)), out["xs"].append(x.copy()), out["conv"].append(False)
            continue
        # the terminal pass is known only after the step: step without P first, then again with it (kf_step has no state)
        xs, dx, conv, _ = oracle.kf_step(x, x_prop, P, rec, params=prm, finalize=False)
        t += int(conv)
        last = t > 1 or i == maximum_iter - 1
        if last:
            xs2, dx2, _, out["P"] = oracle.kf_step(x, x_prop, P, rec, params=prm, finalize=True)
            assert np.array_equal(xs2, xs) and np.array_equal(dx2, dx)
        x = xs
        out["dx"].append(dx), out["xs"].append(x.copy()), out["conv"].append(conv)
        if last:
            break
    out["x"] = x
    out["dx"], out["xs"] = np.array(out["dx"]), np.array(out["xs"])
    return out


def quantities(oracle, case, run):
    """What the branches of the algebra see in a run, per pass: x_before, seg = x_before [-] x_prop (solve_prep's argument to
    A_matrix / Mx), dx (boxplus's), the relative quaternion of the log, the S2 quantities."""
    q = []
    before = case["x0"]
    for k in range(run["passes"]):
        seg = oracle.boxminus(before, case["x0"])
        rel = synth.quat_mul(before[3:7] * [-1, -1, -1, 1], case["x0"][3:7])   # conj(x) x_prop: same |xyz| and w as conj(x_prop) x
        dx = run["dx"][k]
        g, gp = before[23:26], case["x0"][23:26]
        Bu = np.linalg.norm(dx[21:23])   # |Bx d| = |d|: the chart's columns are orthonormal
        q.append(dict(before=before, seg=seg, dx=dx, half2_rot=(np.linalg.norm(dx[3:6]) / 2) ** 2,
                      half2_ext=(np.linalg.norm(dx[6:9]) / 2) ** 2, half2_grav=(Bu / 2) ** 2,
                      log_nv=float(np.linalg.norm(rel[:3])), log_w=float(rel[3]),
                      v_sin=float(np.linalg.norm(np.cross(g, gp))), grav_angle=float(np.arctan2(np.linalg.norm(np.cross(g, gp)), g @ gp)),
                      pole_before=before[23] + S2_LEN, pole_prop=gp[0] + S2_LEN))
        before = run["xs"][k]
    return q


def _rot_case(oracle, mag, ext, offR, with_predicted_P, seed):
    x0 = base_state(offR=offR)
    P = predicted_P(oracle, x0) if with_predicted_P else synth.default_P0()
    d = increment(mag, ext)
    recs = [make_record(ext, seed, d), make_record(ext, seed + 1, 0.3 * d)]
    taylor = (mag / 2) ** 2 < TAYLOR_N_BOUND
    preds = [("pass 1 increment is the one asked for", lambda q, m=mag: abs(np.linalg.norm(q[0]["dx"][3:6]) - m) < 2e-3 * m),
             ("pass 1 exp on the %s side of the Taylor bound" % ("Taylor" if taylor else "sincos"),
              lambda q, t=taylor: (q[0]["half2_rot"] < TAYLOR_N_BOUND) == t),
             ("pass 1 prep: A_matrix and Mx at zero", lambda q: np.linalg.norm(q[0]["seg"]) == 0.0),
             ("pass 2 prep: A_matrix beyond the tolerance", lambda q: np.linalg.norm(q[1]["seg"][3:6]) > MTK_TOL)]
    if mag >= 2.0:
        preds.append(("pass 2 log: atan's argument beyond 1", lambda q: abs(q[1]["log_nv"] / q[1]["log_w"]) > 1.0))
    else:
        preds.append(("pass 2 log: atan's argument within 1", lambda q: abs(q[1]["log_nv"] / q[1]["log_w"]) < 1.0))
    if mag > np.pi:
        preds.append(("pass 2 log: w < 0", lambda q: q[1]["log_w"] < 0.0))
    if ext:
        preds.append(("extrinsic rotation moved by about half", lambda q, m=mag: abs(np.linalg.norm(q[0]["dx"][6:9]) - 0.5 * m) < 0.01 * m))
    return dict(name=f"rot{mag:g}-ext{ext}", ext=ext, x0=x0, P=P, records=recs, predicates=preds)


def _grav_case(oracle, name, ext, grav, want, offR, with_predicted_P, seed, extra):
    x0 = base_state(grav=grav, offR=offR)
    P = grav_moving_P(predicted_P(oracle, x0) if with_predicted_P else synth.default_P0(), D_POS, want)
    d = increment(0.3, ext)
    recs = [make_record(ext, seed, d), make_record(ext, seed + 1, 0.3 * d)]
    wn = float(np.linalg.norm(want))
    preds = [("|g| is 9.809", lambda q: abs(np.linalg.norm(q[0]["before"][23:26]) - S2_LEN) < 1e-12),
             ("gravity moved by what was asked", lambda q, w=wn: abs(q[1]["grav_angle"] - w) < 0.02 * w),
             ("pass 1 S2 boxplus beyond the Taylor bound", lambda q: q[0]["half2_grav"] >= TAYLOR_N_BOUND),
             ("pass 1 S2 boxminus returns at v_sin < tol, Mx at delta = 0", lambda q: q[0]["v_sin"] < MTK_TOL),
             ("pass 2 S2 boxminus past v_sin, Mx with delta", lambda q: q[1]["v_sin"] > MTK_TOL and np.linalg.norm(q[1]["seg"][21:23]) > MTK_TOL)]
    return dict(name=f"{name}-ext{ext}", ext=ext, x0=x0, P=P, records=recs, predicates=preds + extra)


def _antipode_case(oracle, ext, offR, seed):
    """Gravity lands on the antipode of its prediction: the second pass's x [-] x_prop takes the S2 difference's exit for
    theta = pi, v_sin = |g x g_prop| < 1e-11, which wants the first step within 1e-13 rad of pi.  k is tuned on the oracle's own
    step (it is linear in k); what decides the branch is how far INSIDE it the case sits, and the predicate asks for a decade."""
    x0 = base_state(offR=offR)
    d = increment(0.3, ext)
    recs = [make_record(ext, seed, d), make_record(ext, seed + 1, 0.3 * d)]
    k = np.pi * 901.0 / (30.0 * D_POS[0])
    for _ in range(4):
        u = np.zeros(23)
        u[0], u[21] = 30.0, k
        case = dict(name=f"grav-antipode-ext{ext}", ext=ext, x0=x0, P=synth.default_P0() + np.outer(u, u), records=recs)
        k *= np.pi / oracle.kf_step(x0, x0, case["P"], recs[0], params=params_for(oracle, case), finalize=False)[1][21]
    case["predicates"] = [("pass 1 moves gravity by pi", lambda q: abs(q[0]["dx"][21] - np.pi) < 1e-14 and q[0]["dx"][22] == 0.0),
                          ("pass 2 S2 boxminus: v_sin a decade inside the tolerance", lambda q: q[1]["v_sin"] < MTK_TOL / 10),
                          ("... with theta = pi: the literal", lambda q: q[1]["grav_angle"] > 3.14 and np.array_equal(q[1]["seg"][21:23], [3.1415926, 0.0]))]
    return case


_CACHE = {}


def cases(oracle):
    """The table.  Every predicate is asserted on the oracle's run of the case before it is handed out."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = []
    tilted = np.array([3.0, -4.0, -8.387])
    tilted *= S2_LEN / np.linalg.norm(tilted)
    pole = np.array([-S2_LEN, 0.0, 0.0])
    for ext in (0, 1):
        offR = OFF_R if ext else (0, 0, 0, 1)
        for n, mag in enumerate((0.01, 0.0220, 0.0222, 0.3, 2.0, 3.0, 4.0)):
            # a non-identity offset_R_L_I and a predicted P also without extrinsic estimation, in the 0.3 and 3.0 cases
            rich = mag in (0.3, 3.0)
            out.append(_rot_case(oracle, mag, ext, OFF_R if rich else offR, rich, 100 + 10 * n + 50 * ext))
        on_regular = [("regular branch of the chart at x_prop", lambda q: q[0]["pole_prop"] > MTK_TOL)]
        out.append(_grav_case(oracle, "grav-tilted-3deg", ext, tilted, (0.05, -0.02), offR, True, 300 + ext, on_regular))
        out.append(_grav_case(oracle, "grav-down-86deg", ext, (0, 0, -S2_LEN), (1.2, 0.9), offR, False, 310 + ext, on_regular))
        out.append(_grav_case(oracle, "grav-down-172deg", ext, (0, 0, -S2_LEN), (3.0, 0.0), offR, False, 320 + ext,
                              on_regular + [("beyond 170 degrees", lambda q: q[1]["grav_angle"] > np.radians(170))]))
        out.append(_grav_case(oracle, "grav-pole", ext, pole, (0.4, -0.3), OFF_R, True, 330 + ext,
                              [("pole branch of the chart at x_prop", lambda q: q[0]["pole_prop"] <= MTK_TOL),
                               ("regular branch after the move", lambda q: q[1]["pole_before"] > MTK_TOL)]))
        out.append(_grav_case(oracle, "grav-beside-pole", ext, near_pole(1e-9), (0.4, -0.3), offR, False, 340 + ext,
                              [("regular branch, 1e-9 from its bound", lambda q: MTK_TOL < q[0]["pole_prop"] < 2e-9)]))
        out.append(_antipode_case(oracle, ext, offR, 350 + ext))
        # a pass without matches first: solve_kernel's `continue`
        d = increment(0.3, ext)
        out.append(dict(name=f"zero-record-first-ext{ext}", ext=ext, x0=base_state(offR=offR), P=synth.default_P0(),
                        records=[ZERO_RECORD, make_record(ext, 400 + ext, d), make_record(ext, 410 + ext, 0.3 * d)],
                        predicates=[("pass 1 leaves the state alone", lambda q: not q[0]["dx"].any()),
                                    ("pass 2 steps from x_prop", lambda q: np.linalg.norm(q[1]["seg"]) == 0.0 and q[1]["half2_rot"] >= TAYLOR_N_BOUND)]))
    for c in out:
        run = run_chain(oracle, c)
        q = quantities(oracle, c, run)
        assert run["passes"] == len(c["records"]), c["name"]
        # the update ends by count on the last record: no pass may count as converged before
        assert not any(run["conv"]), (c["name"], run["conv"])
        assert all(np.abs(dx).max() > LIMIT for dx, r in zip(run["dx"], c["records"]) if r["n_valid"]), c["name"]
        for what, pred in c["predicates"]:
            assert pred(q), f"{c['name']}: {what}"
        c["run"], c["q"] = run, q
    assert len({c["name"] for c in out}) == len(out)
    _CACHE["cases"] = out
    return out
