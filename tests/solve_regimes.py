"""The case table of the solve-regime tests: the 23-dof solve of one update pass outside the one regime every other test runs
it in (LiDAR_noise 0.001, LIMITS 0.001 on every dof, default_P0 or five predictions of it, a full-rank H^T H ~ 4e4 I, an
update that ends by pass count).  Pure numpy, the oracle and the 50-digit statement of tests/manifold_mp.py; no GPU.

A case is dict(name, ext, x0[26], P[23,23], records, R, limits[23], max_num_iters, keep) with records as in
tests/filter_cases.py; keep is None, or the dofs that have variance (the zero-variance case, whose reference is
manifold_mp.kf_step_reduced).  cases() hands out each case with three runs of its update by esekf's loop rule (chain()):
    c["mp"]     the 50-digit chain  — the adjudicator,
    c["oracle"] oracle.kf_step      — upstream's form, two general 23 x 23 inverses,
    c["block"]  block_form_step     — the device's STATED form (header of lv_solve.hip) in plain numpy f64 with np.linalg.inv:
                                      a second f64 yardstick, not the code under test,
and c["e_o"], c["e_f"], the errors of the two f64 chains against the 50-digit one (max over dx, x of every pass and the
posterior P / max(1, max|P_mp|)), and c["dx_inf"], the largest increment of the 50-digit chain.

Every case carries predicates on CPU quantities and cases() asserts them, so that a change of seed cannot turn a case into one
more default-regime test; and every case is ADMITTED only if both f64 errors are finite and
    e_f <= 8 e_o   or   e_f <= 1e-13 max(1, |dx|_inf),
i.e. the bound the device is held to (bound()) is one that a correct f64 implementation of the device's own form meets.  A
case that does not meet it gets another seed, not a wider bound.  (The zero-variance case has no e_o: the oracle inverts
P / R, which is singular there.  Its bound comes from e_f alone.)"""
import numpy as np

import filter_cases as fc
import manifold_mp as mm
from limo_velo_amd import synth

S2_LEN, MTK_TOL = fc.S2_LEN, fc.MTK_TOL
LIMIT = fc.LIMIT
FLOOR = 1e-12            # TOL_X of tests/test_gpu_pass_kernel.py
DEVICE_FACTOR = 8.0      # what test_predict_one_step gives the device over the oracle's error (few-ulp ddiv / dsincos, FMA contraction)


# ---- the device's stated form in numpy f64 ---------------------------------------------------------------------------------
def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _A_matrix(v):
    n2 = float(v @ v)
    n = np.sqrt(n2)
    if n < MTK_TOL:
        return np.eye(3)
    H = _hat(v)
    return np.eye(3) + (1 - np.cos(n)) / n2 * H + (1 - np.sin(n) / n) / n2 * (H @ H)


def _s2_Bx(g):
    if g[0] + S2_LEN > MTK_TOL:
        d = S2_LEN + g[0]
        return np.array([[-g[1], -g[2]], [S2_LEN - g[1] * g[1] / d, -g[2] * g[1] / d], [-g[2] * g[1] / d, S2_LEN - g[2] * g[2] / d]]) / S2_LEN
    return np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0]])


def _s2_projection(g, g_prop, delta):
    Nx = _s2_Bx(g).T @ _hat(g) / S2_LEN / S2_LEN
    Bx, H = _s2_Bx(g_prop), _hat(g_prop)
    T = -H if np.linalg.norm(delta) < MTK_TOL else -H @ _A_matrix(Bx @ delta).T
    return Nx @ (T @ Bx)


def projection(seg, g, g_prop):
    J = np.eye(23)
    J[3:6, 3:6] = _A_matrix(seg[3:6]).T
    J[6:9, 6:9] = _A_matrix(seg[6:9]).T
    J[21:23, 21:23] = _s2_projection(g, g_prop, seg[21:23])
    return J


def block_form_step(oracle, x, x_prop, P, rec, R, limits, ext, finalize=True):
    """One pass in the form lv_solve.hip states, with w the 6 (12 with extrinsic estimation) dofs H^T H lives in and b the rest:
        A1 = Pr_ww^-1,  X_top = (A1 + HTH_ww)^-1,  X_bot = Pr_bw A1 X_top,  K_x = X HTH,  dx_ = X HTh + K_x dx_new - dx_new,
    Pr = J P J^T / R, and the oracle's finalize.  [+] and [-] are the oracle's.  Returns (x, dx_, conv, P or None)."""
    x, x_prop = np.asarray(x, float), np.asarray(x_prop, float)
    nw = 12 if ext else 6
    HTH, HTh = np.asarray(rec["HTH"], float)[:nw, :nw], np.asarray(rec["HTh"], float)[:nw]
    dx = oracle.boxminus(x, x_prop)
    J = projection(dx, x[23:26], x_prop[23:26])
    dx_new = J @ dx
    P_ = J @ np.asarray(P, float).reshape(23, 23) @ J.T
    Pr = P_ / R
    A1 = np.linalg.inv(Pr[:nw, :nw])
    X_top = np.linalg.inv(A1 + HTH)
    X = np.vstack([X_top, Pr[nw:, :nw] @ A1 @ X_top])
    K_x = X @ HTH
    dxo = X @ HTh + K_x @ dx_new[:nw] - dx_new
    x_new = oracle.boxplus(x, dxo)
    conv = bool(np.all(np.abs(dxo) <= np.asarray(limits, float)))
    P_out = None
    if finalize:
        J2 = projection(dxo, x_new[23:26], x_prop[23:26])
        P_out = J2 @ P_ @ J2.T - (J2 @ K_x) @ (P_ @ J2.T)[:nw, :]
    return x_new, dxo, conv, P_out


# ---- the three steps and the loop rule ----------------------------------------------------------------------------------------
def oracle_params(oracle, case):
    return oracle.default_params(estimate_extrinsics=case["ext"], max_num_iters=case["max_num_iters"], lidar_noise=case["R"],
                                 limits=case["limits"])


def oracle_step(oracle, case):
    prm = oracle_params(oracle, case)

    def step(x, rec, P=None):
        with np.errstate(all="ignore"):
            xs, dx, conv, Pp = oracle.kf_step(x, case["x0"], case["P"] if P is None else P, rec, params=prm, finalize=True)
        return dict(x=xs, dx=dx, conv=conv, P=Pp)
    return step


def block_step(oracle, case):
    def step(x, rec, P=None):
        xs, dx, conv, Pp = block_form_step(oracle, x, case["x0"], case["P"] if P is None else P, rec, case["R"], case["limits"], case["ext"])
        return dict(x=xs, dx=dx, conv=conv, P=Pp)
    return step


_MP_CACHE = {}


def mp_step(case):
    """The 50-digit step of a case, cached by its inputs (a 23 x 23 mp inverse takes a fraction of a second)."""
    def step(x, rec, P=None):
        Pm = case["P"] if P is None else P
        key = (case["name"], np.asarray(x, float).tobytes(), fc.pack_record(rec).tobytes(), np.asarray(Pm, float).tobytes())
        if key not in _MP_CACHE:
            if case["keep"] is None:
                _MP_CACHE[key] = mm.kf_step(x, case["x0"], Pm, rec, case["R"], case["limits"], True)
            else:
                _MP_CACHE[key] = mm.kf_step_reduced(x, case["x0"], Pm, rec, case["R"], case["limits"], True, case["keep"])
        return _MP_CACHE[key]
    return step


def chain(step, case, records=None):
    """The iterated update by esekf's loop rule (filter_cases.run_chain with any step): from -1, `continue` on a pass without
    matches, the end on the second converged pass or on pass MAX_NUM_ITERS + 1, the posterior P of the pass that ends it.  Every
    pass starts from the DOUBLES the pass before returned, as on the device.  Returns dict(x, P, passes, dx, xs, conv, steps)."""
    records = case["records"] if records is None else records
    maximum_iter = case["max_num_iters"]
    x, t = np.array(case["x0"], float), 0
    out = dict(P=np.array(case["P"], float), passes=0, dx=[], xs=[], conv=[], steps=[])
    for i, rec in zip(range(-1, maximum_iter), records):
        out["passes"] += 1
        if rec["n_valid"] == 0:
            out["dx"].append(np.zeros(23)), out["xs"].append(x.copy()), out["conv"].append(False), out["steps"].append(None)
            continue
        r = step(x, rec)
        t += int(r["conv"])
        x = np.array(r["x"], float)
        out["dx"].append(np.array(r["dx"], float)), out["xs"].append(x.copy()), out["conv"].append(bool(r["conv"])), out["steps"].append(r)
        if t > 1 or i == maximum_iter - 1:
            out["P"] = np.array(r["P"], float)
            break
    out["x"] = x
    out["dx"], out["xs"] = np.array(out["dx"]), np.array(out["xs"])
    return out


def step_error(r, ref, with_P):
    """max over dx, x and (with_P) P / max(1, max|P_mp|) of an f64 step result against a 50-digit one; inf where not finite."""
    vals = [r["dx"], r["x"]] + ([r["P"]] if with_P else [])
    if not all(np.isfinite(np.asarray(v, float)).all() for v in vals):
        return float("inf")
    e = max(mm.err(r["dx"], ref["dx_mp"]), mm.err(r["x"], ref["x_mp"]))
    if with_P:
        e = max(e, mm.err_mat(r["P"], ref["P_mp"]) / max(1.0, float(np.abs(ref["P"]).max())))
    return e


def chain_error(run, ref):
    """The error of an f64 chain against the 50-digit chain of the same case, pass by pass; inf on another pass count."""
    if run["passes"] != ref["passes"]:
        return float("inf")
    e = 0.0
    for k in range(ref["passes"]):
        if ref["steps"][k] is None:
            continue
        last = k == ref["passes"] - 1
        r = dict(dx=run["dx"][k], x=run["xs"][k], P=run["P"])
        e = max(e, step_error(r, ref["steps"][k], with_P=last and ref["steps"][k]["P"] is not None))
    return e


def bound(e_o, e_f, dx_inf):
    """What the device is held to, for x and for P / max(1, max|P_mp|): 8 x the worse of the two f64 yardsticks' own errors, with
    the floor 1e-12 max(1, |dx|_inf).  A yardstick that is not finite (the oracle on a singular P) does not enter."""
    es = [e for e in (e_o, e_f) if np.isfinite(e)]
    assert es
    return max(DEVICE_FACTOR * max(es), FLOOR * max(1.0, dx_inf))


def admitted(e_o, e_f, dx_inf, needs_oracle=True):
    if not np.isfinite(e_f) or (needs_oracle and not np.isfinite(e_o)):
        return False
    return (np.isfinite(e_o) and e_f <= 8.0 * e_o) or e_f <= 1e-13 * max(1.0, dx_inf)


# ---- the records ----------------------------------------------------------------------------------------------------------------
def make_record(ext, seed, d12, rows=fc.ROWS, row_scale=fc.ROW_SCALE):
    """filter_cases.make_record with the number of rows and their scale free: H [rows, 12] ~ row_scale N(0, 1) in the live
    columns, h = H d.  rows < 6 (12) gives a rank-deficient H^T H."""
    rng = np.random.default_rng(seed)
    n = 12 if ext else 6
    H = np.zeros((rows, 12))
    H[:, :n] = rng.normal(size=(rows, n)) * row_scale
    return record_of(H, d12, n)


def record_of(H, d12, n):
    d = np.zeros(12)
    d[:n] = np.asarray(d12, float)[:n]
    h = H @ d
    return dict(HTH=H.T @ H, HTh=H.T @ h, n_valid=len(H), sum_h2=float(h @ h))


def corridor_record(ext, seed, d12):
    """5 rows base + 1e-3 noise: five near-parallel planes, a corridor's walls."""
    rng = np.random.default_rng(seed)
    n = 12 if ext else 6
    H = np.zeros((5, 12))
    base = rng.normal(size=n) * fc.ROW_SCALE
    H[:, :n] = base + 1e-3 * rng.normal(size=(5, n))
    return record_of(H, d12, n)


def pose_eigenvalues(rec):
    return np.sort(np.linalg.eigvalsh(np.asarray(rec["HTH"])[:6, :6]))[::-1]


ILL_SCALE = np.array([1e2] * 3 + [1e-4] * 3 + [1e-3] * 6 + [1.0] * 3 + [1e-3] * 6 + [1e-2] * 2)


def _case(name, ext, x0, P, records, R=1e-3, limits=None, max_num_iters=None, predicates=(), keep=None, passes=None, seed=None):
    return dict(name=f"{name}-ext{ext}", ext=ext, x0=np.array(x0, float), P=np.array(P, float), records=list(records), R=float(R),
                limits=np.array([LIMIT] * 23 if limits is None else limits, float),
                max_num_iters=len(records) - 1 if max_num_iters is None else max_num_iters, predicates=list(predicates), keep=keep,
                want_passes=passes, seed=seed)


def _obs(ext):
    return 12 if ext else 6


def _table(oracle):
    rot = {c["name"]: c for c in fc.cases(oracle)}
    out = []
    for ext in (0, 1):
        base = rot[f"rot0.3-ext{ext}"]          # OFF_R, the predicted P, records d and 0.3 d at H^T H ~ 4e4 I
        x0, Pp, recs = base["x0"], base["P"], base["records"]
        d = fc.increment(0.3, ext)
        n = _obs(ext)
        # R sweep (the group predicate — R really enters — is asserted in cases())
        for R in (1e-6, 1.0, 100.0):
            out.append(_case(f"R{R:g}", ext, x0, Pp, recs, R=R))
        # weak scan: H^T H ~ 0.04 I against (P / R)^-1 ~ 1 on the pose and 1e5 on the extrinsics
        weak = [make_record(ext, 500 + ext, d, row_scale=0.01), make_record(ext, 510 + ext, 0.3 * d, row_scale=0.01)]
        out.append(_case("weak-scan", ext, x0, Pp, weak, R=1.0, predicates=[
            ("H^T H ~ 0.04 I", lambda c: 0.02 < np.diag(c["records"][0]["HTH"])[:_obs(c["ext"])].mean() < 0.08),
            ("the observed dofs move by less than half of d", lambda c, d=d, n=n: np.all(np.abs(c["mp"]["dx"][0][:n]) < 0.5 * np.abs(d[:n]))),
            ("... and the scan still moves them", lambda c, n=n: np.abs(c["mp"]["dx"][0][:n]).max() > 1e-3)]))
        out.append(_case("prior-wide", ext, x0, Pp * 1e4, recs))
        out.append(_case("prior-tight", ext, x0, Pp * 1e-6, recs))
        out.append(_case("prior-ill", ext, x0, ILL_SCALE[:, None] * Pp * ILL_SCALE[None, :], recs,
                         predicates=[("cond(P) >= 1e14", lambda c: np.linalg.cond(c["P"]) >= 1e14)]))
        # corridor: the seeds are the first that the admission rule takes (see cases())
        degenerate = ("the 6th eigenvalue of the pose block is below 1e-4 of the first",
                      lambda c: all(pose_eigenvalues(r)[5] < 1e-4 * pose_eigenvalues(r)[0] for r in c["records"]))
        for name, P, R, seed in (("corridor-default", synth.default_P0(), 1e-3, 600), ("corridor-wide-R1e-6", Pp * 1e4, 1e-6, 620)):
            out.append(_case(name, ext, x0, P, [corridor_record(ext, seed + ext, d), corridor_record(ext, seed + 10 + ext, 0.3 * d)],
                             R=R, predicates=[degenerate], seed=seed))
        for rows in (1, 3, 6):
            few = [make_record(ext, 700 + 10 * rows + ext, d, rows=rows), make_record(ext, 705 + 10 * rows + ext, 0.3 * d, rows=rows)]
            out.append(_case(f"rows{rows}", ext, x0, synth.default_P0(), few, predicates=[
                ("n_valid and the rank are the row count", lambda c, rows=rows: all(
                    r["n_valid"] == rows and np.linalg.matrix_rank(r["HTH"]) == rows for r in c["records"]))]))
        if not ext:
            P0 = Pp.copy()
            P0[6:12, :] = 0.0
            P0[:, 6:12] = 0.0
            keep = [i for i in range(23) if not 6 <= i < 12]
            out.append(_case("zero-variance", 0, x0, P0, recs, keep=keep, predicates=[
                ("rows and columns 6..11 of P are exactly zero", lambda c: not c["P"][6:12].any() and not c["P"][:, 6:12].any()),
                ("the reference leaves those dofs and their P alone", lambda c: not c["mp"]["dx"][:, 6:12].any()
                 and not c["mp"]["P"][6:12].any() and not c["mp"]["P"][:, 6:12].any())]))
        out += _ending_cases(oracle, ext, x0, Pp, d)
    return out


def _ending_cases(oracle, ext, x0, Pp, d):
    """Per-dof limits and the way an update ends: MAX_NUM_ITERS = 3, records d, 0.3 d, 0.09 d, 0.027 d (every increment below 1)."""
    recs = [make_record(ext, 800 + 10 * k + ext, s * d) for k, s in enumerate((1.0, 0.3, 0.09, 0.027))]
    uniform = _case("limits-uniform", ext, x0, Pp, recs, limits=[1.0] * 23, passes=2)
    out = [uniform]
    dofs = (0, 5, 12, 22) + ((11,) if ext else (8,))
    P_dof = {j: Pp for j in dofs}
    if not ext:
        # offset_R_L_I has no flow and no process noise: five predictions leave dof 8 uncorrelated, and its increment exactly
        # zero.  The case wants it to move through P's correlations, so the predicted P gets one more rank-one term
        assert not Pp[8, :8].any() and not Pp[8, 9:].any()
        u = np.zeros(23)
        u[1], u[8] = 1.0, 1e-3
        P_dof[8] = Pp + np.outer(u, u)
    for j in sorted(dofs):
        lim = np.ones(23)
        lim[j] = 1e-12
        out.append(_case(f"limits-tight-dof{j}", ext, x0, P_dof[j], recs, limits=lim, passes=4, predicates=[
            (f"dof {j} moves on every pass, a decade beyond its limit", lambda c, j=j: np.all(np.abs(c["mp"]["dx"][:, j]) > 1e-11)),
            ("every other dof stays below its limit", lambda c, j=j: np.all(np.delete(np.abs(c["mp"]["dx"]), j, axis=1) < 1.0))]))
    # the threshold from both sides, on an observed dof: limits[j] = |dx_j| (1 -+ 1e-6) of the ORACLE's pass 1 and pass 2
    run = chain(oracle_step(oracle, uniform), uniform)
    assert run["passes"] == 2
    j = 10 if ext else 1
    for k, want in ((0, (3, 2)), (1, (4, 3))):
        for side, passes in zip((-1, +1), want):
            lim = np.ones(23)
            lim[j] = abs(run["dx"][k][j]) * (1 + side * 1e-6)
            out.append(_case(f"limits-pass{k + 1}-{'below' if side < 0 else 'above'}", ext, x0, Pp, recs, limits=lim, passes=passes))
    # two converged passes that are not adjacent
    recs2 = [make_record(ext, 900 + 10 * k + ext, s * d) for k, s in enumerate((1.0, 1e-4, 1.0, 1e-4))]
    # (with extrinsic estimation the prior of the extrinsics, R / P = 100 against H^T H ~ 4e4, pulls back 0.25 % of the 2 d the
    # state has moved by pass 4 — above the limit; a prior 100 x wider keeps the pull-back two decades below it)
    out.append(_case("limits-converged-apart", ext, x0, Pp * 100.0 if ext else Pp, recs2, limits=[1e-3 * np.abs(d).max()] * 23, passes=4, predicates=[
        ("conv is [F, T, F, T]: the update ends on pass 4 by t > 1", lambda c: c["oracle"]["conv"] == [False, True, False, True]
         and c["mp"]["conv"] == [False, True, False, True])]))
    return out


_CACHE = {}


def cases(oracle):
    """The table, every case with its three runs, its errors, its predicates and the admission rule asserted."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = _table(oracle)
    for c in out:
        c["mp"] = chain(mp_step(c), c)
        c["oracle"] = chain(oracle_step(oracle, c), c)
        c["block"] = chain(block_step(oracle, c), c)
        ref = c["mp"]
        c["dx_inf"] = float(np.abs(ref["dx"]).max())
        # (on a P without variance in some dofs the oracle inverts a singular matrix: whatever it returns is no yardstick)
        c["e_o"] = chain_error(c["oracle"], ref) if c["keep"] is None else float("inf")
        c["e_f"] = chain_error(c["block"], ref)
        c["bound"] = bound(c["e_o"], c["e_f"], c["dx_inf"])
        assert np.isfinite(ref["x"]).all() and np.isfinite(ref["P"]).all(), c["name"]
        assert c["block"]["passes"] == ref["passes"], c["name"]
        if c["keep"] is None:
            assert c["oracle"]["passes"] == ref["passes"] and c["oracle"]["conv"] == ref["conv"], c["name"]
        assert c["block"]["conv"] == ref["conv"], c["name"]
        if c["want_passes"] is not None:
            assert ref["passes"] == c["want_passes"], (c["name"], ref["passes"])
        # no |dx_i| within rounding of its limit: the pass count is the kernel's to get right, not a coin
        for dx in ref["dx"]:
            assert np.all(np.abs(np.abs(dx) - c["limits"]) >= 1e-7 * c["limits"]), c["name"]
        for what, pred in c["predicates"]:
            assert pred(c), f"{c['name']}: {what}"
        assert admitted(c["e_o"], c["e_f"], c["dx_inf"], needs_oracle=c["keep"] is None), (c["name"], c["e_o"], c["e_f"])
    by = {c["name"]: c for c in out}
    assert len(by) == len(out)
    for ext in (0, 1):
        # R really enters: the state increment of the update, x [-] x0, at R = 100 is not the one at R = 1e-6
        inc = [oracle.boxminus(by[f"R{r}-ext{ext}"]["oracle"]["x"], by[f"R{r}-ext{ext}"]["x0"]) for r in ("100", "1e-06")]
        assert np.abs(inc[0] - inc[1]).max() > 1e-3
        # every tight-limit case ends differently from the uniform one, and the two sides of a threshold differ
        uni = by[f"limits-uniform-ext{ext}"]["oracle"]["passes"]
        assert uni == 2
        for c in out:
            if c["ext"] == ext and c["name"].startswith("limits-tight"):
                assert c["oracle"]["passes"] == 4 != uni, c["name"]
        for k in (1, 2):
            assert by[f"limits-pass{k}-below-ext{ext}"]["oracle"]["passes"] != by[f"limits-pass{k}-above-ext{ext}"]["oracle"]["passes"]
    _CACHE["cases"] = out
    return out


NAMES = [f"{n}-ext{ext}" for ext in (0, 1) for n in
         ["R1e-06", "R1", "R100", "weak-scan", "prior-wide", "prior-tight", "prior-ill", "corridor-default", "corridor-wide-R1e-6",
          "rows1", "rows3", "rows6"] + (["zero-variance"] if not ext else []) +
         ["limits-uniform"] + [f"limits-tight-dof{j}" for j in sorted((0, 5, 12, 22) + ((11,) if ext else (8,)))] +
         ["limits-pass1-below", "limits-pass1-above", "limits-pass2-below", "limits-pass2-above", "limits-converged-apart"]]
