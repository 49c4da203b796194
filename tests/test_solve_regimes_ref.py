"""CPU tests of what tests/test_gpu_solve_regimes.py compares the device with: the 50-digit kf_step of tests/manifold_mp.py
and the case table of tests/solve_regimes.py.

Measured here (x86-64, glibc libm):
* the 50-digit step against oracle.kf_step over the 28 cases of tests/filter_cases.py (the default regime, well conditioned):
  dx and x within 5e-15.  The posterior P within 5.6e-12 absolute — in the grav-down-86deg cases, whose PRIOR holds entries of
  18 265 (filter_cases.grav_moving_P) while the posterior's largest entry is 3.4: the posterior is the difference L - K_x P_ of
  terms of the prior's size, so one ulp of the prior (3.6e-12) is the floor of any f64 statement.  P is therefore held to
  1e-12 of max(1, max|P_prop|, max|P|); with that scale the worst case is 1.0e-15 (rot0.01-ext1).
* the table's own figures e_o (oracle) and e_f (f64 block form) are printed by test_admission_rule."""
import numpy as np
import pytest

import filter_cases as fc
import manifold_mp as mm
import solve_regimes as sr

TOL = 1e-12


@pytest.fixture(scope="module")
def table(oracle):
    return sr.cases(oracle)


def _default_case(c):
    return dict(name="fc-" + c["name"], ext=c["ext"], x0=c["x0"], P=c["P"], records=c["records"], R=1e-3, limits=np.full(23, fc.LIMIT),
                max_num_iters=len(c["records"]) - 1, keep=None)


def test_50_digit_step_against_the_oracle_in_the_default_regime(oracle):
    worst = dict(dx=(0.0, None), x=(0.0, None), P=(0.0, None))
    for c in fc.cases(oracle):
        case, run = _default_case(c), c["run"]
        step = sr.mp_step(case)
        prm = fc.params_for(oracle, c)
        before = c["x0"]
        for k, rec in enumerate(c["records"]):
            if rec["n_valid"]:
                ref = step(before, rec)
                xs, dx, conv, P = oracle.kf_step(before, c["x0"], c["P"], rec, params=prm, finalize=True)
                assert np.array_equal(xs, run["xs"][k]) and np.array_equal(dx, run["dx"][k])
                assert conv == ref["conv"] == run["conv"][k]
                scale = max(1.0, np.abs(c["P"]).max(), np.abs(ref["P"]).max())
                for what, e in (("dx", mm.err(dx, ref["dx_mp"])), ("x", mm.err(xs, ref["x_mp"])), ("P", mm.err_mat(P, ref["P_mp"]) / scale)):
                    if e > worst[what][0]:
                        worst[what] = (e, (c["name"], k))
                    assert e <= TOL, (c["name"], k, what, e)
            before = run["xs"][k]
    print("oracle.kf_step vs 50 digits, filter_cases: " + ", ".join(f"{w} {e:.2e} at {at}" for w, (e, at) in worst.items()))


def test_50_digit_chain_against_run_chain(oracle):
    """The 50-digit chain (solve_regimes.chain) against filter_cases.run_chain, which test_filter_cases_ref holds to oracle.update:
    the same passes, the same conv, x and P at 1e-12 (P relative to the prior's largest entry: the module's note)."""
    for c in fc.cases(oracle):
        case, run = _default_case(c), c["run"]
        ref = sr.chain(sr.mp_step(case), case)
        assert ref["passes"] == run["passes"] and ref["conv"] == run["conv"], c["name"]
        scale = max(1.0, np.abs(c["P"]).max())
        assert np.abs(ref["x"] - run["x"]).max() <= TOL and np.abs(ref["P"] - run["P"]).max() <= TOL * scale, c["name"]
        assert np.abs(ref["xs"] - run["xs"]).max() <= TOL and np.abs(ref["dx"] - run["dx"]).max() <= TOL, c["name"]


@pytest.mark.parametrize("max_num_iters", [3, 8])
def test_50_digit_chain_against_oracle_update(oracle, scene_small, max_num_iters):
    """... and against oracle.update itself, fed with the sums of its own passes: by count with MAX_NUM_ITERS = 3, by the second
    converged pass with room for eight."""
    sc = scene_small
    prm = oracle.default_params(max_num_iters=max_num_iters)
    x, P, passes, trace, sums = oracle.update(sc["x_init"], sc["P0"], sc["map_xyz"], sc["scan_xyz"][:600], params=prm, tree=oracle.KdTree(sc["map_xyz"]))
    case = dict(name=f"update-{max_num_iters}", ext=0, x0=sc["x_init"], P=sc["P0"], records=sums, R=1e-3, limits=np.full(23, fc.LIMIT),
                max_num_iters=max_num_iters, keep=None)
    ref = sr.chain(sr.mp_step(case), case)
    assert ref["passes"] == passes and (passes < max_num_iters + 1) == (max_num_iters == 8)
    ex, eP = np.abs(ref["x"] - x).max(), np.abs(ref["P"] - P).max()
    print(f"MAX_NUM_ITERS {max_num_iters}: passes {passes}, |x - x_mp| {ex:.2e}, |P - P_mp| {eP:.2e}")
    assert ex <= TOL and eP <= TOL
    assert np.abs(ref["dx"] - trace[:, :23]).max() <= TOL


def test_reduced_step_is_the_limit_of_the_full_one(oracle, table):
    """kf_step_reduced on the 17 dofs with variance against kf_step with variance 1e-30 on the other six (50 digits carry it)."""
    c = next(c for c in table if c["name"] == "zero-variance-ext0")
    P = c["P"].copy()
    P[range(6, 12), range(6, 12)] = 1e-30
    full = mm.kf_step(c["x0"], c["x0"], P, c["records"][0], c["R"], c["limits"], True)
    red = c["mp"]["steps"][0]
    assert mm.err(red["dx"], full["dx_mp"]) <= 1e-15 and mm.err(red["x"], full["x_mp"]) <= 1e-15
    assert mm.err_mat(red["P"], full["P_mp"]) <= 1e-15 * max(1.0, np.abs(red["P"]).max())


def test_table_holds_the_required_cases(table):
    assert [c["name"] for c in table] == sr.NAMES
    by = {c["name"]: c for c in table}
    for ext in (0, 1):
        assert [by[f"R{r}-ext{ext}"]["R"] for r in ("1e-06", "1", "100")] == [1e-6, 1.0, 100.0]
        assert by[f"corridor-default-ext{ext}"]["R"] == 1e-3 and by[f"corridor-wide-R1e-6-ext{ext}"]["R"] == 1e-6
        assert np.array_equal(by[f"prior-wide-ext{ext}"]["P"], by[f"R1-ext{ext}"]["P"] * 1e4)
        assert np.array_equal(by[f"prior-tight-ext{ext}"]["P"], by[f"R1-ext{ext}"]["P"] * 1e-6)
        assert [by[f"rows{n}-ext{ext}"]["records"][0]["n_valid"] for n in (1, 3, 6)] == [1, 3, 6]
        assert by[f"limits-uniform-ext{ext}"]["mp"]["passes"] == 2
        for j in (0, 5, 12, 22, 11 if ext else 8):
            c = by[f"limits-tight-dof{j}-ext{ext}"]
            assert c["mp"]["passes"] == 4 and c["limits"][j] == 1e-12 and np.all(np.delete(c["limits"], j) == 1.0)
        assert [by[f"limits-pass{k}-{s}-ext{ext}"]["mp"]["passes"] for k in (1, 2) for s in ("below", "above")] == [3, 2, 4, 3]
        assert by[f"limits-converged-apart-ext{ext}"]["mp"]["conv"] == [False, True, False, True]
    assert "zero-variance-ext0" in by and "zero-variance-ext1" not in by
    for c in table:
        assert c["max_num_iters"] == len(c["records"]) - 1
        if c["name"].startswith("limits"):
            assert c["max_num_iters"] == 3
        for r in c["records"]:   # a record is what the device reduces: symmetric, zero outside the live columns
            assert np.array_equal(r["HTH"], r["HTH"].T)
            if not c["ext"]:
                assert not r["HTH"][6:].any() and not r["HTh"][6:].any()


def test_predicates_hold(table):
    """cases() asserted them; once more, by name, so that a predicate that went missing shows."""
    n = 0
    for c in table:
        for what, pred in c["predicates"]:
            assert pred(c), (c["name"], what)
            n += 1
    assert n >= 30


def test_admission_rule(table):
    print()
    for c in table:
        print(f"{c['name']:30s} passes {c['mp']['passes']}  |dx|_inf {c['dx_inf']:9.3e}  e_o {c['e_o']:9.2e}  e_f {c['e_f']:9.2e}  bound {c['bound']:9.2e}")
        assert np.isfinite(c["e_f"]), c["name"]
        if c["keep"] is None:
            assert np.isfinite(c["e_o"]), c["name"]
            assert c["e_f"] <= 8 * c["e_o"] or c["e_f"] <= 1e-13 * max(1.0, c["dx_inf"]), (c["name"], c["e_o"], c["e_f"])
        else:
            assert c["e_f"] <= 1e-13 * max(1.0, c["dx_inf"]), (c["name"], c["e_f"])
        assert c["bound"] == max(8 * max(e for e in (c["e_o"], c["e_f"]) if np.isfinite(e)), 1e-12 * max(1.0, c["dx_inf"]))
