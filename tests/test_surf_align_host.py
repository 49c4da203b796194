"""The rule of lv_surf_align.hpp (the trilinear sample with its gradient, one evaluation's H, g and E, the cost, the
Levenberg-Marquardt turn, the argument rules: what the kernels of lv_surf_align.hip run) compiled with g++ and
-fsanitize=address,undefined through tests/emu/hip/hip_runtime.h as a stand-alone program (tests/emu/surf_align_emu.cpp) and held
to tests/surf_align_ref.py: the sample by equality (only + - * / and floor occur: the repr of a double round-trips), the sums of
an evaluation within 1e-12 relative, the whole loop by the device test's own bounds."""
import math
import os
import subprocess

import numpy as np
import pytest

import surf_align_cases as cases
import surf_align_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
TOL = 1e-12


def _f(v):
    return " ".join(repr(float(x)) for x in np.asarray(v, float).reshape(-1))


def _vol(v, min_weight=1):
    head = f"{_f(v['origin'])} {float(v['resolution'])!r} {v['nx']} {v['ny']} {v['nz']} {min_weight}"
    return head + "\n" + " ".join(map(str, np.asarray(v["S"]).reshape(-1).tolist())) + "\n" + " ".join(map(str, np.asarray(v["W"]).reshape(-1).tolist()))


def _pts(p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return f"{len(p)}\n" + "\n".join(_f(r) for r in p)


def _prm(**kw):
    a = dict(sr.ALIGN, **kw)
    return f"{a['min_weight']} {a['max_iterations']} {a['min_points']} " + _f([a[k] for k in ("max_dist", "huber", "step_tol", "lambda_init", "lambda_min",
                                                                                                "lambda_max")])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("surf_align_host") / "surf_align_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "surf_align_emu.cpp"), "-o", str(exe)])

    def run(mode, text):
        return subprocess.run([str(exe)], input=f"{mode}\n{text}\n".encode(), stdout=subprocess.PIPE, check=True).stdout.decode().strip().split("\n")

    return run


def _rel(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _check_sample(emu, vol, pts, min_weight):
    out = emu(0, _vol(vol, min_weight) + "\n" + _pts(pts))
    d, n, status = sr.sample(vol, pts, min_weight)
    got = np.array([row.split() for row in out], float)
    assert len(got) == len(pts)
    assert np.array_equal(got[:, 0].astype(np.uint8), status)
    assert np.array_equal(got[:, 1], d) and np.array_equal(got[:, 2:], n)          # the same bits
    return status


def test_sample_is_the_reference(emu):
    pts = cases.sample_points(np.random.default_rng(2)).astype(np.float64)
    status = _check_sample(emu, cases.volume(), pts, 1)
    assert (np.bincount(status, minlength=3) >= 300).all()
    s3 = _check_sample(emu, cases.volume(True), pts, 3)
    assert ((status == sr.KNOWN) & (s3 == sr.UNKNOWN)).sum() >= 100
    # the transformed source points of a case, which are not f32 numbers
    x, _, _ = sr.transform(cases.source(), cases.guesses()[2])
    _check_sample(emu, cases.volume(), x, 1)
    exact, _ = cases.exact_points(np.random.default_rng(1), 500)
    _check_sample(emu, cases.linear_volume(), exact.astype(np.float64), 1)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_one_evaluation(emu, name):
    c = cases.CASES[name]()
    s = dict(sr.ALIGN, **c["solve"])
    for pose in c["guesses"][:4]:
        out = emu(1, "\n".join([_vol(c["vol"], s["min_weight"]), _pts(c["source"]), _f(pose), _f([s["max_dist"], s["huber"]])]))
        acc, n_in = sr.evaluate(c["vol"], c["source"], pose, s["min_weight"], s["max_dist"], s["huber"])
        got = np.array(out[0].split(), float)
        assert int(out[1]) == n_in and n_in > 100
        assert abs(got[27] - acc[27]) <= TOL * acc[27] and _rel(got[21:27], acc[21:27]) <= TOL and _rel(got[:21], acc[:21]) <= TOL
        want = sr.cost_of(acc[27], len(c["source"]), n_in, s["max_dist"], s["huber"])
        assert abs(float(out[2]) - want) <= TOL * want


def test_no_overlap_evaluation(emu):
    c = cases.corner()
    out = emu(1, "\n".join([_vol(c["vol"]), _pts(c["source"]), _f(c["guesses"][4]), "0.25 0.1"]))
    assert not np.array(out[0].split(), float).any() and int(out[1]) == 0
    assert float(out[2]) == pytest.approx(len(c["source"]) * 0.1 * (0.25 - 0.05), rel=1e-15)      # everyone pays the gate


@pytest.mark.parametrize("name", list(cases.CASES))
def test_loop(emu, name):
    """align_turn over SurfAlignRule on the host against the reference's loop, by the bounds the device is held to"""
    c = cases.CASES[name]()
    ref, best = cases.reference(name)
    g = c["guesses"]
    out = emu(5, "\n".join([_vol(c["vol"]), _pts(c["source"]), _prm(**c["solve"]), str(len(g))] + [_f(x) for x in g]))
    got = []
    for k, r in enumerate(ref):
        head, ints, info = np.array(out[3 * k].split(), float), [int(v) for v in out[3 * k + 1].split()], np.array(out[3 * k + 2].split(), float)
        assert ints == [r["n_in"], r["status"], r["accepted"], r["rejected"]], (k, ints)
        got.append(dict(cost=head[7], n_in=ints[0], status=ints[1]))
        if r["status"] == sr.NO_OVERLAP:
            assert np.array_equal(head[:7], g[k]) and head[7] == 0.0 and not info.any()
            continue
        assert sr.pose_distance(head[:7], r["pose"]) <= 1e-8 and abs(head[7] - r["cost"]) <= 1e-9 * r["cost"]
        assert np.abs(info - r["info"]).max() <= 1e-9 * np.abs(r["info"]).max()
        assert head[8] == pytest.approx(r["last_step"], rel=1e-6, abs=1e-12) and head[9] == pytest.approx(r["lambda"], rel=1e-12)
    unique = cases.check_best(tuple(int(v) for v in out[-1].split()), got, name)
    assert unique == (name in ("floor", "weights"))      # on these two the reference's best is the only answer


def test_loop_edges(emu):
    c = cases.corner()
    g = c["guesses"][[1, 4]]
    text = lambda **kw: "\n".join([_vol(c["vol"]), _pts(c["source"]), _prm(**dict(c["solve"], **kw)), "2"] + [_f(x) for x in g])
    out = emu(5, text(max_iterations=0))      # only scores the guesses
    acc, n_in = sr.evaluate(c["vol"], c["source"], g[0], 1, 0.25, 0.1)
    want = sr.cost_of(acc[27], len(c["source"]), n_in, 0.25, 0.1)
    head = np.array(out[0].split(), float)
    assert np.array_equal(head[:7], g[0]) and abs(head[7] - want) <= TOL * want and out[1] == f"{n_in} {sr.MAX_ITERATIONS} 0 0"
    assert np.array_equal(np.array(out[3].split(), float)[:7], g[1]) and out[4] == f"0 {sr.NO_OVERLAP} 0 0" and out[-1] == f"0 {n_in}"
    out = emu(5, text(min_points=len(c["source"]) + 1))      # more points asked for than there are: NO_OVERLAP at the guess
    assert out[1] == f"0 {sr.NO_OVERLAP} 0 0" and out[-1] == "-1 -1"


def test_defaults(emu):
    out = emu(6, "")
    a = sr.ALIGN
    assert out[0] == f"{a['min_weight']} {a['max_iterations']} {a['min_points']} 0"
    assert [float(v) for v in out[1].split()] == [a[k] for k in ("max_dist", "huber", "step_tol", "lambda_init", "lambda_min", "lambda_max")]
    assert (a["max_iterations"], a["min_points"], a["max_dist"], a["huber"]) == (50, 6, 0.4, 0.1)


def test_align_params_rule(emu):
    bad = [dict(min_weight=0), dict(min_weight=-3), dict(max_iterations=-1), dict(max_iterations=1001), dict(min_points=0), dict(max_dist=0.0),
           dict(max_dist=-1.0), dict(max_dist=math.inf), dict(max_dist=math.nan), dict(huber=-1e-9), dict(huber=math.inf), dict(huber=math.nan),
           dict(step_tol=-1e-12), dict(step_tol=math.inf), dict(lambda_min=0.0), dict(lambda_init=1e-11), dict(lambda_init=1e9),
           dict(lambda_max=math.inf), dict(lambda_min=math.nan)]
    good = [dict(), dict(min_weight=1 << 18), dict(max_iterations=0), dict(max_iterations=1000), dict(min_points=1), dict(huber=0.0), dict(step_tol=0.0),
            dict(lambda_init=1e-10), dict(lambda_init=1e8)]
    out = emu(2, f"{len(bad) + len(good)}\n" + "\n".join(_prm(**kw) for kw in bad + good))
    assert all(o.startswith("bad: ") for o in out[:len(bad)]), out
    assert out[len(bad):] == ["ok"] * len(good)
    for o, what in zip(out, ["min_weight"] * 2 + ["max_iterations"] * 2 + ["min_points"] + ["max_dist"] * 4 + ["huber"] * 3 + ["step_tol"] * 2 + ["lambda"] * 5):
        assert what in o, (o, what)


def test_align_arguments_rule(emu):
    # has_src stride n_src has_guesses K has_results has_best, the last guess' q and t0
    unit = "0 0 0 1 0"
    rows = [("1 12 400 1 8 1 1 " + unit, "ok"), ("0 0 0 1 8 1 1 " + unit, "ok"), ("0 0 0 0 0 0 1 " + unit, "ok"),
            ("1 12 1048576 1 1024 1 1 " + unit, "ok"), ("1 16 4 1 4096 1 1 " + unit, "ok"), ("1 12 4 1 3 1 1 0 0 0 1.0000009 0", "ok"),
            ("1 12 400 1 8 1 0 " + unit, "null best"), ("1 12 4 1 4097 1 1 " + unit, "K = 4097"), ("1 12 1048577 1 1 1 1 " + unit, "n_src"),
            ("1 12 1048576 1 1025 1 1 " + unit, "2^30"), ("0 12 4 1 1 1 1 " + unit, "source"), ("1 8 4 1 1 1 1 " + unit, "stride 8"),
            ("1 12 4 0 2 1 1 " + unit, "null guesses"), ("1 12 4 1 2 0 1 " + unit, "null results"),
            ("1 12 4 1 3 1 1 0 0 0 1.000002 0", "guess 2: q: norm"), ("1 12 4 1 3 1 1 0 0 nan 1 0", "guess 2: q: a non-finite"),
            ("1 12 4 1 2 1 1 0 0 0 1 inf", "guess 1: t: a non-finite")]
    out = emu(3, f"{len(rows)}\n" + "\n".join(r for r, _ in rows))
    for o, (_, want) in zip(out, rows):
        assert (o == "ok") if want == "ok" else (o.startswith("bad: lv_surf_align: ") and want in o), (o, want)


def test_sample_arguments_rule(emu):
    # min_weight has_pts stride n has_out has_status
    rows = [("1 1 12 100 1 1", "ok"), ("1 1 12 100 1 0", "ok"), ("1 1 12 100 0 1", "ok"), ("7 0 0 0 1 1", "ok"), ("1 1 16 2147483646 1 1", "ok"),
            ("0 1 12 100 1 1", "min_weight = 0"), ("1 1 12 100 0 0", "both null"), ("1 1 12 2147483647 1 1", "too many"),
            ("1 0 12 100 1 1", "bad point array"), ("1 1 8 100 1 1", "stride 8")]
    out = emu(4, f"{len(rows)}\n" + "\n".join(r for r, _ in rows))
    for o, (_, want) in zip(out, rows):
        assert (o == "ok") if want == "ok" else (o.startswith("bad: lv_surf_sample: ") and want in o), (o, want)
