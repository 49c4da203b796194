"""The rule of lv_ndt.hpp (the voxel of a point, the Gaussians from integer moments, one evaluation's S, g, H, the
Levenberg-Marquardt turn, the argument rules: what the kernels of lv_ndt.hip run) compiled with g++ and
-fsanitize=address,undefined through tests/emu/hip/hip_runtime.h as a stand-alone program (tests/emu/ndt_emu.cpp) and held to
tests/ndt_ref.py: the moments by equality, the f64 algebra within 1e-12 relative (libm differs between the two, so not by bits).
The whole loop on the host is held to the reference's by the device test's own bounds."""
import math
import os
import subprocess

import numpy as np
import pytest

import graph_ref as gr
import ndt_cases as cases
import ndt_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
TOL = 1e-12


def _f(v):
    return " ".join(repr(float(x)) for x in np.asarray(v, float).reshape(-1))


def _prm(p):
    return f"{_f(p['origin'])} {float(p['resolution'])!r} {p['nx']} {p['ny']} {p['nz']} {p['min_points']} {float(p['reg'])!r}"


def _pts(p):
    p = np.asarray(p, np.float32).reshape(-1, 3)
    return f"{len(p)}\n" + "\n".join(_f(r) for r in p)


def _align_prm(**kw):
    a = dict(nr.ALIGN, **kw)
    return f"{a['search']} {a['max_iterations']} " + _f([a[k] for k in ("d2", "step_tol", "lambda_init", "lambda_min", "lambda_max")])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ndt_host") / "ndt_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "ndt_emu.cpp"), "-o", str(exe)])

    def run(mode, text):
        return subprocess.run([str(exe)], input=f"{mode}\n{text}\n".encode(), stdout=subprocess.PIPE, check=True).stdout.decode().strip().split("\n")

    return run


def _rel(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _check_target(out, T):
    assert [int(v) for v in out[0].split()] == nr.stats(T)
    occupied = np.nonzero(T["n"])[0]
    assert len(out) == 1 + 2 * len(occupied)
    for k, c in enumerate(occupied):
        ints = [int(v) for v in out[1 + 2 * k].split()]
        assert ints == [c, T["n"][c]] + T["S1"][c].tolist() + T["S2"][c].tolist(), c     # bit-equal
        row = np.array(out[2 + 2 * k].split(), float)
        if T["n"][c] < 5:
            assert not row.any()
            continue
        assert _rel(row[:3], T["mean"][c]) <= TOL and _rel(row[3:9], T["cov"][c]) <= TOL and _rel(row[9:], T["icov"][c]) <= TOL, c
        assert np.abs(nr.full3(row[3:9]) @ nr.full3(row[9:]) - np.eye(3)).max() <= 1e-9


@pytest.mark.parametrize("name", ["corner-near", "plane"])
def test_target(emu, name):
    c = cases.ALIGN_CASES[name]()
    _check_target(emu(0, _prm(c["prm"]) + "\n" + _pts(c["target"])), cases.target(name))


def test_target_edge_cases(emu):
    for prm, pts in (cases.coincident(), cases.dirty()):
        _check_target(emu(0, _prm(prm) + "\n" + _pts(pts)), nr.build(prm, pts))


@pytest.mark.parametrize("name,search", [("corner-near", 7), ("corner-near", 1), ("corner-far", 7), ("plane", 7)])
def test_one_evaluation(emu, name, search):
    c = cases.ALIGN_CASES[name]()
    T = cases.target(name)
    for pose in (c["guesses"][0], c["guesses"][5], c["truth"]):
        out = emu(1, "\n".join([_prm(c["prm"]), _pts(c["target"]), _pts(c["source"]), _f(pose), f"{search} {cases.D2!r}"]))
        acc, n_in = nr.evaluate(c["prm"], T, c["source"], pose, search, cases.D2)
        got = np.array(out[0].split(), float)
        assert int(out[1]) == n_in and n_in > 300
        assert abs(got[27] - acc[27]) <= TOL * acc[27] and _rel(got[21:27], acc[21:27]) <= TOL and _rel(got[:21], acc[:21]) <= TOL


def test_no_overlap_evaluation(emu):
    c = cases.corner_near()
    far = np.array([500.0, 0, 0, 0, 0, 0, 1])
    out = emu(1, "\n".join([_prm(c["prm"]), _pts(c["target"]), _pts(c["source"]), _f(far), "7 0.43"]))
    assert not np.array(out[0].split(), float).any() and int(out[1]) == 0


@pytest.mark.parametrize("name", list(cases.ALIGN_CASES))
def test_loop(emu, name):
    """align_turn over NdtRule on the host against the reference's loop, by the bounds the device is held to"""
    c = cases.ALIGN_CASES[name]()
    ref, best = cases.reference(name)
    g = c["guesses"]
    out = emu(5, "\n".join([_prm(c["prm"]), _pts(c["target"]), _pts(c["source"]), _align_prm(**c["solve"]), str(len(g))] + [_f(x) for x in g]))
    for k, r in enumerate(ref):
        head, ints, info = np.array(out[3 * k].split(), float), [int(v) for v in out[3 * k + 1].split()], np.array(out[3 * k + 2].split(), float)
        assert ints == [r["n_in"], r["status"], r["accepted"], r["rejected"]], (k, ints)
        assert nr.pose_distance(head[:7], r["pose"]) <= 1e-8 and abs(head[7] - r["score"]) <= 1e-9 * r["score"]
        assert np.abs(info - r["info"]).max() <= 1e-9 * np.abs(r["info"]).max()
        assert head[8] == pytest.approx(r["last_step"], rel=1e-6, abs=1e-12) and head[9] == pytest.approx(r["lambda"], rel=1e-12)
    assert tuple(int(v) for v in out[-1].split()) == best


def test_loop_edges(emu):
    c = cases.corner_near()
    far = np.array([500.0, 0, 0, 0, 0, 0, 1])
    g = [c["guesses"][0], far]
    text = lambda **kw: "\n".join([_prm(c["prm"]), _pts(c["target"]), _pts(c["source"]), _align_prm(**dict(c["solve"], **kw)), "2"] + [_f(x) for x in g])
    out = emu(5, text(max_iterations=0))      # only scores the guesses
    acc, n_in = nr.evaluate(c["prm"], cases.target("corner-near"), c["source"], g[0], 7, cases.D2)
    head = np.array(out[0].split(), float)
    assert np.array_equal(head[:7], g[0]) and abs(head[7] - acc[27]) <= TOL * acc[27] and out[1] == f"{n_in} {nr.MAX_ITERATIONS} 0 0"
    assert np.array_equal(np.array(out[3].split(), float)[:7], far) and out[4] == f"0 {nr.NO_OVERLAP} 0 0" and out[-1] == f"0 {n_in}"
    out = emu(5, "\n".join([_prm(c["prm"]), _pts(c["target"]), _pts(c["source"]), _align_prm(**c["solve"]), "1", _f(far)]))
    assert out[1] == f"0 {nr.NO_OVERLAP} 0 0" and out[-1] == "-1 -1"


def test_loop_takes_a_trial_without_overlap(emu):
    """NDT asks one point of the guess and NOTHING of a trial: with the score underflowed to 0 a trial that lost every point is
    taken (S = 0 >= 0).  One used voxel; one source point 2 km out on the sensor's x axis, half a metre off the voxel's mean and
    1 mm inside its face: exp(-0.5 d2 e' Omega e) is 0 at d2 = 10, so S, g and H are 0 and the step is 0.  The guess' quaternion is a
    quarter turn about z of norm 1 + 5e-7: R(q) stretches by |q|^2, the retraction renormalises, and the point moves 2 mm across
    the face into an empty voxel.  (A loop that asked one point of a trial too would reject it five times: MAX_ITERATIONS,
    accepted = 0, n_in = 1.)"""
    prm = nr.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=4, ny=4, nz=4)
    target = (np.array([1.5, 1.5, 1.5]) + np.random.default_rng(3).uniform(-0.01, 0.01, (8, 3))).astype(np.float32)
    src = np.array([[2048.0, 0.0, 0.0]], np.float32)
    q = (1.0 + 5e-7) * np.array([0.0, 0.0, math.sqrt(0.5), math.sqrt(0.5)])
    guess = np.concatenate([np.array([1.999, 1.5, 1.5]) - gr.rot(q) @ src[0].astype(float), q])
    solve = dict(search=1, d2=10.0, max_iterations=5)
    T = nr.build(prm, target)
    acc, n_in = nr.evaluate(prm, T, src, guess, 1, 10.0)
    assert n_in == 1 and not acc.any()
    r = nr.align_one(prm, T, src, guess, **solve)
    assert (r["status"], r["accepted"], r["rejected"], r["n_in"], r["score"]) == (nr.CONVERGED, 1, 0, 0, 0.0)
    assert nr.evaluate(prm, T, src, r["pose"], 1, 10.0)[1] == 0 and not np.array_equal(r["pose"], guess)
    out = emu(1, "\n".join([_prm(prm), _pts(target), _pts(src), _f(guess), "1 10.0"]))
    assert not np.array(out[0].split(), float).any() and int(out[1]) == 1
    out = emu(5, "\n".join([_prm(prm), _pts(target), _pts(src), _align_prm(**solve), "1", _f(guess)]))
    head = np.array(out[0].split(), float)
    assert [int(v) for v in out[1].split()] == [0, nr.CONVERGED, 1, 0]
    assert nr.pose_distance(head[:7], r["pose"]) <= 1e-8 and not np.array_equal(head[:7], guess)
    assert head[7] == 0.0 and head[8] == 0.0 and head[9] == pytest.approx(r["lambda"], rel=1e-12)
    assert not np.array(out[2].split(), float).any() and out[-1] == "0 0"


def test_params_rule(emu):
    P = cases.ROOM
    bad = [dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=math.inf), dict(resolution=math.nan), dict(origin=(0, math.nan, 0)),
           dict(origin=(math.inf, 0, 0)), dict(nx=0), dict(ny=1025), dict(nz=0), dict(nx=1024, ny=1024, nz=5), dict(min_points=1),
           dict(min_points=(1 << 20) + 1), dict(reg=-1e-9), dict(reg=1.0000001), dict(reg=math.nan)]
    good = [dict(), dict(nx=1024, ny=1024, nz=4), dict(nx=1, ny=1, nz=1), dict(min_points=2), dict(min_points=1 << 20), dict(reg=0.0), dict(reg=1.0)]
    out = emu(2, f"{len(bad) + len(good)}\n" + "\n".join(_prm(dict(P, **kw)) for kw in bad + good))
    assert all(o.startswith("bad: ") for o in out[:len(bad)]), out
    assert out[len(bad):] == ["ok"] * len(good)
    for o, what in zip(out, ["resolution"] * 4 + ["origin"] * 2 + ["nx, ny, nz"] * 3 + ["2^22"] + ["min_points"] * 2 + ["reg"] * 3):
        assert what in o, (o, what)


def test_align_params_rule(emu):
    bad = [dict(search=0), dict(search=2), dict(search=27), dict(max_iterations=-1), dict(max_iterations=1001), dict(d2=0.0), dict(d2=-1.0),
           dict(d2=math.inf), dict(d2=math.nan), dict(step_tol=-1e-12), dict(step_tol=math.inf), dict(lambda_min=0.0), dict(lambda_init=1e-11),
           dict(lambda_init=1e9), dict(lambda_max=math.inf), dict(lambda_min=math.nan)]
    good = [dict(), dict(search=1), dict(max_iterations=0), dict(max_iterations=1000), dict(step_tol=0.0), dict(lambda_init=1e-10), dict(lambda_init=1e8)]
    out = emu(3, f"{len(bad) + len(good)}\n" + "\n".join(_align_prm(**kw) for kw in bad + good))
    assert all(o.startswith("bad: ") for o in out[:len(bad)]), out
    assert out[len(bad):] == ["ok"] * len(good)
    for o, what in zip(out, ["search"] * 3 + ["max_iterations"] * 2 + ["d2"] * 4 + ["step_tol"] * 2 + ["lambda"] * 5):
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
    out = emu(4, f"{len(rows)}\n" + "\n".join(r for r, _ in rows))
    for o, (_, want) in zip(out, rows):
        assert (o == "ok") if want == "ok" else (o.startswith("bad: ") and want in o), (o, want)
