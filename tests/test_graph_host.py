"""The rule of lv_graph.hpp (residuals, Jacobian blocks, Huber weight, retraction, block inverse, warp, argument rules, incidence
lists: what the kernels of lv_graph.hip run) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h
as a stand-alone program (tests/emu/graph_emu.cpp) and held to tests/graph_ref.py at 1e-9, the project's figure for f64 algebra
held to the oracle (libm differs between the two, so not by bits)."""
import math
import os
import subprocess

import numpy as np
import pytest

import graph_cases as cases
import graph_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
TOL = 1e-9


def _f(v):
    return " ".join(repr(float(x)) for x in np.asarray(v, float).reshape(-1))


def _edge_text(e):
    return f"{int(e['i'])} {int(e['j'])} {_f(e['t'])} {_f(e['q'])} {_f(e['info'])} {_f(e['huber'])}"


def _prior_text(p, reserved=None):
    head = f"{int(p['i'])}" + ("" if reserved is None else f" {reserved}")
    return f"{head} {_f(p['t'])} {_f(p['q'])} {_f(p['lever'])} {_f(p['info'])} {_f(p['huber'])}"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("graph_host") / "graph_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "graph_emu.cpp"), "-o", str(exe)])

    def run(mode, records):
        text = f"{mode} {len(records)}\n" + "\n".join(records) + "\n"
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().strip().split("\n")
        return out

    return run


def _close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))))


def _pose(rng, scale=5.0):
    q = rng.normal(size=4)
    return np.concatenate([rng.normal(0, scale, 3), q / np.linalg.norm(q)])


def _edge_with_rotation_residual(rng, th, huber=0.0, info=None):
    """(xi, xj, edge) whose rotation residual has norm th"""
    xi = _pose(rng)
    t, q = rng.normal(0, 2, 3), gr.qexp(rng.normal(0, 1, 3))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    xj = gr.compose(xi, t + rng.normal(0, 0.05, 3), gr.qmul(q, gr.qexp(th * axis)))
    W = gr.random_info(rng, 0.05, 0.02) if info is None else info
    return xi, xj, gr.edge_record(0, 1, t, q, W, huber)


def _semi_definite(rng):
    A = rng.normal(size=(3, 6))   # rank 3
    return A.T @ A


def _edge_cases():
    rng = np.random.default_rng(1)
    out = []
    for th in (0.0, 1e-7, 0.99e-4, 1.01e-4, 1e-3, 0.3, math.pi / 2 - 1e-3, math.pi / 2, math.pi / 2 + 1e-3, 2.5):
        out.append(_edge_with_rotation_residual(rng, th))
    # Huber on both sides of the knee: sqrt(s) of the plain edge is measured, the knee set just above and just below it
    for k in range(4):
        xi, xj, e = _edge_with_rotation_residual(rng, 0.2)
        s = gr.edge_lin(xi, xj, e)["s"]
        for f in (1.0 + 1e-6, 1.0 - 1e-6, 0.1, 10.0):
            h = e.copy()
            h["huber"] = f * math.sqrt(s)
            out.append((xi, xj, h))
    for k in range(4):
        out.append(_edge_with_rotation_residual(rng, 0.4, info=_semi_definite(rng)))
        out.append(_edge_with_rotation_residual(rng, 0.4, huber=0.5, info=_semi_definite(rng)))
    return out


def test_edges(emu):
    cs = _edge_cases()
    out = emu(0, [f"{_f(xi)} {_f(xj)} {_edge_text(e)}" for xi, xj, e in cs])
    assert len(out) == 3 * len(cs)
    weights = []
    for k, (xi, xj, e) in enumerate(cs):
        L = gr.edge_lin(xi, xj, e)
        r, head, lin = (np.array(out[3 * k + m].split(), float) for m in range(3))
        assert _close(r, L["r"]), (k, r, L["r"])
        assert _close(head, [L["s"], L["w"], L["rho"]]), (k, head)
        want = np.concatenate([L["Hii"].ravel(), L["Hjj"].ravel(), L["Hij"].ravel(), L["gi"], L["gj"]])
        scale = max(1.0, float(np.abs(want).max()))
        assert lin.shape == want.shape and np.abs(lin - want).max() <= TOL * scale, (k, np.abs(lin - want).max() / scale)
        weights.append(L["w"])
    assert any(w < 1.0 for w in weights) and sum(w == 1.0 for w in weights) > 10   # both sides of the knee were there


def test_priors(emu):
    rng = np.random.default_rng(2)
    cs = []
    for th in (0.0, 0.5e-4, 2e-4, 0.7, math.pi / 2, 3.0):
        xi = _pose(rng)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        qp = gr.qmul(xi[3:], gr.qexp(-th * axis))
        for W, huber in ((gr.random_info(rng, 0.1, 0.02), 0.0), (gr.random_info(rng, 0.1, 0.02), 0.3)):
            cs.append((xi, gr.prior_record(0, xi[:3] + rng.normal(0, 0.3, 3), qp, rng.normal(0, 0.5, 3), W, huber)))
    for xi, p in list(cs[:4]):   # a GPS fix: rotation rows and columns zero
        g = p.copy()
        W = gr.info_full(p["info"])
        W[3:, :] = 0
        W[:, 3:] = 0
        g["info"] = gr.info21(W)
        cs.append((xi, g))
    out = emu(1, [f"{_f(xi)} {_prior_text(p)}" for xi, p in cs])
    for k, (xi, p) in enumerate(cs):
        L = gr.prior_lin(xi, p)
        r, head, lin = (np.array(out[3 * k + m].split(), float) for m in range(3))
        want = np.concatenate([L["Hii"].ravel(), L["gi"]])
        scale = max(1.0, float(np.abs(want).max()))
        assert _close(r, L["r"]) and _close(head, [L["s"], L["w"], L["rho"]]) and np.abs(lin - want).max() <= TOL * scale, k


def test_retract_inverse_and_warp(emu):
    rng = np.random.default_rng(3)
    xs = [_pose(rng) for _ in range(8)]
    ds = [np.concatenate([rng.normal(0, 1, 3), s * rng.normal(0, 1, 3)]) for s in (0.0, 1e-10, 1e-9, 1e-7, 1e-3, 0.1, 1.0, 2.0)]
    out = emu(2, [f"{_f(x)} {_f(d)}" for x, d in zip(xs, ds)])
    for k, (x, d) in enumerate(zip(xs, ds)):
        got = np.concatenate([np.array(out[2 * k].split(), float), np.array(out[2 * k + 1].split(), float)])
        assert _close(got, gr.retract(x, d)) and abs(np.linalg.norm(got[3:]) - 1.0) < 1e-15
    Ms = [gr.random_info(rng, 0.1, 0.02) for _ in range(4)]
    dead = Ms[0].copy()
    dead[3:, :] = 0
    dead[:, 3:] = 0                      # a GPS-only block: the rotation components do not move
    Ms.append(dead)
    Ms.append(np.zeros((6, 6)))          # a node nothing holds
    out = emu(3, [_f(M) for M in Ms])
    for k, M in enumerate(Ms):
        got = np.array(out[k].split(), float).reshape(6, 6)
        want = gr.block_inverse(M)
        assert np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max())
        if k < 4:
            assert np.abs(got @ M - np.eye(6)).max() < 1e-8
    assert np.all(np.array(out[4].split(), float).reshape(6, 6)[3:, :] == 0) and np.all(np.array(out[5].split(), float) == 0)
    # the warp: within one f32 ulp of the f64 reference, and the identity for a node that has not moved
    recs, want = [], []
    for _ in range(20):
        now, x0, p = _pose(rng, 20), _pose(rng, 20), rng.uniform(-30, 30, 3).astype(np.float32)
        DR = gr.rot(now[3:]) @ gr.rot(x0[3:]).T
        recs.append(f"{_f(now)} {_f(x0)} {_f(p)}")
        want.append((DR @ p.astype(float) + now[:3] - DR @ x0[:3]).astype(np.float32))
    x = _pose(rng, 20)
    p = rng.uniform(-30, 30, 3).astype(np.float32)
    recs.append(f"{_f(x)} {_f(x)} {_f(p)}")
    out = emu(4, recs)
    for k, w in enumerate(want):
        got = np.array(out[k].split(), np.float32)
        assert np.all(np.abs(got - w) <= np.spacing(np.abs(w))), k
    assert np.array_equal(np.array(out[-1].split(), np.float32), p)


def _check(emu, g, fixed="given", reserved=0):
    """graph_check (and, when it passes, graph_incidence) of one graph: mode 6, whose record list is the graph's lines"""
    lines = [str(len(g["poses"]))] + [_f(x) for x in g["poses"]]
    lines.append("0" if fixed is None else "1 " + " ".join(str(int(v)) for v in g["fixed"]))
    lines.append(str(len(g["edges"])))
    lines += [_edge_text(e) for e in g["edges"]]
    lines.append(str(len(g["priors"])))
    lines += [_prior_text(p, reserved) for p in g["priors"]]
    return emu(6, lines)


def _copy(g):
    return {k: v.copy() for k, v in g.items()}


def test_argument_rules_and_lists(emu):
    g = cases.gps40()[0]
    g = _copy(g)
    g["fixed"][7] = True
    out = _check(emu, g)
    assert out[0].startswith("ok ")
    n, ne, npr = len(g["poses"]), len(g["edges"]), len(g["priors"])
    start, items = np.array(out[1].split(), np.int64), np.array(out[2].split(), np.int64)
    assert len(start) == n + 1 and len(items) == 2 * ne + npr and start[0] == 0 and start[-1] == len(items)
    for k in range(n):   # edge id ascending (an edge in both its ends' lists), then priors
        want = [(e << 2) | (0 if int(g["edges"][e]["i"]) == k else 1) for e in range(ne) if k in (int(g["edges"][e]["i"]), int(g["edges"][e]["j"]))]
        want += [(p << 2) | 2 for p in range(npr) if int(g["priors"][p]["i"]) == k]
        assert list(items[start[k]:start[k + 1]]) == want, k
    assert int(out[0].split()[1]) == int(np.diff(start).max())

    def refused(change, what, **kw):
        b = _copy(g)
        change(b)
        o = _check(emu, b, **kw)
        assert o[0].startswith("bad: ") and all(w in o[0] for w in what), (what, o[0])

    def put(kind, k, field, value, idx=None):
        def f(b):
            if idx is None:
                b[kind][k][field] = value
            else:
                b[kind][k][field][idx] = value
        return f

    refused(put("edges", 5, "i", n), ("edge 5", "i =", "out of range"))
    refused(put("edges", 6, "j", n + 3), ("edge 6", "j =", "out of range"))
    refused(put("priors", 2, "i", n), ("prior 2", "i =", "out of range"))
    refused(put("edges", 4, "j", int(g["edges"][4]["i"])), ("edge 4", "i == j"))
    refused(lambda b: b["poses"].__setitem__((9, 1), np.nan), ("pose 9", "t:", "non-finite"))
    refused(lambda b: b["poses"].__setitem__((3, 5), np.inf), ("pose 3", "q:", "non-finite"))
    refused(put("edges", 1, "t", np.inf, 2), ("edge 1", "t:", "non-finite"))
    refused(put("edges", 1, "info", np.nan, 7), ("edge 1", "info", "non-finite"))
    refused(put("priors", 0, "lever", np.nan, 0), ("prior 0", "lever", "non-finite"))
    refused(put("edges", 2, "huber", np.nan), ("edge 2", "huber"))
    refused(lambda b: b["poses"].__setitem__((11, slice(3, 7)), b["poses"][11, 3:] * (1 + 2e-6)), ("pose 11", "q:", "norm"))
    refused(lambda b: b["edges"][8].__setitem__("q", b["edges"][8]["q"] * (1 - 2e-6)), ("edge 8", "q:", "norm"))
    refused(lambda b: b["priors"][1].__setitem__("q", np.array([0, 0, 0, 1.00001])), ("prior 1", "q:", "norm"))
    refused(put("edges", 3, "info", -1e-12, 6), ("edge 3", "info", "negative diagonal"))     # entry 6 is (1, 1)
    refused(put("priors", 3, "info", -1.0, 20), ("prior 3", "info", "negative diagonal"))   # entry 20 is (5, 5)
    refused(put("edges", 0, "huber", -0.5), ("edge 0", "huber"))
    refused(put("priors", 0, "huber", -1e-9), ("prior 0", "huber"))
    refused(lambda b: None, ("prior 0", "reserved"), reserved=1)

    def free_gauge(b):
        b["priors"] = b["priors"][:0]
        b["fixed"][:] = False
    refused(free_gauge, ("neither a fixed node nor a prior",))
    refused(lambda b: b.__setitem__("priors", b["priors"][:0]) or b["fixed"].__setitem__(slice(None), False), ("neither",), fixed=None)
    # what is allowed: a norm off by just under 1e-6, a zero diagonal entry, a negative off-diagonal entry, no fixed array with priors
    ok = _copy(g)
    ok["poses"][11, 3:] *= 1 + 0.9e-6
    ok["edges"][3]["info"][6] = 0.0
    ok["edges"][3]["info"][1] = -5.0
    assert _check(emu, ok)[0].startswith("ok ") and _check(emu, ok, fixed=None)[0].startswith("ok ")


def test_params_rule(emu):
    d = gr.DEFAULTS
    order = ("max_iterations", "pcg_max_iterations", "pcg_tol", "step_tol", "lambda_init", "lambda_min", "lambda_max")

    def rec(**kw):
        p = dict(d, **kw)
        return " ".join(str(p[k]) if k.endswith("iterations") else repr(float(p[k])) for k in order)

    bad = [dict(max_iterations=0), dict(max_iterations=10001), dict(pcg_max_iterations=0), dict(pcg_max_iterations=100001), dict(pcg_tol=0.0),
           dict(pcg_tol=1.0), dict(pcg_tol=math.nan), dict(step_tol=-1e-12), dict(step_tol=math.inf), dict(lambda_min=0.0), dict(lambda_init=1e-11),
           dict(lambda_init=1e9), dict(lambda_max=math.inf), dict(lambda_min=math.nan)]
    good = [dict(), dict(max_iterations=1, pcg_max_iterations=1), dict(max_iterations=10000, pcg_max_iterations=100000), dict(step_tol=0.0),
            dict(lambda_init=1e-10), dict(lambda_init=1e8)]
    out = emu(5, [rec(**b) for b in bad] + [rec(**o) for o in good])
    assert all(o.startswith("bad: graph params: ") for o in out[:len(bad)]), out
    assert out[len(bad):] == ["ok"] * len(good)
