"""tests/graph_ref.py against itself: its Jacobians against central differences of its residuals, and its Levenberg-Marquardt loop
(conjugate-gradient inner solve, the loop the device runs) against its dense Gauss-Newton answer on the graphs of
tests/graph_cases.py.  The 300-node ring is left to the GPU test: the numpy loop needs 15 s for it (measured once: converged after
16 iterations and 14072 conjugate-gradient iterations, 3e-12 from dense, cost 2e-14 relative)."""
import math

import numpy as np
import pytest

import graph_cases as cases
import graph_ref as gr


def _numeric(f, x, k, h=1e-6):
    """d f / d (increment k of pose x) by central differences"""
    d = np.zeros(6)
    d[k] = h
    return (f(gr.retract(x, d)) - f(gr.retract(x, -d))) / (2 * h)


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(0)
    worst = 0.0
    for th in (1e-5, 0.3, 1.2, math.pi / 2, 2.6):
        q = rng.normal(size=4)
        xi = np.concatenate([rng.normal(0, 3, 3), q / np.linalg.norm(q)])
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        t, qz = rng.normal(0, 2, 3), gr.qexp(rng.normal(0, 1, 3))
        xj = gr.compose(xi, t + rng.normal(0, 0.1, 3), gr.qmul(qz, gr.qexp(th * axis)))
        e = gr.edge_record(0, 1, t, qz, np.eye(6))
        r = gr.edge_residual(xi, xj, e)
        assert abs(np.linalg.norm(r[3:]) - th) < 1e-9
        Ji, Jj = gr.edge_jacobians(xi, xj, r)
        for k in range(6):
            worst = max(worst, np.abs(_numeric(lambda x: gr.edge_residual(x, xj, e), xi, k) - Ji[:, k]).max(),
                        np.abs(_numeric(lambda x: gr.edge_residual(xi, x, e), xj, k) - Jj[:, k]).max())
        p = gr.prior_record(0, xi[:3] + rng.normal(0, 0.2, 3), gr.qmul(xi[3:], gr.qexp(-th * axis)), [0.3, 0.1, 0.8], np.eye(6))
        rp = gr.prior_residual(xi, p)
        Jp = gr.prior_jacobian(xi, p, rp)
        for k in range(6):
            worst = max(worst, np.abs(_numeric(lambda x: gr.prior_residual(x, p), xi, k) - Jp[:, k]).max())
    print("worst Jacobian difference", worst)
    assert worst < 2e-9   # central differences at h = 1e-6: h^2 truncation and eps / h rounding, both about 1e-10 here


def test_series_switch_is_smooth():
    a, b = gr.jrinv(np.array([0.99999e-4, 0, 0])), gr.jrinv(np.array([1.00001e-4, 0, 0]))
    assert np.abs(a - b).max() < 1e-9   # (the closed form loses digits below the switch: c ~ 1/12 from a difference of 1e8-sized terms)


def test_huber_and_packing():
    assert gr.rho_w(4.0, 0.0) == (4.0, 1.0) and gr.rho_w(4.0, 2.0) == (4.0, 1.0)
    rho, w = gr.rho_w(9.0, 2.0)
    assert rho == 2 * 2 * 3 - 4 and w == 2.0 / 3.0
    M = np.arange(36.0).reshape(6, 6)
    M = M + M.T
    u = gr.info21(M)
    assert list(u[:7]) == [M[0, 0], M[0, 1], M[0, 2], M[0, 3], M[0, 4], M[0, 5], M[1, 1]] and np.array_equal(gr.info_full(u), M)


def test_two_and_exact_ring():
    g, want = cases.two()
    x, info = gr.lm(g, **cases.SOLVE)
    assert info["status"] == gr.CONVERGED and gr.distance(x[1:], want) <= 1e-9
    g, truth = cases.ring12()
    x, info = gr.lm(g, **cases.SOLVE)
    assert info["status"] == gr.CONVERGED and gr.distance(x, truth) <= 1e-9


@pytest.mark.parametrize("name", list(cases.CASES))
def test_lm_against_dense(name):
    g = cases.CASES[name]()[0]
    xd, cd = cases.dense(name)
    for inner in ("pcg", "dense"):
        x, info = gr.lm(g, inner=inner, **cases.SOLVE)
        d, rel = gr.distance(x, xd), abs(info["final_cost"] - cd) / cd
        print(name, inner, "distance", d, "relative cost", rel, info["accepted"], info["rejected"], info["pcg_iterations"])
        assert info["status"] == gr.CONVERGED and d <= 1e-10 and rel <= 1e-12
        c = [info["initial_cost"]] + info["costs"]
        assert all(gr.accept(b, a) for a, b in zip(c, c[1:]))


def test_gps_graph_is_held_by_positions_alone():
    g = cases.gps40()[0]
    assert not g["fixed"].any() and len(g["priors"]) == 14
    W = gr.info_full(g["priors"][0]["info"])
    assert np.all(W[3:, :] == 0) and np.all(W[:, 3:] == 0) and np.allclose(np.diag(W)[:3], [25, 25, 4])
    H, _, _ = gr.linearise(g, g["poses"])
    assert np.linalg.eigvalsh(H).min() > 0   # no gauge freedom left
