"""The graphs of the pose-graph tests (include/limovelo_hip.h "Pose graph"), built once by tests/graph_ref.py's seeded generator and
shared by tests/test_graph_ref.py and tests/test_gpu_graph.py together with their dense Gauss-Newton answers."""
import functools
import math

import numpy as np

import graph_ref as gr

SOLVE = dict(step_tol=1e-10, max_iterations=100)


def _fix(g, *nodes):
    g["fixed"][list(nodes)] = True
    return g


def _full_prior(truth, k, sigma_t=0.01, sigma_r=0.002):
    W = np.diag([1 / sigma_t ** 2] * 3 + [1 / sigma_r ** 2] * 3)
    return np.array([gr.prior_record(k, truth[k, :3], truth[k, 3:], [0, 0, 0], W)], gr.PRIOR_DTYPE)


@functools.lru_cache(maxsize=None)
def two():
    """N = 2, one edge, node 0 fixed; the answer is T0 Z"""
    a = np.concatenate([[1.0, -2.0, 0.5], gr.quat_rpy(0.1, -0.2, 0.7)])
    t, q = np.array([2.0, 0.3, -0.1]), gr.quat_rpy(-0.05, 0.1, 0.4)
    b = gr.compose(a, t + np.array([0.4, -0.3, 0.2]), gr.qmul(q, gr.qexp([0.1, -0.2, 0.3])))   # a start off the answer
    g = gr.make_graph(np.array([a, b]), [True, False], np.array([gr.edge_record(0, 1, t, q, gr.random_info(np.random.default_rng(1), 0.05, 0.01))], gr.EDGE_DTYPE))
    return g, gr.compose(a, t, q)[None]


@functools.lru_cache(maxsize=None)
def ring12():
    """N = 12 ring, exact measurements, drifted start, node 0 fixed; the answer is the truth"""
    g, truth = gr.ring(12, seed=12, noise=False, drift=(0.05, 0.01))
    return _fix(g, 0), truth


@functools.lru_cache(maxsize=None)
def ring40(gauge="fixed"):
    """N = 40 noisy ring + 4 loops; gauge "fixed": node 0 fixed; "prior": nothing fixed, a full prior on node 0"""
    g, truth = gr.ring(40, seed=40, loops=4)
    if gauge == "fixed":
        return _fix(g, 0), truth
    g["priors"] = _full_prior(truth, 0)
    return g, truth


@functools.lru_cache(maxsize=None)
def ring67():
    """N = 67 + 5 loops + 130 extra edges on node 0 (duplicate pairs, i > j): a list longer than two wavefronts on a free node
    (the gauge is a full prior on node 0, so node 0 takes increments and its list is walked)"""
    g, truth = gr.ring(67, seed=67, loops=5)
    rng = np.random.default_rng(670)
    extra = []
    for k in range(130):
        other = 1 + (k * 7) % 33                       # 33 partners, each about four times
        i, j = (other, 0) if k % 2 else (0, other)     # half of them with i > j
        t, q = gr.relative(truth[i], truth[j])
        q = gr.qmul(q, gr.qexp(rng.normal(0, 0.004, 3)))
        extra.append(gr.edge_record(i, j, t + rng.normal(0, 0.02, 3), q / math.sqrt(q @ q), gr.random_info(rng, 0.02, 0.004)))
    g["edges"] = np.concatenate([g["edges"], np.array(extra, gr.EDGE_DTYPE)])
    g["priors"] = _full_prior(truth, 0)
    return g, truth


@functools.lru_cache(maxsize=None)
def gps40():
    """N = 40, nothing fixed, GPS priors on every third node: position rows only, lever arm (0.3, 0.1, 0.8), sigma 0.2 / 0.2 / 0.5"""
    g, truth = gr.ring(40, seed=41, loops=4)
    g["priors"] = gr.gps_priors(truth, range(0, 40, 3), rng=np.random.default_rng(410))
    return g, truth


@functools.lru_cache(maxsize=None)
def ring300():
    g, truth = gr.ring(300, seed=300, sigma_t=0.01, sigma_r=0.002, drift=(0.002, 0.0003))
    return _fix(g, 0), truth


@functools.lru_cache(maxsize=None)
def huber40(huber=1.0):
    """The N = 40 graph plus one false loop edge (3 m, 0.4 rad off), the given huber on every edge"""
    g, truth = gr.ring(40, seed=40, loops=4, huber=huber)
    t, q = gr.relative(truth[10], truth[30])
    false = gr.edge_record(10, 30, t + np.array([3.0, 0.0, 0.0]), gr.qmul(q, gr.qexp([0.0, 0.0, 0.4])), gr.random_info(np.random.default_rng(7), 0.02, 0.004), huber)
    g["edges"] = np.concatenate([g["edges"], np.array([false], gr.EDGE_DTYPE)])
    return _fix(g, 0), truth


CASES = {"ring40-fixed": lambda: ring40("fixed"), "ring40-prior": lambda: ring40("prior"), "ring67-long": ring67, "gps40": gps40}


@functools.lru_cache(maxsize=None)
def dense(name):
    """(poses, cost) of the dense Gauss-Newton answer from the graph's own start"""
    g = {"two": two, "ring12": ring12, "ring300": ring300, "huber40": huber40, "plain40": lambda: huber40(0.0), **CASES}[name]()[0]
    return gr.dense_gn(g, iterations=3000 if name == "huber40" else 300)
