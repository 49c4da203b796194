"""lv_graph_* (include/limovelo_hip.h "Pose graph") on the GPU, through capi, against tests/graph_ref.py on the graphs of
tests/graph_cases.py.  "Dense" is the reference's Gauss-Newton answer from the same start; distance is the max over nodes of |dt|
and |Log(Ra^T Rb)|.  Solver runs use step_tol = 1e-10 and allow 100 iterations unless stated.

The 1e-9 bounds are the issue's: the reference's own Levenberg-Marquardt loop with the conjugate-gradient inner solve sits 2e-14
to 2e-12 from dense on these graphs (tests/test_graph_ref.py asserts it).  The Huber bound is not fixed in advance: the reference
loop runs on the test's own graph and the device has to come within ten times its distance from dense (the factor covers the other
summation order and the other stopping point of the conjugate gradients)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import graph_cases as cases
import graph_ref as gr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
EPS = 2.0 ** -52
# the reference loop's distance from dense on huber40, measured: 6.5e-10 (169 accepted steps); the test measures it again
HUBER_FACTOR = 10.0


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def ctx(capi):
    with capi.Context() as c:
        yield c


def _set(ctx, g):
    ctx.graph_set(g["poses"], g["fixed"], g["edges"], g["priors"])


def _solve(ctx, g, **kw):
    _set(ctx, g)
    info = ctx.graph_optimise(**dict(cases.SOLVE, **kw))
    return ctx.graph_fetch(), info


def test_two_nodes(ctx, capi):
    g, want = cases.two()
    x, info = _solve(ctx, g)
    assert info["status"] == capi.GRAPH_CONVERGED and info["n"] == 2 and info["n_edges"] == 1 and info["n_fixed"] == 1
    assert np.array_equal(x[0], g["poses"][0])   # the fixed node: not a bit moves
    d = gr.distance(x[1:], want)
    print("two: distance", d, info)
    assert d <= 1e-9


def test_exact_ring(ctx, capi):
    g, truth = cases.ring12()
    x, info = _solve(ctx, g)
    d = gr.distance(x, truth)
    print("ring12: distance from the truth", d, info)
    assert info["status"] == capi.GRAPH_CONVERGED and d <= 1e-9 and info["final_cost"] <= 1e-18


def _stepwise(ctx, capi, g, **kw):
    """The same loop one iteration per call (lambda handed on): the cost after every iteration"""
    _set(ctx, g)
    prm = dict(cases.SOLVE, **kw)
    lam, costs, accepted, status = capi.default_graph_params().lambda_init, [], [], capi.GRAPH_MAX_ITERATIONS
    for _ in range(prm["max_iterations"]):
        info = ctx.graph_optimise(**dict(prm, max_iterations=1, lambda_init=lam))
        if not costs:
            costs.append(info["initial_cost"])
        lam = info["lambda"]
        if info["accepted"]:
            costs.append(info["final_cost"])
        status = info["status"]
        if status == capi.GRAPH_CONVERGED:
            break
    return ctx.graph_fetch(), costs, status


@pytest.mark.parametrize("name", list(cases.CASES))
def test_against_dense(ctx, capi, name):
    """Tests 3 and 4: converged, the cost never rises across accepted steps (beyond the acceptance slack of the rule), cost and
    poses within 1e-9 of dense."""
    g = cases.CASES[name]()[0]
    xd, cd = cases.dense(name)
    x, info = _solve(ctx, g)
    d, rel = gr.distance(x, xd), abs(info["final_cost"] - cd) / cd
    print(name, "distance", d, "relative cost", rel, info)
    assert info["status"] == capi.GRAPH_CONVERGED
    lists = np.bincount(np.concatenate([g["edges"]["i"], g["edges"]["j"], g["priors"]["i"]]), minlength=len(g["poses"]))
    assert info["longest_list"] == lists.max() and (name != "ring67-long" or lists[0] > 128)
    assert rel <= 1e-9 and d <= 1e-9
    xs, costs, status = _stepwise(ctx, capi, g)
    assert status == capi.GRAPH_CONVERGED and len(costs) == info["accepted"] + 1
    assert all(b <= a + 64 * EPS * abs(a) for a, b in zip(costs, costs[1:])), costs
    assert costs[0] == info["initial_cost"] and costs[-1] == info["final_cost"]
    assert np.array_equal(xs, x)   # one iteration per call is the same loop


def test_ring300(ctx, capi):
    """More than one workgroup of nodes, a dot product over several partials: converged, and the cost within 1e-9 of dense."""
    g = cases.ring300()[0]
    xd, cd = cases.dense("ring300")
    x, info = _solve(ctx, g)
    rel = abs(info["final_cost"] - cd) / cd
    print("ring300: relative cost", rel, "distance", gr.distance(x, xd), info)
    assert info["status"] == capi.GRAPH_CONVERGED and rel <= 1e-9


@functools.lru_cache(maxsize=None)
def _huber_reference():
    g = cases.huber40()[0]
    xd, _ = cases.dense("huber40")
    x, info = gr.lm(g, inner="pcg", step_tol=1e-10, max_iterations=400)
    return gr.distance(x, xd), info


def test_huber(ctx, capi):
    g, truth = cases.huber40()
    xd, cd = cases.dense("huber40")
    ref_d, ref_info = _huber_reference()
    x, info = _solve(ctx, g, max_iterations=400)
    d, rel = gr.distance(x, xd), abs(info["final_cost"] - cd) / cd
    print("huber: device", d, "reference", ref_d, "relative cost", rel, info, ref_info["accepted"])
    assert d <= HUBER_FACTOR * ref_d and rel <= 1e-9
    es, _ = ctx.graph_chi2()
    assert int(np.argmax(es)) == len(es) - 1        # lv_graph_chi2 ranks the false edge first
    res, _ = gr.chi2(g, x)
    assert np.allclose(es, res, rtol=1e-9, atol=1e-12)
    # without Huber the same graph ends more than 1 m further from the truth
    gp = cases.huber40(0.0)[0]
    xp, infop = _solve(ctx, gp)
    assert infop["status"] == capi.GRAPH_CONVERGED and gr.distance(xp, cases.dense("plain40")[0]) <= 1e-9
    far, near = gr.distance(xp, truth), gr.distance(x, truth)
    print("huber: from the truth", near, "without", far)
    assert far > near + 1.0


def test_two_runs_give_equal_bytes(ctx):
    g = cases.ring67()[0]
    runs = []
    for _ in range(2):
        x, info = _solve(ctx, g)
        es, ps = ctx.graph_chi2()
        runs.append((x.tobytes(), repr(sorted(info.items())), es.tobytes(), ps.tobytes()))
    assert runs[0] == runs[1]


def test_max_iterations(ctx, capi):
    g = cases.ring40("fixed")[0]
    x1, info = _solve(ctx, g, max_iterations=1)
    assert info["status"] == capi.GRAPH_MAX_ITERATIONS and info["accepted"] + info["rejected"] == 1
    # the one-step poses: the reference's first step (the same rule; the conjugate gradients stop at the same tolerance)
    xr, ir = gr.lm(g, inner="pcg", step_tol=1e-10, max_iterations=1)
    assert ir["accepted"] == info["accepted"] == 1
    moved, off = gr.distance(x1, g["poses"]), gr.distance(x1, xr)
    print("one step: moved", moved, "from the reference's step", off)
    assert moved > 1e-3 and off <= 1e-6 * moved
    assert abs(info["final_cost"] - ir["final_cost"]) <= 1e-6 * ir["final_cost"]
    assert ctx.graph_info()["status"] == capi.GRAPH_MAX_ITERATIONS


def _warp_ref(now, x0, pts, keys):
    out = np.empty((len(pts), 3), np.float32)
    for k in set(keys.tolist()):
        DR = gr.rot(now[k, 3:]) @ gr.rot(x0[k, 3:]).T
        Dt = now[k, :3] - DR @ x0[k, :3]
        m = keys == k
        out[m] = (pts[m].astype(np.float64) @ DR.T + Dt).astype(np.float32)
    return out


def test_warp_points(ctx, capi):
    g = cases.ring40("fixed")[0]
    n = len(g["poses"])
    rng = np.random.default_rng(9)
    pts = rng.uniform(-20, 20, (1000, 3)).astype(np.float32)
    keys = rng.integers(0, n, 1000).astype(np.uint32)
    keys[:4] = [0, n - 1, 0, n - 1]
    _set(ctx, g)
    assert np.array_equal(ctx.graph_warp_points(pts, keys), pts)    # no optimise has run: the identity, exactly (a node equal to its x0)
    x, _ = _solve(ctx, g)
    got = ctx.graph_warp_points(pts, keys)
    want = _warp_ref(x, g["poses"], pts, keys)
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(got - want) <= ulp), float(np.max(np.abs(got - want) / ulp))
    assert np.max(np.abs(got - pts)) > 1e-3                          # (the correction is not nothing)
    wide = np.zeros((1000, 5), np.float32)                          # a stride of 20 bytes
    wide[:, :3] = pts
    assert np.array_equal(ctx.graph_warp_points(wide, keys), got)
    bad = keys.copy()
    bad[500] = n
    out = np.full((1000, 3), 7.0, np.float32)
    rc = ctx.lib.lv_graph_warp_points(ctx.h, pts.ctypes.data_as(C.c_void_p), 12, bad.ctypes.data_as(C.POINTER(C.c_uint32)), 1000,
                                      out.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == LV_EINVAL and "key 500" in ctx.lib.lv_last_error().decode() and np.all(out == 7.0)


def test_states_and_refusals(capi):
    g = cases.ring12()[0]
    with capi.Context() as c:
        info = capi.GraphInfo()
        assert c.lib.lv_graph_get_info(c.h, C.byref(info)) == LV_OK and info.set == 0 and info.status == -1
        buf = np.zeros((12, 7))
        s = np.zeros(12)
        pts, keys, out = np.zeros((1, 3), np.float32), np.zeros(1, np.uint32), np.zeros((1, 3), np.float32)
        calls = lambda: (c.lib.lv_graph_optimise(c.h, None, None), c.lib.lv_graph_fetch(c.h, buf.ctypes.data_as(C.POINTER(capi.GraphPose)), 12),
                         c.lib.lv_graph_chi2(c.h, s.ctypes.data_as(C.POINTER(C.c_double)), None),
                         c.lib.lv_graph_warp_points(c.h, pts.ctypes.data_as(C.c_void_p), 12, keys.ctypes.data_as(C.POINTER(C.c_uint32)), 1,
                                                    out.ctypes.data_as(C.POINTER(C.c_float))), c.lib.lv_graph_clear(c.h))
        assert calls() == (LV_ESTATE,) * 5 and "lv_graph_set" in c.lib.lv_last_error().decode()
        _set(c, g)
        first = c.graph_fetch()
        assert np.array_equal(first, g["poses"]) and c.graph_info()["set"] == 1
        # a rejected set writes nothing: the graph held stays bit for bit
        bad = g["edges"].copy()
        bad[3]["j"] = 12
        with pytest.raises(capi.LvError, match="edge 3: j"):
            c.graph_set(g["poses"], g["fixed"], bad, g["priors"])
        with pytest.raises(capi.LvError, match="neither a fixed node nor a prior"):
            c.graph_set(g["poses"], None, g["edges"], None)
        assert np.array_equal(c.graph_fetch(), first) and c.graph_info()["n_edges"] == 12
        assert c.lib.lv_graph_fetch(c.h, buf.ctypes.data_as(C.POINTER(capi.GraphPose)), 11) == LV_EINVAL
        with pytest.raises(capi.LvError, match="pcg_tol"):
            c.graph_optimise(pcg_tol=1.5)
        assert c.graph_optimise(**cases.SOLVE)["status"] == capi.GRAPH_CONVERGED
        c.graph_clear()
        assert calls() == (LV_ESTATE,) * 5 and c.graph_info()["set"] == 0
        # a graph with no factor at all: one fixed node and a free one nothing holds; the free one stays where it is
        c.graph_set(g["poses"][:2], [True, False], None, None)
        info = c.graph_optimise(**cases.SOLVE)
        assert info["status"] == capi.GRAPH_CONVERGED and info["final_cost"] == 0.0 and np.array_equal(c.graph_fetch(), g["poses"][:2])


def test_graph_py_end_to_end(ctx, capi):
    """limo_velo_amd.graph on records only (no scans: a scene with keyframe clouds and a map rebuild is exercised by
    test_rebuild_map below): a drifted loop of keyframes, odometry edges from the drifted states, one loop edge from the true
    relative pose, optimise; against the reference on the same records."""
    from limo_velo_amd import graph as pg, synth

    truth = gr.circle(24)
    g0, _ = gr.ring(24, seed=24, noise=False, drift=(0.03, 0.004), ring_closed=False)
    states = [synth.make_state(p[:3], p[3:]) for p in g0["poses"]]
    G = pg.PoseGraph()
    for s in states:
        G.add_keyframe(s, sigma_t=0.05, sigma_r=0.01)
    x_true0, x_true_last = synth.make_state(truth[0, :3], truth[0, 3:]), synth.make_state(truth[-1, :3], truth[-1, 3:])
    G.add_loop(23, 0, x_true_last, x_true0, sigma_t=0.01, sigma_r=0.002)
    info = G.optimise(ctx, **cases.SOLVE)
    assert info["status"] == capi.GRAPH_CONVERGED
    poses, fixed, edges, priors = G.records()
    xr, _ = gr.dense_gn(gr.make_graph(poses, fixed, edges, priors))
    got = np.array([np.concatenate([s[:3], s[3:7]]) for s in G.corrected_states()])
    assert gr.distance(got, xr) <= 1e-9
    # the loop is closed: the last keyframe is nearer to its true place than the drifted one was
    before, after = np.linalg.norm(g0["poses"][-1, :3] - truth[-1, :3]), np.linalg.norm(got[-1, :3] - truth[-1, :3])
    print("graph.py: last keyframe", before, "->", after)
    assert after < 0.5 * before
    t, q = pg.relative(x_true_last, x_true0)
    tr, qr = gr.relative(truth[-1], truth[0])
    assert np.allclose(t, tr, atol=1e-12) and np.allclose(q, qr, atol=1e-12)


def test_rebuild_map(ctx, capi):
    """rebuild_map: body-frame keyframe clouds of one wall seen on both passes of a drifted loop.  After the optimise the rebuilt
    map's points of the revisit lie nearer to the first pass's points than before."""
    from limo_velo_amd import graph as pg, synth

    truth = gr.circle(24)
    g0, _ = gr.ring(24, seed=24, noise=False, drift=(0.03, 0.004), ring_closed=False)
    rng = np.random.default_rng(5)
    wall = np.column_stack([rng.uniform(11.5, 12.5, 400), rng.uniform(-2, 2, 400), rng.uniform(0, 2, 400)])   # beside keyframes 0 and 23

    def body(k):
        return ((wall - truth[k, :3]) @ gr.rot(truth[k, 3:])).astype(np.float32)

    scans = {0: body(0), 23: body(23)}
    G = pg.PoseGraph()
    for p in g0["poses"]:
        G.add_keyframe(synth.make_state(p[:3], p[3:]), sigma_t=0.05, sigma_r=0.01)
    G.add_loop(23, 0, synth.make_state(truth[23, :3], truth[23, 3:]), synth.make_state(truth[0, :3], truth[0, 3:]), sigma_t=0.01, sigma_r=0.002)

    def gap(poses):
        a = scans[0].astype(np.float64) @ gr.rot(poses[0, 3:]).T + poses[0, :3]
        b = scans[23].astype(np.float64) @ gr.rot(poses[23, 3:]).T + poses[23, :3]
        return float(np.max(np.linalg.norm(a - b, axis=1)))

    before = gap(g0["poses"])
    G.optimise(ctx, **cases.SOLVE)
    world = G.rebuild_map(ctx, scans)
    got = np.array([np.concatenate([s[:3], s[3:7]]) for s in G.corrected_states()])
    after = gap(got)
    print("rebuild_map: revisit gap", before, "->", after)
    assert after < 0.1 * before and before > 0.3
    # what was handed to lv_map_build: the body clouds at the corrected poses (f32 rounding of the warp and of the start)
    want = np.concatenate([scans[k].astype(np.float64) @ gr.rot(got[k, 3:]).T + got[k, :3] for k in (0, 23)])
    assert world.shape == want.shape and np.max(np.abs(world - want)) <= 1e-4
    assert ctx.lib.lv_map_size(ctx.h) > 0
