"""CPU checks of the pose-graph entry points (include/limovelo_hip.h "Pose graph"): the built library exports them, the ctypes
signatures and record layouts capi installs agree with the header (sizes and offsets against a compiled C program), the defaults,
and the refusals that need no GPU: lv_graph_set judges its records and lv_graph_optimise its parameters before the context, so a
null context shows every LV_EINVAL path; "null context" itself comes last.  (LV_ESTATE needs a context and so a GPU:
tests/test_gpu_graph.py::test_states_and_refusals.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_cases as cases
import graph_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_graph_params", "lv_graph_set", "lv_graph_optimise", "lv_graph_fetch", "lv_graph_chi2", "lv_graph_warp_points",
           "lv_graph_get_info", "lv_graph_clear")
LV_EINVAL = -1


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return c


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|void|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in limovelo_hip.h"
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_library_exports_the_symbols(capi):
    lib = capi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "void*": C.c_void_p, "size_t": C.c_size_t, "lv_graph_pose*": C.POINTER(capi.GraphPose),
             "lv_graph_edge*": C.POINTER(capi.GraphEdge), "lv_graph_prior*": C.POINTER(capi.GraphPrior),
             "lv_graph_params*": C.POINTER(capi.GraphParams), "lv_graph_info*": C.POINTER(capi.GraphInfo), "uint8_t*": C.POINTER(C.c_uint8),
             "uint32_t*": C.POINTER(C.c_uint32), "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float)}
    for name in SYMBOLS:
        rtype, params = _prototype(name)
        want = [table[re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")] for p in params]
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if rtype == "void" else C.c_int), name


def test_layouts_match_c(capi, tmp_path):
    records = {"lv_graph_pose": (capi.GraphPose, capi.GRAPH_POSE_DTYPE, 56), "lv_graph_edge": (capi.GraphEdge, capi.GRAPH_EDGE_DTYPE, 240),
               "lv_graph_prior": (capi.GraphPrior, capi.GRAPH_PRIOR_DTYPE, 264), "lv_graph_params": (capi.GraphParams, None, 48),
               "lv_graph_info": (capi.GraphInfo, None, 72)}
    exprs, want = [], []
    for cname, (ct, dt, size) in records.items():
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(ct))
        assert C.sizeof(ct) == size and (dt is None or dt.itemsize == size)
        for f, _ in ct._fields_:
            exprs.append(f"offsetof({cname}, {f.rstrip('_')})")
            want.append(getattr(ct, f).offset)
            if dt is not None:
                assert dt.fields[f][1] == getattr(ct, f).offset, (cname, f)
    assert gr.EDGE_DTYPE == capi.GRAPH_EDGE_DTYPE and gr.PRIOR_DTYPE == capi.GRAPH_PRIOR_DTYPE and gr.POSE_DTYPE == capi.GRAPH_POSE_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


def test_defaults(capi):
    p = capi.default_graph_params()
    got = {f: getattr(p, f) for f, _ in p._fields_}
    assert got == gr.DEFAULTS == dict(max_iterations=100, pcg_max_iterations=1000, pcg_tol=1e-2, step_tol=1e-8, lambda_init=1e-4,
                                      lambda_min=1e-10, lambda_max=1e8)
    assert capi.default_graph_params(step_tol=1e-10).step_tol == 1e-10
    assert (capi.GRAPH_CONVERGED, capi.GRAPH_MAX_ITERATIONS) == (gr.CONVERGED, gr.MAX_ITERATIONS) == (0, 1)


def _set(capi, g, fixed="given", n=None, n_edges=None, n_priors=None):
    lib = capi.load_library()
    x, e, p = np.ascontiguousarray(g["poses"]), np.ascontiguousarray(g["edges"]), np.ascontiguousarray(g["priors"])
    f = np.ascontiguousarray(g["fixed"].astype(np.uint8))
    rc = lib.lv_graph_set(None, x.ctypes.data_as(C.POINTER(capi.GraphPose)), len(x) if n is None else n,
                          None if fixed is None else f.ctypes.data_as(C.POINTER(C.c_uint8)),
                          e.ctypes.data_as(C.POINTER(capi.GraphEdge)) if len(e) else None, len(e) if n_edges is None else n_edges,
                          p.ctypes.data_as(C.POINTER(capi.GraphPrior)) if len(p) else None, len(p) if n_priors is None else n_priors)
    return rc, lib.lv_last_error().decode()


def test_set_judges_the_records_before_the_context(capi):
    g = cases.gps40()[0]
    rc, why = _set(capi, g)
    assert rc == LV_EINVAL and why == "null context"       # good records: only the context is missing
    n = len(g["poses"])

    def refused(change, *what, **kw):
        b = {k: v.copy() for k, v in g.items()}
        change(b)
        rc, why = _set(capi, b, **kw)
        assert rc == LV_EINVAL and all(w in why for w in what) and "null context" not in why, (what, why)

    refused(lambda b: b["edges"][5].__setitem__("i", n), "edge 5", "i =", "out of range")
    refused(lambda b: b["priors"][2].__setitem__("i", n), "prior 2", "i =", "out of range")
    refused(lambda b: b["edges"][4].__setitem__("j", int(b["edges"][4]["i"])), "edge 4", "i == j")
    refused(lambda b: b["poses"].__setitem__((9, 1), np.nan), "pose 9", "t:", "non-finite")
    refused(lambda b: b["edges"][8].__setitem__("q", b["edges"][8]["q"] * (1 - 2e-6)), "edge 8", "q:", "norm")
    refused(lambda b: b["edges"][3]["info"].__setitem__(6, -1e-12), "edge 3", "info", "negative diagonal")
    refused(lambda b: b["priors"][0].__setitem__("huber", -1.0), "prior 0", "huber")
    refused(lambda b: b["priors"][0].__setitem__("reserved", 1), "prior 0", "reserved")
    refused(lambda b: b.__setitem__("priors", b["priors"][:0]), "neither a fixed node nor a prior")
    refused(lambda b: None, "n = 0", n=0)
    refused(lambda b: None, "n = ", "2^20", n=(1 << 20) + 1)
    refused(lambda b: None, "n_edges", "2^22", n_edges=(1 << 22) + 1)
    refused(lambda b: None, "n_priors", "2^20", n_priors=(1 << 20) + 1)
    refused(lambda b: b.__setitem__("edges", b["edges"][:0]), "null edges", n_edges=3)


def test_other_calls_judge_their_arguments_before_the_context(capi):
    lib = capi.load_library()
    info = capi.GraphInfo()
    assert lib.lv_graph_optimise(None, None, C.byref(info)) == LV_EINVAL and lib.lv_last_error().decode() == "null context"
    for kw, what in ((dict(pcg_tol=1.0), "pcg_tol"), (dict(max_iterations=0), "max_iterations"), (dict(lambda_min=1.0), "lambda"),
                     (dict(step_tol=-1.0), "step_tol"), (dict(pcg_max_iterations=0), "pcg_max_iterations")):
        p = capi.default_graph_params(**kw)
        assert lib.lv_graph_optimise(None, C.byref(p), None) == LV_EINVAL and what in lib.lv_last_error().decode()
    assert lib.lv_graph_fetch(None, None, 4) == LV_EINVAL and "null poses" in lib.lv_last_error().decode()
    assert lib.lv_graph_get_info(None, None) == LV_EINVAL and "null info" in lib.lv_last_error().decode()
    pts, keys, out = np.zeros((2, 3), np.float32), np.zeros(2, np.uint32), np.zeros((2, 3), np.float32)
    P, K, O = pts.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.lv_graph_warp_points(None, P, 8, K, 2, O) == LV_EINVAL and "stride" in lib.lv_last_error().decode()
    assert lib.lv_graph_warp_points(None, P, 12, None, 2, O) == LV_EINVAL and "null argument" in lib.lv_last_error().decode()
    assert lib.lv_graph_warp_points(None, P, 12, K, (1 << 28) + 1, O) == LV_EINVAL and "2^28" in lib.lv_last_error().decode()
    for rc in (lib.lv_graph_warp_points(None, P, 12, K, 2, O), lib.lv_graph_chi2(None, None, None), lib.lv_graph_clear(None),
               lib.lv_graph_get_info(None, C.byref(info)), lib.lv_graph_fetch(None, pts.ctypes.data_as(C.POINTER(capi.GraphPose)), 0)):
        assert rc == LV_EINVAL and lib.lv_last_error().decode() == "null context"


def test_graph_py_records(capi):
    """limo_velo_amd.graph without a context: relative, the records a PoseGraph collects, and what vet drops (a fake context)."""
    from limo_velo_amd import graph as pg, synth

    truth = gr.circle(8)
    states = [synth.make_state(p[:3], p[3:]) for p in truth]
    G = pg.PoseGraph()
    for s in states:
        G.add_keyframe(s, sigma_t=0.1, sigma_r=0.02)
    G.add_loop(7, 0, states[7], states[0], sigma_t=0.01, sigma_r=0.002, huber=1.5)
    G.add_gps(3, [1.0, 2.0, 3.0], sigma=(0.2, 0.2, 0.5), lever=(0.3, 0.1, 0.8))
    poses, fixed, edges, priors = G.records()
    assert poses.shape == (8, 7) and not fixed.any() and len(edges) == 8 and len(priors) == 1
    for k, e in enumerate(edges):
        i, j = (k, k + 1) if k < 7 else (7, 0)
        t, q = gr.relative(truth[i], truth[j])
        assert (int(e["i"]), int(e["j"])) == (i, j) and np.allclose(e["t"], t, atol=1e-12) and np.allclose(e["q"], q, atol=1e-12)
    assert np.allclose(gr.info_full(edges[0]["info"]), np.diag([100.0] * 3 + [2500.0] * 3)) and edges[7]["huber"] == 1.5
    W = gr.info_full(priors[0]["info"])
    assert np.allclose(np.diag(W), [25, 25, 4, 0, 0, 0]) and list(priors[0]["lever"]) == [0.3, 0.1, 0.8] and int(priors[0]["i"]) == 3
    g = gr.make_graph(poses, fixed, edges, priors)
    assert gr.cost(g, poses) == pytest.approx(0.5 * gr.chi2(g, poses)[1][0])   # the edges are exact; only the GPS fix pulls
    H = pg.PoseGraph()
    H.add_keyframe(states[0])
    H.add_keyframe(states[1])
    assert list(H.records()[1]) == [True, False]       # nothing holds the graph: keyframe 0 is fixed

    class Fake:
        def __init__(self):
            self.sets = []

        def graph_set(self, poses, fixed, edges, priors):
            self.sets.append(len(edges))
            self.n = len(poses)

        def graph_optimise(self, **kw):
            return dict(status=0)

        def graph_fetch(self):
            return poses.copy()

        def graph_chi2(self):
            return np.array([0.1] * 7 + [50.0][:self.sets[-1] - 7]), np.zeros(1)

    f = Fake()
    dropped, info = G.vet(f, threshold=16.8)
    assert dropped == [7] and info == dict(status=0) and f.sets == [8, 7] and len(G.edges) == 7 and not any(G.is_loop)
    assert G.vet(f, threshold=16.8) == ([], None)
    assert np.array_equal(G.corrected_states()[2][:7], poses[2]) and np.array_equal(G.corrected_states()[2][7:], states[2][7:])
