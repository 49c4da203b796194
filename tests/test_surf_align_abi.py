"""CPU checks of the surface-registration entry points (include/limovelo_hip.h "Surface registration"): the built library exports
them, the ctypes signatures and record layouts capi installs agree with the header (sizes and offsets against a compiled C
program), the defaults, and the refusals that need no GPU: both calls judge their parameters and their NULL or short arguments
before the context, so a null context shows every LV_EINVAL path; "null context" itself comes last.  (LV_ESTATE needs a context and
so a GPU: tests/test_gpu_surf_align.py::test_states.)  mesh.frame_points and mesh.align_params_for run on the host."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import surf_align_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_surf_align_params", "lv_surf_sample", "lv_surf_align")
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
    table = {"lv_ctx*": C.c_void_p, "void*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "lv_graph_pose*": C.POINTER(capi.GraphPose),
             "lv_surf_align_params*": C.POINTER(capi.SurfAlignParams), "lv_surf_align_result*": C.POINTER(capi.SurfAlignResult),
             "double*": C.POINTER(C.c_double), "uint8_t*": C.POINTER(C.c_uint8), "int32_t": C.POINTER(C.c_int32)}   # (the array: best[2])
    for name in SYMBOLS:
        rtype, params = _prototype(name)
        want = [table[re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*(\[\d+\])?$", "", p).replace("const ", "").replace(" ", "")] for p in params]
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if rtype == "void" else C.c_int), name


def test_layouts_match_c(capi, tmp_path):
    records = {"lv_surf_align_params": (capi.SurfAlignParams, None, 64), "lv_surf_align_result": (capi.SurfAlignResult, capi.SURF_ALIGN_RESULT_DTYPE, 264)}
    exprs, want = [], []
    for cname, (ct, dt, size) in records.items():
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(ct))
        assert C.sizeof(ct) == size and (dt is None or dt.itemsize == size)
        for f, _ in ct._fields_:
            exprs.append(f"offsetof({cname}, {f.rstrip('_')})")
            want.append(getattr(ct, f).offset)
            if dt is not None and f != "pose":
                assert dt.fields[f.rstrip("_")][1] == getattr(ct, f).offset, (cname, f)
    d = capi.SURF_ALIGN_RESULT_DTYPE
    assert d.fields["t"][1] == 0 and d.fields["q"][1] == 24
    # laid out as lv_ndt_result with cost for score: what takes the one takes the other
    assert [(n, d.fields[n][1]) for n in d.names if n != "cost"] == [(n, capi.NDT_RESULT_DTYPE.fields[n][1]) for n in capi.NDT_RESULT_DTYPE.names if n != "score"]
    assert d.fields["cost"][1] == capi.NDT_RESULT_DTYPE.fields["score"][1]
    consts = ("LV_SURF_SAMPLE_OUTSIDE", "LV_SURF_SAMPLE_UNKNOWN", "LV_SURF_SAMPLE_KNOWN", "LV_SURF_ALIGN_CONVERGED", "LV_SURF_ALIGN_MAX_ITERATIONS",
              "LV_SURF_ALIGN_NO_OVERLAP", "LV_SURF_ALIGN_CHUNK")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "".join(f'printf("%d\\n", {c});' for c in consts) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[:-7] == want
    assert out[-7:] == [capi.SURF_SAMPLE_OUTSIDE, capi.SURF_SAMPLE_UNKNOWN, capi.SURF_SAMPLE_KNOWN, capi.SURF_ALIGN_CONVERGED,
                        capi.SURF_ALIGN_MAX_ITERATIONS, capi.SURF_ALIGN_NO_OVERLAP, capi.SURF_ALIGN_CHUNK] == [0, 1, 2, 0, 1, 2, sr.CHUNK]
    assert (sr.OUTSIDE, sr.UNKNOWN, sr.KNOWN, sr.CONVERGED, sr.MAX_ITERATIONS, sr.NO_OVERLAP) == (0, 1, 2, 0, 1, 2)


def test_defaults(capi):
    a = capi.default_surf_align_params()
    got = {f: getattr(a, f) for f, _ in a._fields_ if f != "reserved"}
    assert got == sr.ALIGN == dict(min_weight=1, max_iterations=50, min_points=6, max_dist=0.4, huber=0.1, step_tol=1e-6, lambda_init=1e-4,
                                   lambda_min=1e-10, lambda_max=1e8)
    assert a.reserved == 0 and capi.default_surf_align_params(huber=0.0, min_points=9).min_points == 9


class _Volume:
    """what mesh.align_params_for reads of a context"""

    def __init__(self, **kw):
        self.p = kw

    def tsdf_params(self):
        from limo_velo_amd import capi

        return capi.default_tsdf_params(**self.p)


def test_align_params_for(capi):
    from limo_velo_amd import mesh

    p = mesh.align_params_for(_Volume(resolution=0.1, trunc_cells=3))
    assert p.max_dist == 2 * float(np.float32(0.1)) and p.huber == float(np.float32(0.1)) / 2 and (p.min_weight, p.max_iterations, p.min_points) == (1, 50, 6)
    p = mesh.align_params_for(_Volume(resolution=0.25, trunc_cells=5), huber=0.0, min_weight=4, max_iterations=7)
    assert (p.max_dist, p.huber, p.min_weight, p.max_iterations) == (1.0, 0.0, 4, 7)
    assert mesh.align_params_for(_Volume(resolution=0.25, trunc_cells=5), max_dist=0.3).max_dist == 0.3


def test_frame_points(capi):
    from limo_velo_amd import mesh

    fx, fy, cx, cy = 50.0, 40.0, 3.5, 2.5
    depth = np.full((6, 8), 2.0, np.float32)
    depth[0, 0], depth[2, 4], depth[4, 4], depth[5, 7] = np.nan, 0.0, np.inf, -1.0
    depth[2, 0] = 3.0
    f = mesh.depth_frame(depth, np.eye(3), np.zeros(3), fx, fy, cx, cy)
    p = mesh.frame_points(f)
    assert p.dtype == np.float32 and p.shape == (48 - 4, 3)                  # NaN, 0, inf and a negative depth are skipped
    v, u = np.divmod(np.arange(48), 8)
    ok = np.isfinite(depth.reshape(-1)) & (depth.reshape(-1) > 0)
    z = depth.reshape(-1).astype(np.float64)
    want = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)[ok].astype(np.float32)
    assert np.array_equal(p, want)                                          # row-major, pixel centres at whole u, v
    # every second row and column: the pixels (0, 0), (0, 2), ... of which (0, 0), (2, 4) and (4, 4) are invalid
    p2 = mesh.frame_points(f, stride=2)
    keep = ((v % 2 == 0) & (u % 2 == 0))
    assert np.array_equal(p2, np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)[ok & keep].astype(np.float32)) and len(p2) == 12 - 3
    # uint16 in units of depth_scale, 0 = no measurement
    d16 = np.where(ok, np.round(z * 1000), 0).astype(np.uint16).reshape(6, 8)
    p16 = mesh.frame_points(mesh.depth_frame(d16, np.eye(3), np.zeros(3), fx, fy, cx, cy, depth_scale=0.001))
    assert p16.shape == p.shape and np.abs(p16 - p).max() <= 1e-6
    # the pattern of mesh.camera_pattern: a point lies on its pixel's ray
    ray = mesh.camera_pattern(fx, fy, cx, cy, 8, 6, 1.0).astype(np.float64)[ok]
    assert np.abs(np.cross(ray, p.astype(np.float64))).max() <= 1e-6
    with pytest.raises(ValueError, match="dist"):
        mesh.frame_points(mesh.depth_frame(depth, np.eye(3), np.zeros(3), fx, fy, cx, cy, dist=[0.1, 0, 0, 0, 0]))
    assert len(mesh.frame_points(mesh.depth_frame(depth, np.eye(3), np.zeros(3), fx, fy, cx, cy, dist=[0, 0, 0, 0, 0]))) == 44
    with pytest.raises(ValueError, match="stride"):
        mesh.frame_points(f, stride=0)


def test_loop_measurement_takes_a_surface_result(capi):
    from limo_velo_amd import mesh, ndt

    import graph_ref as gr
    rng = np.random.default_rng(5)
    xi, xj = np.concatenate([rng.normal(size=3), gr.qexp(rng.normal(size=3))]), np.concatenate([rng.normal(size=3), gr.qexp(rng.normal(size=3))])
    A = rng.normal(size=(6, 6))
    res = np.zeros((), capi.SURF_ALIGN_RESULT_DTYPE)
    res["t"], res["q"], res["info"] = xj[:3], xj[3:], (A.T @ A)[np.triu_indices(6)]
    as_ndt = np.zeros((), capi.NDT_RESULT_DTYPE)
    as_ndt["t"], as_ndt["q"], as_ndt["info"] = res["t"], res["q"], res["info"]
    for a, b in zip(mesh.loop_measurement(xi, res), ndt.loop_measurement(xi, as_ndt)):
        assert np.array_equal(a, b)
    tr, qr = gr.relative(xi, xj)
    assert np.allclose(mesh.loop_measurement(xi, res)[0], tr, atol=1e-14)
    # the quaternion of a rotation matrix, every branch
    for v in ([0.1, -0.2, 0.3], [3.0, 0.1, 0.1], [0.1, 3.0, -0.1], [0.1, 0.1, 3.1], [0, 0, 0]):
        q = gr.qexp(np.array(v, float))
        got = mesh._quat_of(gr.rot(q))
        assert min(np.abs(got - q).max(), np.abs(got + q).max()) <= 1e-14


def test_every_einval_path_through_a_null_context(capi):
    lib = capi.load_library()
    err = lambda: lib.lv_last_error().decode()
    pts = np.zeros((4, 3), np.float32)
    A = C.c_void_p(pts.ctypes.data)
    out, status = (C.c_double * 16)(*([7.0] * 16)), (C.c_uint8 * 4)(9, 9, 9, 9)
    # sample: min_weight, the outputs, n, the points, then the context
    assert lib.lv_surf_sample(None, 0, A, 12, 4, out, status) == LV_EINVAL and "min_weight = 0" in err()
    assert lib.lv_surf_sample(None, 1, A, 12, 4, None, None) == LV_EINVAL and "both null" in err()
    assert lib.lv_surf_sample(None, 1, A, 12, (1 << 31) - 1, out, status) == LV_EINVAL and "too many points" in err()
    assert lib.lv_surf_sample(None, 1, None, 12, 4, out, status) == LV_EINVAL and "bad point array" in err()
    assert lib.lv_surf_sample(None, 1, A, 8, 4, out, status) == LV_EINVAL and "stride 8" in err()
    assert lib.lv_surf_sample(None, 1, A, 12, 4, out, status) == LV_EINVAL and err() == "null context"
    assert lib.lv_surf_sample(None, 1, A, 12, 4, out, None) == LV_EINVAL and err() == "null context"
    assert lib.lv_surf_sample(None, 1, None, 0, 0, None, status) == LV_EINVAL and err() == "null context"
    assert list(out) == [7.0] * 16 and list(status) == [9] * 4       # nothing was written
    # align
    g = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (4, 1))
    G = g.ctypes.data_as(C.POINTER(capi.GraphPose))
    res, best = (capi.SurfAlignResult * 4)(), (C.c_int32 * 2)(7, 7)
    AP = capi.default_surf_align_params

    def align(prm=None, src=A, stride=12, n=4, guesses=G, K=4, results=res, b=best):
        return lib.lv_surf_align(None, None if prm is None else C.byref(prm), src, stride, n, guesses, K, results, b)

    for kw, what in ((dict(min_weight=0), "min_weight"), (dict(max_iterations=-1), "max_iterations"), (dict(max_iterations=1001), "max_iterations"),
                     (dict(min_points=0), "min_points"), (dict(max_dist=0.0), "max_dist"), (dict(max_dist=math.inf), "max_dist"),
                     (dict(max_dist=math.nan), "max_dist"), (dict(huber=-0.1), "huber"), (dict(huber=math.inf), "huber"), (dict(step_tol=-1.0), "step_tol"),
                     (dict(lambda_min=0.0), "lambda"), (dict(lambda_init=1e9), "lambda"), (dict(lambda_max=math.inf), "lambda")):
        assert align(AP(**kw)) == LV_EINVAL and err().startswith("lv_surf_align: ") and what in err() and "null context" not in err(), (kw, err())
    assert align(b=None) == LV_EINVAL and "null best" in err()
    assert align(K=4097) == LV_EINVAL and "4096" in err()
    assert align(n=(1 << 20) + 1) == LV_EINVAL and "2^20" in err()
    assert align(n=1 << 20, K=1025) == LV_EINVAL and "2^30" in err()
    assert align(src=None) == LV_EINVAL and "source" in err()
    assert align(stride=4) == LV_EINVAL and "stride 4" in err()
    assert align(guesses=None) == LV_EINVAL and "null guesses" in err()
    assert align(results=None) == LV_EINVAL and "null results" in err()
    g[2, 6] = 1.00001
    assert align() == LV_EINVAL and "guess 2: q: norm" in err()
    g[2, 6], g[1, 0] = 1.0, math.nan
    assert align() == LV_EINVAL and "guess 1: t: a non-finite" in err()
    g[1, 0] = 0.0
    assert align() == LV_EINVAL and err() == "null context"
    assert align(AP()) == LV_EINVAL and err() == "null context"
    assert align(src=None, n=0, guesses=None, K=0, results=None) == LV_EINVAL and err() == "null context"
    assert list(best) == [7, 7] and not bytes(res).strip(b"\0")     # nothing was written
