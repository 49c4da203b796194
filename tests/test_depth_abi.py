"""CPU checks of the depth fusion's entry points (include/limovelo_hip.h "Depth fusion"): the built library exports them, the
ctypes signatures and struct layouts capi installs agree with the header, the defaults round-trip, every argument outside its limits
is refused before the context (LV_EINVAL; the null context comes last); capi.depth_view's frames and mesh.py's chunking.  LV_ESTATE
before lv_tsdf_configure needs a live context: tests/test_gpu_depth.py holds it on the device, tests/test_depth_host.py on the host
against the same VolumeTools."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_depth_params", "lv_depth_integrate")
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
    m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in limovelo_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _frame(**kw):
    f = dict(R=np.eye(3), t=np.zeros(3), fx=5.0, fy=5.0, cx=2.5, cy=1.5, depth=np.full((4, 6), 1000, np.uint16))
    f.update(kw)
    return f


def test_library_exports_the_symbols(capi):
    lib = capi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS
        assert "tsdf" not in name   # (the set of lv_tsdf_* functions is closed: tests/test_tsdf_abi.py)
    assert sorted(s for s in capi.ABI_SYMBOLS if "depth" in s) == sorted(SYMBOLS)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "lv_depth_view*": C.POINTER(capi.DepthView), "size_t": C.c_size_t,
             "lv_depth_params*": C.POINTER(capi.DepthParams), "uint64_t[4]": C.POINTER(C.c_uint64)}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = p.replace("const ", "")
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*(\[4\])?$", r"\1", t).replace(" ", "")
            assert t in table, (name, p, t)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_depth_params" else C.c_int)


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fv = [f for f, _ in capi.DepthView._fields_]
    fp = [f for f, _ in capi.DepthParams._fields_]
    exprs = ["sizeof(lv_depth_view)"] + [f"offsetof(lv_depth_view, {f})" for f in fv] + ["sizeof(lv_depth_params)"] + \
            [f"offsetof(lv_depth_params, {f})" for f in fp] + ["LV_DEPTH_U16", "LV_DEPTH_F32"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for cls, fields in ((capi.DepthView, fv), (capi.DepthParams, fp)):
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want + [capi.LV_DEPTH_U16, capi.LV_DEPTH_F32] and got[-2:] == [0, 1]
    assert fv == ["R", "t", "fx", "fy", "cx", "cy", "dist", "width", "height", "format", "depth_scale", "depth", "row_stride"]
    assert fp == ["min_depth", "max_depth", "max_norm_radius", "carve", "reserved"]
    # R .. dist lie as in lv_camera_view: "exactly the meaning they have" includes the place
    for f in ("R", "t", "fx", "fy", "cx", "cy", "dist", "width", "height", "format"):
        assert getattr(capi.DepthView, f).offset == getattr(capi.LvCameraView, f).offset


def test_default_params_round_trip(capi):
    p = capi.default_depth_params()
    q = capi.default_paint_params()
    assert (p.min_depth, p.max_depth, p.max_norm_radius, p.carve, p.reserved) == (np.float32(0.3), 10.0, 1.5, 0, 0)
    assert (p.min_depth, p.max_norm_radius) == (q.min_depth, q.max_norm_radius)
    r = capi.default_depth_params(max_depth=4.0, carve=1)
    assert (r.min_depth, r.max_depth, r.max_norm_radius, r.carve) == (np.float32(0.3), 4.0, 1.5, 1)
    capi.load_library().lv_default_depth_params(None)   # (a null pointer is ignored)


def test_limits_are_refused_before_the_context(capi):
    lib = capi.load_library()
    view, keep = capi.depth_view(_frame())
    views = (capi.DepthView * 33)(*([view] * 33))

    def why(rc):
        assert rc == LV_EINVAL
        return lib.lv_last_error().decode()

    def integrate(n=1, v=views, **kw):
        return why(lib.lv_depth_integrate(None, v, n, C.byref(capi.default_depth_params(**kw)), None))

    def with_view(**kw):
        bad = (capi.DepthView * 1)(view)
        for k, val in kw.items():
            if k in ("R", "t", "dist"):
                getattr(bad[0], k)[1] = val
            else:
                setattr(bad[0], k, val)
        return integrate(v=bad)

    assert integrate() == "null context"   # everything else holds: the context is judged last
    assert integrate(n=32) == "null context" and integrate(carve=1) == "null context"
    assert "n_views = 0" in integrate(n=0) and "n_views = 33" in integrate(n=33)
    assert "null argument" in integrate(v=None)
    assert "null argument" in why(lib.lv_depth_integrate(None, views, 1, None, None))
    assert "depths [0, 10]" in integrate(min_depth=0.0) and "depths [5, 5]" in integrate(min_depth=5.0, max_depth=5.0)
    assert "depths [0.3, inf]" in integrate(max_depth=float("inf")) and "depths [nan, 10]" in integrate(min_depth=float("nan"))
    assert "max_norm_radius = 0" in integrate(max_norm_radius=0.0) and "max_norm_radius = inf" in integrate(max_norm_radius=float("inf"))
    assert "carve = 2" in integrate(carve=2) and "carve = -1" in integrate(carve=-1)
    assert "non-finite R" in with_view(R=float("inf")) and "non-finite t" in with_view(t=float("nan"))
    assert "non-finite intrinsics" in with_view(fx=float("nan")) and "non-finite intrinsics" in with_view(cy=float("inf"))
    assert "non-finite distortion" in with_view(dist=float("nan"))
    assert "image of 0 x 4" in with_view(width=0) and "image of 6 x 8193" in with_view(height=8193)
    assert "image of 8192 x 8192" in with_view(width=8192, height=8192, row_stride=1 << 20)
    assert "format 2" in with_view(format=2) and "format -1" in with_view(format=-1)
    assert "depth_scale = 0" in with_view(depth_scale=0.0) and "depth_scale = inf" in with_view(depth_scale=float("inf"))
    assert "depth_scale = nan" in with_view(depth_scale=float("nan")) and "depth_scale = -0.001" in with_view(depth_scale=-0.001)
    assert "null depth" in with_view(depth=None) and "row_stride 11 < 12" in with_view(row_stride=11)
    assert "row_stride 23 < 24" in with_view(format=capi.LV_DEPTH_F32, row_stride=23)
    assert with_view(format=capi.LV_DEPTH_F32, row_stride=24, depth_scale=0.0) == "null context"   # (ignored for F32)
    big = (capi.DepthView * 5)(*([view] * 5))
    for b in big:
        b.width = b.height = 4096
        b.row_stride = 8192
    assert "more than 2^26 pixels" in integrate(n=5, v=big) and integrate(n=4, v=big) == "null context"   # (nothing is read before the context)


def test_depth_view_frames(capi):
    v, img = capi.depth_view(_frame())
    assert (v.width, v.height, v.format, v.row_stride, v.depth_scale) == (6, 4, capi.LV_DEPTH_U16, 12, np.float32(0.001)) and v.depth == img.ctypes.data
    assert list(v.dist) == [0.0] * 5 and list(v.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    wide = np.zeros((4, 9), np.float32)
    v, img = capi.depth_view(_frame(depth=wide[:, 2:8], depth_scale=0.5, dist=[1, 2, 3, 4, 5]))   # strided rows are handed on as they are
    assert (v.format, v.row_stride, v.width, v.depth_scale) == (capi.LV_DEPTH_F32, 36, 6, 0.5) and v.depth == wide.ctypes.data + 8
    assert list(v.dist) == [1, 2, 3, 4, 5]
    v, img = capi.depth_view(_frame(depth=np.zeros((4, 12), np.uint16)[:, ::2]))   # strided pixels are copied
    assert v.row_stride == 12 and img.flags["C_CONTIGUOUS"]
    v, img = capi.depth_view(_frame(depth=np.zeros((4, 6), np.uint16)[::-1]))      # and so are rows that run backwards
    assert v.row_stride == 12 and v.depth == img.ctypes.data
    for bad in (np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.float64), np.zeros((4, 6, 1), np.uint16), np.zeros(6, np.uint16)):
        with pytest.raises(ValueError):
            capi.depth_view(_frame(depth=bad))


class _FakeCtx:
    def __init__(self):
        self.calls = []

    def tsdf_integrate_depth(self, frames, params):
        self.calls.append(([f["id"] for f in frames], params))
        return np.array([10 * len(frames), len(frames), 2, 1], np.uint64)


def test_integrate_depth_chunks_and_frames(capi):
    from limo_velo_amd import mesh

    ctx = _FakeCtx()
    p = capi.default_depth_params(carve=1)
    stats = mesh.integrate_depth(ctx, [dict(id=i) for i in range(70)], p)
    assert [c[0] for c in ctx.calls] == [list(range(32)), list(range(32, 64)), list(range(64, 70))] and all(c[1] is p for c in ctx.calls)
    assert list(stats) == [700, 70, 6, 3]
    assert mesh.integrate_depth(_FakeCtx(), []).tolist() == [0, 0, 0, 0]
    ctx = _FakeCtx()
    mesh.integrate_depth(ctx, [dict(id=0)])
    assert (ctx.calls[0][1].max_depth, ctx.calls[0][1].carve) == (10.0, 0)
    d = np.full((4, 6), 700, np.uint16)
    f = mesh.depth_frame(d, np.eye(3), [1, 2, 3], 5, 6, 2.5, 1.5)
    assert f["depth"] is d and f["depth_scale"] == 0.001 and "dist" not in f and f["R"].dtype == np.float32 and f["t"].tolist() == [1, 2, 3]
    assert (f["fx"], f["fy"], f["cx"], f["cy"]) == (5.0, 6.0, 2.5, 1.5)
    g = mesh.depth_frame(d.astype(np.float32), np.eye(3), [0, 0, 0], 5, 5, 2.5, 1.5, depth_scale=0.002, dist=[0.1, 0, 0, 0, 0])
    v, _ = capi.depth_view(g)
    assert v.format == capi.LV_DEPTH_F32 and v.depth_scale == np.float32(0.002) and v.dist[0] == np.float32(0.1)
