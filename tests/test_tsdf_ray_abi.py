"""CPU checks of the surface ray casting entry points (include/limovelo_hip.h "Surface ray casting"): the built library exports
them, the ctypes signatures and the layout of the two structs capi installs agree with the header (lv_tsdf_ray_result is 32
bytes), the defaults are as documented, and every refusal that needs no GPU shows in the stated order: arguments are judged before
the context, both calls refuse a NULL context last, and a refused call writes nothing.  LV_ESTATE before lv_tsdf_configure needs a
live context: the one test here marked gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_surf_ray_params", "lv_surf_raycast", "lv_surf_raycast_views")
FIELDS = ["status", "cell", "steps", "axis", "depth", "t", "n_known", "n_unknown"]
LV_EINVAL, LV_ESTATE = -1, -4
F = np.float32


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


def test_library_exports_the_symbols(capi):
    lib = capi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS
    text = open(HEADER).read()
    for name, value in (("LV_SURF_IGNORED", 0), ("LV_SURF_CLEAR", 1), ("LV_SURF_HIT", 2), ("LV_SURF_BLOCKED", 3)):
        assert getattr(capi, name) == value and re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text)
    assert "/* ---- Surface ray casting" in text and text.index("/* ---- Surface ray casting") > text.index("/* ---- Colour layer")


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "void*": C.c_void_p, "lv_tsdf_ray_params*": C.POINTER(capi.TsdfRayParams),
             "lv_tsdf_ray_result*": C.POINTER(capi.TsdfRayResult), "lv_view*": C.POINTER(capi.View), "uint64_t": C.POINTER(C.c_uint64),
             "float*": C.POINTER(C.c_float), "uint8_t*": C.POINTER(C.c_uint8)}
    counts = {"lv_default_surf_ray_params": 1, "lv_surf_raycast": 10, "lv_surf_raycast_views": 9}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = re.sub(r"\[\d+\]$", "", p)   # (uint64_t stats[4]: a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_surf_ray_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = [("lv_tsdf_ray_params", capi.TsdfRayParams), ("lv_tsdf_ray_result", capi.TsdfRayResult)]
    assert [f for f, _ in capi.TsdfRayParams._fields_] == ["min_weight", "reserved"]
    assert [f for f, _ in capi.TsdfRayResult._fields_] == FIELDS
    exprs, want = [], []
    for cname, t in structs:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(t))
        for f, _ in t._fields_:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(t, f).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) +
                   'printf("%d %d %d %d\\n", LV_SURF_IGNORED, LV_SURF_CLEAR, LV_SURF_HIT, LV_SURF_BLOCKED);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want + [0, 1, 2, 3]
    assert C.sizeof(capi.TsdfRayResult) == 32 and capi.TSDF_RAY_RESULT_DTYPE.itemsize == 32 and C.sizeof(capi.TsdfRayParams) == 8
    assert [getattr(capi.TsdfRayResult, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [capi.TSDF_RAY_RESULT_DTYPE.fields[f][1] for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert all(capi.TSDF_RAY_RESULT_DTYPE.fields[f][0] == np.int32 for f in FIELDS)


def test_default_params(capi):
    p = capi.TsdfRayParams(99, 99)
    capi.load_library().lv_default_surf_ray_params(C.byref(p))
    assert (p.min_weight, p.reserved) == (1, 0)
    assert capi.default_tsdf_ray_params(min_weight=3).min_weight == 3
    capi.load_library().lv_default_surf_ray_params(None)   # (a NULL target is ignored)


def _rays(capi, n):
    a = np.zeros((n, 3), F)
    b = np.ones((n, 3), F)
    out = np.full(n, 9, np.uint8).repeat(32).view(capi.TSDF_RAY_RESULT_DTYPE)
    return a, b, out, np.full((n, 3), 9.0, F), np.full((n, 4), 9, np.uint8)


def test_raycast_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    p = capi.default_tsdf_ray_params()
    a, b, out, nrm, col = _rays(capi, 4)
    vp, rp = C.c_void_p, C.POINTER(capi.TsdfRayResult)
    N, K = nrm.ctypes.data_as(C.POINTER(C.c_float)), col.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(params, frm, fs, to, ts, n, res, normals=N, rgba=K):
        rc = lib.lv_surf_raycast(None, params, frm, fs, to, ts, n, res, normals, rgba)
        return rc, lib.lv_last_error().decode()

    A, B, O = a.ctypes.data_as(vp), b.ctypes.data_as(vp), out.ctypes.data_as(rp)
    for args in ((C.byref(p), A, 12, B, 12, 4, O), (C.byref(p), A, 12, B, 12, 0, O), (C.byref(p), None, 0, None, 0, 0, None),
                 (C.byref(capi.default_tsdf_ray_params(min_weight=7)), A, 16, B, 24, 2, O), (C.byref(p), A, 12, B, 12, 4, O, None, None)):
        rc, why = call(*args)
        assert rc == LV_EINVAL and "null context" in why, (args, why)   # (good arguments: only the context is missing)
    zero, minus = capi.default_tsdf_ray_params(min_weight=0), capi.default_tsdf_ray_params(min_weight=-3)
    bad = [((None, A, 12, B, 12, 4, O), "null params"), ((C.byref(zero), A, 12, B, 12, 4, O), "min_weight"),
           ((C.byref(minus), A, 12, B, 12, 0, O), "min_weight"), ((C.byref(p), None, 12, B, 12, 4, O), "point arrays"),
           ((C.byref(p), A, 12, None, 12, 4, O), "point arrays"), ((C.byref(p), A, 12, B, 12, 4, None), "null output"),
           ((C.byref(p), A, 11, B, 12, 4, O), "strides 11"), ((C.byref(p), A, 12, B, 8, 4, O), "12, 8"),
           ((C.byref(p), A, 12, B, 12, 2 ** 31 - 1, O), "too many"), ((C.byref(p), A, 12, B, 12, 2 ** 40, O), "too many"),
           ((C.byref(zero), A, 8, B, 12, 4, None), "min_weight")]   # (the parameters come first)
    for args, what in bad:
        rc, why = call(*args)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (what, why)
    assert np.all(out.view(np.uint8) == 9) and np.all(nrm == 9.0) and np.all(col == 9)   # (nothing written)


def test_views_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    p = capi.default_tsdf_ray_params()
    pts = np.ones((5, 3), F)
    Id = np.eye(3, dtype=F)
    _, _, out, nrm, col = _rays(capi, 200)
    stats = (C.c_uint64 * 4)(*([7] * 4))
    O, N, K = out.ctypes.data_as(C.POINTER(capi.TsdfRayResult)), nrm.ctypes.data_as(C.POINTER(C.c_float)), col.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(views, n=None, params=p, res=O, capacity=200, st=stats):
        arr, keep = capi.view_array(views)
        rc = lib.lv_surf_raycast_views(None, C.byref(params) if params is not None else None, arr, len(views) if n is None else n, res, N, K,
                                       capacity, st)
        return rc, lib.lv_last_error().decode()

    good = [(Id, np.zeros(3, F), pts), (Id, np.ones(3, F), np.zeros((0, 3), F))]
    for kw in (dict(views=good), dict(views=good[:1], capacity=5), dict(views=good * 16), dict(views=[(Id, np.array([np.nan, 0, 0], F), pts)]),
               dict(views=good, st=None), dict(views=good[1:], capacity=0)):   # (a non-finite t is a view without evidence)
        rc, why = call(**kw)
        assert rc == LV_EINVAL and "null context" in why, why
    R = Id.copy()
    R[1, 2] = np.inf
    zero = capi.default_tsdf_ray_params(min_weight=0)
    for kw, what in ((dict(views=good, params=None), "null params"), (dict(views=good, params=zero), "min_weight"),
                     (dict(views=good, params=zero, res=None, capacity=0), "min_weight"), (dict(views=good, res=None), "null argument"),
                     (dict(views=good, n=0), "n_views"), (dict(views=good * 16, n=33), "n_views"),
                     (dict(views=[(R, np.zeros(3, F), pts)]), "non-finite R"), (dict(views=good, capacity=4), "room for 5"),
                     (dict(views=good * 16, capacity=79), "room for 80")):
        rc, why = call(**kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (what, why)
    assert lib.lv_surf_raycast_views(None, C.byref(p), None, 1, O, N, K, 200, stats) == LV_EINVAL and "null argument" in lib.lv_last_error().decode()
    arr, keep = capi.view_array(good)
    arr[0].stride = 8
    assert lib.lv_surf_raycast_views(None, C.byref(p), arr, 2, O, N, K, 200, stats) == LV_EINVAL and "stride 8" in lib.lv_last_error().decode()
    arr[0].stride, arr[0].points = 12, None
    assert lib.lv_surf_raycast_views(None, C.byref(p), arr, 2, O, N, K, 200, stats) == LV_EINVAL and "bad point array" in lib.lv_last_error().decode()
    arr[0].n = (1 << 24) + 1
    arr[0].points = pts.ctypes.data
    assert lib.lv_surf_raycast_views(None, C.byref(p), arr, 2, O, N, K, 1 << 25, stats) == LV_EINVAL and "too many returns" in lib.lv_last_error().decode()
    assert list(stats) == [7] * 4 and np.all(out.view(np.uint8) == 9) and np.all(nrm == 9.0) and np.all(col == 9)   # (nothing written)


@pytest.mark.gpu
def test_state_comes_after_the_arguments(capi):
    a, b, out, _, _ = _rays(capi, 4)
    with capi.Context() as ctx:
        with pytest.raises(capi.LvError, match="-4.*lv_tsdf_configure"):
            ctx.tsdf_raycast(a, b)
        with pytest.raises(capi.LvError, match="-4.*lv_tsdf_configure"):
            ctx.tsdf_raycast_views([(np.eye(3, dtype=F), np.zeros(3, F), b)])
        with pytest.raises(capi.LvError, match="-1.*min_weight"):    # (the arguments before the state)
            ctx.tsdf_raycast(a, b, capi.default_tsdf_ray_params(min_weight=0))
        with pytest.raises(capi.LvError, match="-1.*min_weight"):
            ctx.tsdf_raycast_views([(np.eye(3, dtype=F), np.zeros(3, F), b)], capi.default_tsdf_ray_params(min_weight=0))
        ctx.tsdf_configure(capi.default_tsdf_params(nx=8, ny=8, nz=8))
        res, _, _ = ctx.tsdf_raycast(a, b)
        assert np.all(res["status"] == capi.LV_SURF_CLEAR)
