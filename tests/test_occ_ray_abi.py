"""CPU checks of the ray-casting entry points (include/limovelo_hip.h "Ray casting"): the built library exports them, the ctypes
signatures and the layout of the two structs capi installs agree with the header (lv_ray_result is 32 bytes), the defaults are as
documented, and every refusal that needs no GPU shows: arguments are judged before the context, both calls refuse a NULL context,
and a refused call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_ray_params", "lv_occ_raycast", "lv_occ_view_gain")
LV_EINVAL = -1
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
    for name, value in (("LV_RAY_IGNORED", 0), ("LV_RAY_CLEAR", 1), ("LV_RAY_STOPPED", 2)):
        assert getattr(capi, name) == value and re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text)
    assert "/* ---- Ray casting" in text and text.index("/* ---- Ray casting") > text.index("/* ---- Frontiers")


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "void*": C.c_void_p, "lv_ray_params*": C.POINTER(capi.RayParams),
             "lv_ray_result*": C.POINTER(capi.RayResult), "lv_view*": C.POINTER(capi.View), "uint64_t*": C.POINTER(C.c_uint64)}
    counts = {"lv_default_ray_params": 1, "lv_occ_raycast": 8, "lv_occ_view_gain": 4}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_ray_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = [("lv_ray_params", capi.RayParams), ("lv_ray_result", capi.RayResult)]
    assert [f for f, _ in capi.RayParams._fields_] == ["stop_unknown"]
    assert [f for f, _ in capi.RayResult._fields_] == ["status", "cell", "steps", "axis", "n_free", "n_unknown", "num", "den"]
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
                   'printf("%d %d %d\\n", LV_RAY_IGNORED, LV_RAY_CLEAR, LV_RAY_STOPPED);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want + [0, 1, 2]
    assert C.sizeof(capi.RayResult) == 32 and capi.RAY_RESULT_DTYPE.itemsize == 32
    assert [getattr(capi.RayResult, f).offset for f, _ in capi.RayResult._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [capi.RAY_RESULT_DTYPE.fields[f][1] for f, _ in capi.RayResult._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert all(capi.RAY_RESULT_DTYPE.fields[f][0] == np.int32 for f, _ in capi.RayResult._fields_)


def test_default_params(capi):
    p = capi.RayParams(99)
    capi.load_library().lv_default_ray_params(C.byref(p))
    assert p.stop_unknown == 0
    assert capi.default_ray_params(stop_unknown=1).stop_unknown == 1
    capi.load_library().lv_default_ray_params(None)   # (a NULL target is ignored)


def _rays(capi, n):
    a = np.zeros((n, 3), F)
    b = np.ones((n, 3), F)
    out = np.full(n, 9, np.uint8).repeat(32).view(capi.RAY_RESULT_DTYPE)
    return a, b, out


def test_raycast_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    p = capi.default_ray_params()
    a, b, out = _rays(capi, 4)
    vp, rp = C.c_void_p, C.POINTER(capi.RayResult)

    def call(params, frm, fs, to, ts, n, res):
        rc = lib.lv_occ_raycast(None, params, frm, fs, to, ts, n, res)
        return rc, lib.lv_last_error().decode()

    A, B, O = a.ctypes.data_as(vp), b.ctypes.data_as(vp), out.ctypes.data_as(rp)
    for args in ((C.byref(p), A, 12, B, 12, 4, O), (C.byref(p), A, 12, B, 12, 0, O), (C.byref(p), None, 0, None, 0, 0, None),
                 (C.byref(capi.default_ray_params(stop_unknown=7)), A, 16, B, 24, 2, O)):
        rc, why = call(*args)
        assert rc == LV_EINVAL and "null context" in why, (args, why)   # (good arguments: only the context is missing)
    bad = [((None, A, 12, B, 12, 4, O), "null params"), ((C.byref(p), None, 12, B, 12, 4, O), "point arrays"),
           ((C.byref(p), A, 12, None, 12, 4, O), "point arrays"), ((C.byref(p), A, 12, B, 12, 4, None), "null output"),
           ((C.byref(p), A, 11, B, 12, 4, O), "strides 11"), ((C.byref(p), A, 12, B, 8, 4, O), "12, 8"),
           ((C.byref(p), A, 12, B, 12, 2 ** 31 - 1, O), "too many"), ((C.byref(p), A, 12, B, 12, 2 ** 40, O), "too many")]
    for args, what in bad:
        rc, why = call(*args)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (what, why)
    assert np.all(out.view(np.uint8) == 9)   # (nothing written)


def test_view_gain_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    pts = np.ones((5, 3), F)
    Id = np.eye(3, dtype=F)
    gain = (C.c_uint64 * 8)(*([7] * 8))

    def call(views, n=None, g=gain):
        arr, keep = capi.view_array(views)
        rc = lib.lv_occ_view_gain(None, arr, len(views) if n is None else n, g)
        return rc, lib.lv_last_error().decode()

    good = [(Id, np.zeros(3, F), pts), (Id, np.ones(3, F), np.zeros((0, 3), F))]
    for views in (good, good[:1], good * 16, [(Id, np.array([np.nan, 0, 0], F), pts)]):   # (a non-finite t is a view without evidence)
        rc, why = call(views) if len(views) <= 2 else call(views, g=(C.c_uint64 * 128)())
        assert rc == LV_EINVAL and "null context" in why, why
    R = Id.copy()
    R[1, 2] = np.inf
    for (views, n, g), what in ((((good, 0, gain)), "n_views"), ((good * 16, 33, gain), "n_views"), ((good, None, None), "null argument"),
                                (([(R, np.zeros(3, F), pts)], None, gain), "non-finite R")):
        rc, why = call(views, n, g)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (what, why)
    assert lib.lv_occ_view_gain(None, None, 1, gain) == LV_EINVAL and "null argument" in lib.lv_last_error().decode()
    arr, keep = capi.view_array(good)
    arr[0].stride = 8
    assert lib.lv_occ_view_gain(None, arr, 2, gain) == LV_EINVAL and "stride 8" in lib.lv_last_error().decode()
    arr[0].stride, arr[0].points = 12, None
    assert lib.lv_occ_view_gain(None, arr, 2, gain) == LV_EINVAL and "bad point array" in lib.lv_last_error().decode()
    assert list(gain) == [7] * 8   # (nothing written)
