"""CPU checks of the surface entry points (include/limovelo_hip.h "Surface normals and outlier removal"): the built library
exports them, the ctypes signatures and struct layouts capi installs agree with the header, the defaults are as documented and
null arguments are refused."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_surface_params", "lv_default_outlier_params", "lv_map_normals", "lv_map_remove_outliers")


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


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "lv_surface_params*": C.POINTER(capi.SurfaceParams),
             "lv_outlier_params*": C.POINTER(capi.OutlierParams), "uint8_t*": C.POINTER(C.c_uint8), "size_t*": C.POINTER(C.c_size_t),
             "float*": C.POINTER(C.c_float), "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double)}
    for name, restype in (("lv_map_normals", C.c_int), ("lv_map_remove_outliers", C.c_int),
                          ("lv_default_surface_params", None), ("lv_default_outlier_params", None)):
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is restype


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fields_s = [f for f, _ in capi.SurfaceParams._fields_]
    fields_o = [f for f, _ in capi.OutlierParams._fields_]
    exprs = ["sizeof(lv_surface_params)"] + [f"offsetof(lv_surface_params, {f})" for f in fields_s] + ["sizeof(lv_outlier_params)"] + \
            [f"offsetof(lv_outlier_params, {f})" for f in fields_o]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.SurfaceParams)] + [getattr(capi.SurfaceParams, f).offset for f in fields_s] + [C.sizeof(capi.OutlierParams)] + \
           [getattr(capi.OutlierParams, f).offset for f in fields_o]
    assert got == want
    assert fields_s == ["k", "max_dist", "min_neighbours", "orient", "viewpoint"]
    assert fields_o == ["mode", "k", "max_dist", "std_mul", "radius", "min_neighbours", "dry_run"]


def test_default_params_round_trip(capi):
    p = capi.default_surface_params()
    assert (p.k, p.max_dist, p.min_neighbours, p.orient, list(p.viewpoint)) == (10, 2.0, 5, 0, [0.0, 0.0, 0.0])
    o = capi.default_outlier_params()
    assert (o.mode, o.k, o.max_dist, o.std_mul, o.radius, o.min_neighbours, o.dry_run) == (0, 10, 2.0, 2.0, 0.5, 5, 0)
    q = capi.default_surface_params(k=20, orient=1, viewpoint=(1.0, 2.0, 3.0))
    assert (q.k, q.orient, list(q.viewpoint), q.min_neighbours) == (20, 1, [1.0, 2.0, 3.0], 5)
    assert capi.default_outlier_params(mode=1, radius=0.25).radius == 0.25


def test_bad_arguments_are_refused_without_a_context(capi):
    lib = capi.load_library()
    p = capi.default_surface_params()
    o = capi.default_outlier_params()
    assert lib.lv_map_normals(None, C.byref(p), None, None, None, None, 0) != 0
    assert lib.lv_map_remove_outliers(None, C.byref(o), None, None, None) != 0
