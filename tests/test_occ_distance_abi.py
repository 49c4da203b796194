"""CPU checks of the distance field's entry points (include/limovelo_hip.h "Distance field"): the built library exports them, the
ctypes signatures and the layout of both structs capi installs agree with the header, the defaults are as documented, and every
refusal that needs no GPU shows: lv_occ_distance_build judges its parameters and lv_occ_distance_fetch its outputs before the
context, and every call refuses a NULL context."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_distance_params", "lv_occ_distance_build", "lv_occ_distance_fetch", "lv_occ_distance_query", "lv_occ_distance_info",
           "lv_occ_distance_clear")
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


def test_library_exports_the_symbols(capi):
    lib = capi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS
    assert capi.LV_OCC_FAR == 2147483647 and re.search(r"#define\s+LV_OCC_FAR\s+2147483647\b", open(HEADER).read())


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "lv_distance_params*": C.POINTER(capi.DistanceParams),
             "lv_distance_info*": C.POINTER(capi.DistanceInfo), "void*": C.c_void_p, "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "uint64_t*": C.POINTER(C.c_uint64)}
    counts = {"lv_default_distance_params": 1, "lv_occ_distance_build": 3, "lv_occ_distance_fetch": 4, "lv_occ_distance_query": 6,
              "lv_occ_distance_info": 2, "lv_occ_distance_clear": 1}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = p.replace("stats[4]", "*stats")   # (uint64_t stats[4] is a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_distance_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    pf = [f for f, _ in capi.DistanceParams._fields_]
    inf = [f for f, _ in capi.DistanceInfo._fields_]
    assert pf == ["planar", "k_lo", "k_hi", "unknown_is_obstacle", "signed_field", "max_cells"]
    assert inf == ["built", "planar", "nx", "ny", "nz", "stale", "params"]
    exprs = (["sizeof(lv_distance_params)"] + [f"offsetof(lv_distance_params, {f})" for f in pf] + ["sizeof(lv_distance_info)"] +
             [f"offsetof(lv_distance_info, {f})" for f in inf] + ["LV_OCC_FAR"])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = ([C.sizeof(capi.DistanceParams)] + [getattr(capi.DistanceParams, f).offset for f in pf] + [C.sizeof(capi.DistanceInfo)] +
            [getattr(capi.DistanceInfo, f).offset for f in inf] + [capi.LV_OCC_FAR])
    assert got == want


def test_default_params(capi):
    p = capi.DistanceParams(9, 9, 9, 9, 9, 9)
    capi.load_library().lv_default_distance_params(C.byref(p))
    assert [getattr(p, f) for f, _ in capi.DistanceParams._fields_] == [0] * 6
    q = capi.default_distance_params(planar=1, k_hi=4, max_cells=10)
    assert (q.planar, q.k_lo, q.k_hi, q.unknown_is_obstacle, q.signed_field, q.max_cells) == (1, 0, 4, 0, 0, 10)
    capi.load_library().lv_default_distance_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)

    def refused(**kw):
        p = capi.default_distance_params(**kw)
        rc = lib.lv_occ_distance_build(None, C.byref(p), stats)
        return rc, lib.lv_last_error().decode()

    for kw in (dict(), dict(max_cells=1), dict(max_cells=1024), dict(planar=1, k_lo=3, k_hi=3), dict(k_lo=5, k_hi=2), dict(signed_field=1)):
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and "null context" in why, (kw, why)   # (good parameters: only the context is missing)
    for kw, what in ((dict(max_cells=-1), "max_cells"), (dict(max_cells=1025), "max_cells"), (dict(planar=1, k_lo=3, k_hi=2), "k_lo <= k_hi")):
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, why)
    assert lib.lv_occ_distance_build(None, None, stats) == LV_EINVAL and "null params" in lib.lv_last_error().decode()
    assert lib.lv_occ_distance_fetch(None, None, None, 8) == LV_EINVAL and "both null" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7]


def test_a_null_context_is_refused_by_every_call(capi):
    lib = capi.load_library()
    p = capi.default_distance_params()
    info = capi.DistanceInfo(5, 5, 5, 5, 5, 5)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    s2 = (C.c_int32 * 1)(3)
    out = (C.c_float * 4)(5.0, 5.0, 5.0, 5.0)
    pts = (C.c_float * 3)(0.0, 0.0, 0.0)
    for rc in (lib.lv_occ_distance_build(None, C.byref(p), stats), lib.lv_occ_distance_fetch(None, s2, out, 1),
               lib.lv_occ_distance_fetch(None, s2, None, 1), lib.lv_occ_distance_fetch(None, None, out, 1),
               lib.lv_occ_distance_query(None, pts, 12, 1, out, None), lib.lv_occ_distance_query(None, pts, 12, 1, out, out),
               lib.lv_occ_distance_info(None, C.byref(info)), lib.lv_occ_distance_clear(None)):
        assert rc == LV_EINVAL and "null context" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7] and s2[0] == 3 and list(out) == [5.0] * 4 and info.built == 5   # (nothing written)
