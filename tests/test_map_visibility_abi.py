"""CPU checks of the dynamic-point removal entry points (include/limovelo_hip.h "Dynamic-point removal"): the built library
exports lv_default_visibility_params / lv_map_remove_dynamic, the ctypes signatures and struct layouts capi installs agree
with the header, and the defaults round-trip."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_visibility_params", "lv_map_remove_dynamic")


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
    table = {"lv_ctx*": C.c_void_p, "lv_view*": C.POINTER(capi.View), "size_t": C.c_size_t,
             "lv_visibility_params*": C.POINTER(capi.VisibilityParams), "uint8_t*": C.POINTER(C.c_uint8),
             "size_t*": C.POINTER(C.c_size_t)}
    for name, restype in (("lv_map_remove_dynamic", C.c_int), ("lv_default_visibility_params", None)):
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
    fields_v = ["R", "t", "points", "stride", "n"]
    fields_p = [f for f, _ in capi.VisibilityParams._fields_]
    exprs = ["sizeof(lv_view)"] + [f"offsetof(lv_view, {f})" for f in fields_v] + ["sizeof(lv_visibility_params)"] + \
            [f"offsetof(lv_visibility_params, {f})" for f in fields_p]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.View)] + [getattr(capi.View, f).offset for f in fields_v] + [C.sizeof(capi.VisibilityParams)] + \
           [getattr(capi.VisibilityParams, f).offset for f in fields_p]
    assert got == want
    assert [f for f, _ in capi.View._fields_] == fields_v


def test_default_params_round_trip(capi):
    p = capi.default_visibility_params()
    assert (p.width, p.height, p.window, p.min_hits, p.dry_run) == (2048, 64, 1, 1, 0)
    assert (p.v_min_deg, p.v_max_deg, p.min_range, p.max_range) == (-25.0, 3.0, 1.0, 80.0)
    assert abs(p.margin_abs - 0.3) < 1e-7 and abs(p.margin_rel - 0.02) < 1e-9
    q = capi.default_visibility_params(width=512, window=3)
    assert (q.width, q.window, q.height) == (512, 3, 64)


def test_bad_arguments_are_refused_without_a_context(capi):
    lib = capi.load_library()
    p = capi.default_visibility_params()
    views = (capi.View * 1)()
    assert lib.lv_map_remove_dynamic(None, views, 1, C.byref(p), None, None) != 0
