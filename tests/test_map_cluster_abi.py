"""CPU checks of the clustering entry points (include/limovelo_hip.h "Map clustering"): the built library exports them, the
ctypes signatures and the struct layout capi installs agree with the header, the defaults are as documented and null arguments
are refused."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_cluster_params", "lv_map_cluster", "lv_map_remove_clusters")


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
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "lv_cluster_params*": C.POINTER(capi.ClusterParams),
             "uint8_t*": C.POINTER(C.c_uint8), "size_t*": C.POINTER(C.c_size_t), "int32_t*": C.POINTER(C.c_int32),
             "uint32_t*": C.POINTER(C.c_uint32)}
    for name, restype in (("lv_map_cluster", C.c_int), ("lv_map_remove_clusters", C.c_int), ("lv_default_cluster_params", None)):
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is restype
    assert len(_prototype("lv_map_cluster")) == 8 and len(_prototype("lv_map_remove_clusters")) == 6


def test_struct_layout_matches_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fields = [f for f, _ in capi.ClusterParams._fields_]
    exprs = ["sizeof(lv_cluster_params)"] + [f"offsetof(lv_cluster_params, {f})" for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.ClusterParams)] + [getattr(capi.ClusterParams, f).offset for f in fields]
    assert got == want
    assert fields == ["radius", "min_size", "max_size", "dry_run"]


def test_default_params_round_trip(capi):
    p = capi.default_cluster_params()
    assert (p.radius, p.min_size, p.max_size, p.dry_run) == (0.5, 1, 0, 0)
    q = capi.default_cluster_params(radius=0.25, min_size=10, max_size=5000)
    assert (q.radius, q.min_size, q.max_size, q.dry_run) == (0.25, 10, 5000, 0)
    capi.load_library().lv_default_cluster_params(None)   # (a NULL target is ignored)


def test_bad_arguments_are_refused_without_a_context(capi):
    lib = capi.load_library()
    p = capi.default_cluster_params()
    n = C.c_size_t(77)
    assert lib.lv_map_cluster(None, C.byref(p), None, None, 0, None, 0, C.byref(n)) != 0
    assert lib.lv_map_remove_clusters(None, C.byref(p), None, None, None, C.byref(n)) != 0
    assert lib.lv_map_cluster(None, None, None, None, 0, None, 0, C.byref(n)) != 0
    assert lib.lv_map_remove_clusters(None, None, None, None, None, C.byref(n)) != 0
    assert n.value == 77   # (nothing written)
