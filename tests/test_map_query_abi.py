"""CPU checks of the map-query entry points (include/limovelo_hip.h "Map queries"): the built library exports
lv_map_knn / lv_map_radius_search / lv_map_box_search, and the ctypes signatures capi installs agree with the
header's prototypes parameter by parameter."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
QUERIES = ("lv_map_knn", "lv_map_radius_search", "lv_map_box_search")


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return c


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in limovelo_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    """The ctypes type a C parameter declaration maps to."""
    p = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*\s*(\[3\])?$", lambda m: "*" if m.group(1) else "", param.strip()).strip()
    p = p.replace("const ", "").replace(" ", "")
    table = {"lv_ctx*": C.c_void_p, "void*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "float": C.c_float,
             "uint32_t*": C.POINTER(C.c_uint32), "float*": C.POINTER(C.c_float), "int32_t*": C.POINTER(C.c_int32),
             "size_t*": C.POINTER(C.c_size_t)}
    assert p in table, (param, p)
    return table[p]


def test_library_exports_the_map_queries(capi):
    lib = capi.load_library()
    for name in QUERIES:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS


@pytest.mark.parametrize("name", QUERIES)
def test_argtypes_agree_with_the_header(capi, name):
    lib = capi.load_library()
    want = [_ctype_of(p) for p in _prototype(name)]
    got = getattr(lib, name).argtypes
    assert got is not None, f"capi sets no argtypes for {name}"
    assert len(got) == len(want), (name, got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w or (g is C.c_void_p and w is C.c_void_p), f"{name} parameter {i}: {g} vs {w}"
    assert getattr(lib, name).restype is C.c_int


def test_bad_arguments_are_refused_without_a_context(capi):
    """Argument checks come first: a null context is LV_EINVAL (or another error) and never a crash."""
    lib = capi.load_library()
    idx = (C.c_uint32 * 4)()
    assert lib.lv_map_knn(None, None, 12, 0, 5, 1.0, idx, None, None) != 0
