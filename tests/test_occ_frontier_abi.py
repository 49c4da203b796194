"""CPU checks of the frontier entry points (include/limovelo_hip.h "Frontiers"): the built library exports them, the ctypes
signatures and the layout of the three structs capi installs agree with the header (lv_frontier_cluster is 72 bytes), the defaults
are as documented, and every refusal that needs no GPU shows: parameters are judged before the context, every call refuses a NULL
context, and a refused call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_frontier_params", "lv_occ_frontier_build", "lv_occ_frontier_fetch", "lv_occ_frontier_clusters", "lv_occ_frontier_rank",
           "lv_occ_frontier_info", "lv_occ_frontier_clear")
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
    assert capi.LV_FRONTIER_NONE == -1 and re.search(r"#define\s+LV_FRONTIER_NONE\s+\(-1\)", open(HEADER).read())


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "lv_frontier_params*": C.POINTER(capi.FrontierParams),
             "lv_frontier_info*": C.POINTER(capi.FrontierInfo), "lv_frontier_cluster*": C.POINTER(capi.FrontierCluster),
             "int32_t*": C.POINTER(C.c_int32), "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64), "size_t*": C.POINTER(C.c_size_t)}
    counts = {"lv_default_frontier_params": 1, "lv_occ_frontier_build": 3, "lv_occ_frontier_fetch": 3, "lv_occ_frontier_clusters": 4,
              "lv_occ_frontier_rank": 5, "lv_occ_frontier_info": 2, "lv_occ_frontier_clear": 1}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = p.replace("stats[4]", "*stats")   # (uint64_t stats[4] is a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_frontier_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = [("lv_frontier_params", capi.FrontierParams), ("lv_frontier_info", capi.FrontierInfo), ("lv_frontier_cluster", capi.FrontierCluster)]
    assert [f for f, _ in capi.FrontierParams._fields_] == ["planar", "k_lo", "k_hi", "connectivity", "min_size"]
    assert [f for f, _ in capi.FrontierInfo._fields_] == ["built", "planar", "nx", "ny", "nz", "stale", "n_clusters", "params"]
    assert [f for f, _ in capi.FrontierCluster._fields_] == ["size", "first", "rep", "centre", "lo", "hi", "sum"]
    exprs, want = [], []
    for cname, t in structs:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(t))
        for f, _ in t._fields_:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(t, f).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + 'printf("%d\\n", LV_FRONTIER_NONE);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want + [-1]
    assert C.sizeof(capi.FrontierCluster) == 72 and capi.FRONTIER_CLUSTER_DTYPE.itemsize == 72
    assert [capi.FRONTIER_CLUSTER_DTYPE.fields[f][1] for f, _ in capi.FrontierCluster._fields_] == [0, 4, 8, 12, 24, 36, 48]
    assert [getattr(capi.FrontierCluster, f).offset for f, _ in capi.FrontierCluster._fields_] == [0, 4, 8, 12, 24, 36, 48]


def test_default_params(capi):
    p = capi.FrontierParams(99, 99, 99, 99, 99)
    capi.load_library().lv_default_frontier_params(C.byref(p))
    assert (p.planar, p.k_lo, p.k_hi, p.connectivity, p.min_size) == (0, 0, 0, 26, 1)
    q = capi.default_frontier_params(planar=1, connectivity=8, min_size=5)
    assert (q.planar, q.connectivity, q.min_size) == (1, 8, 5)
    capi.load_library().lv_default_frontier_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)

    def refused(**kw):
        p = capi.default_frontier_params(**kw)
        return lib.lv_occ_frontier_build(None, C.byref(p), stats), lib.lv_last_error().decode()

    for kw in (dict(), dict(connectivity=6), dict(connectivity=18), dict(planar=1, connectivity=4), dict(planar=1, connectivity=8, k_lo=3, k_hi=3),
               dict(min_size=2 ** 28), dict(k_lo=5, k_hi=1), dict(planar=1, connectivity=8, k_lo=-9, k_hi=2000)):
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and "null context" in why, (kw, why)   # (good arguments: only the context is missing)
    bad = [(dict(connectivity=0), "connectivity"), (dict(connectivity=5), "connectivity"), (dict(connectivity=27), "connectivity"),
           (dict(connectivity=8), "connectivity"), (dict(connectivity=4), "connectivity"), (dict(planar=1, connectivity=6), "connectivity"),
           (dict(planar=1, connectivity=18), "connectivity"), (dict(planar=1), "connectivity"), (dict(min_size=0), "min_size"),
           (dict(min_size=-3), "min_size"), (dict(min_size=2 ** 28 + 1), "min_size"), (dict(planar=1, connectivity=8, k_lo=2, k_hi=1), "k_lo")]
    for kw, what in bad:
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, why)
    assert lib.lv_occ_frontier_build(None, None, stats) == LV_EINVAL and "null params" in lib.lv_last_error().decode()
    bp = (C.c_uint32 * 1)(3)
    bc = (C.c_int32 * 1)(4)
    for reach in (9, -1, 100):
        assert lib.lv_occ_frontier_rank(None, reach, bp, bc, 1) == LV_EINVAL and "reach" in lib.lv_last_error().decode()
    assert lib.lv_occ_frontier_rank(None, 0, None, None, 1) == LV_EINVAL and "both null" in lib.lv_last_error().decode()
    assert lib.lv_occ_frontier_fetch(None, None, 8) == LV_EINVAL and "null labels" in lib.lv_last_error().decode()
    assert lib.lv_occ_frontier_clusters(None, None, 0, None) == LV_EINVAL and "null count" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7] and bp[0] == 3 and bc[0] == 4


def test_a_null_context_is_refused_by_every_call(capi):
    lib = capi.load_library()
    p = capi.default_frontier_params()
    info = capi.FrontierInfo(5, 5, 5, 5, 5, 5, 5)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    labels = (C.c_int32 * 2)(3, 3)
    cl = np.full(2, 9, np.uint8).repeat(72).view(capi.FRONTIER_CLUSTER_DTYPE)
    clp = cl.ctypes.data_as(C.POINTER(capi.FrontierCluster))
    n = C.c_size_t(9)
    bp = (C.c_uint32 * 2)(3, 3)
    bc = (C.c_int32 * 2)(4, 4)
    for rc in (lib.lv_occ_frontier_build(None, C.byref(p), stats), lib.lv_occ_frontier_build(None, C.byref(p), None),
               lib.lv_occ_frontier_fetch(None, labels, 2), lib.lv_occ_frontier_clusters(None, None, 0, C.byref(n)),
               lib.lv_occ_frontier_clusters(None, clp, 2, C.byref(n)), lib.lv_occ_frontier_rank(None, 0, bp, bc, 2),
               lib.lv_occ_frontier_rank(None, 8, bp, None, 2), lib.lv_occ_frontier_rank(None, 8, None, bc, 2),
               lib.lv_occ_frontier_info(None, C.byref(info)), lib.lv_occ_frontier_clear(None)):
        assert rc == LV_EINVAL and "null context" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7] and list(labels) == [3, 3] and n.value == 9 and list(bp) == [3, 3] and list(bc) == [4, 4]   # (nothing written)
    assert info.built == 5 and info.n_clusters == 5 and np.all(cl.view(np.uint8) == 9)
