"""CPU checks of the planner's entry points (include/limovelo_hip.h "Planner"): the built library exports them, the ctypes
signatures and the layout of both structs capi installs agree with the header, the defaults are as documented, and every refusal
that needs no GPU shows: lv_occ_plan_build judges parameters, table and counts and lv_occ_plan_fetch its outputs before the
context, every call refuses a NULL context, and a refused call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_plan_params", "lv_occ_plan_build", "lv_occ_plan_fetch", "lv_occ_plan_paths", "lv_occ_plan_info", "lv_occ_plan_clear")
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
    assert capi.LV_PLAN_UNREACHED == 0xFFFFFFFF and re.search(r"#define\s+LV_PLAN_UNREACHED\s+0xFFFFFFFFu\b", open(HEADER).read())


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "lv_plan_params*": C.POINTER(capi.PlanParams), "lv_plan_info*": C.POINTER(capi.PlanInfo),
             "void*": C.c_void_p, "uint8_t*": C.POINTER(C.c_uint8), "int32_t*": C.POINTER(C.c_int32), "uint32_t*": C.POINTER(C.c_uint32),
             "uint64_t*": C.POINTER(C.c_uint64), "size_t*": C.POINTER(C.c_size_t)}
    counts = {"lv_default_plan_params": 1, "lv_occ_plan_build": 8, "lv_occ_plan_fetch": 4, "lv_occ_plan_paths": 10, "lv_occ_plan_info": 2,
              "lv_occ_plan_clear": 1}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = p.replace("stats[4]", "*stats")   # (uint64_t stats[4] is a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_plan_params" else C.c_int)
        assert len(want) == counts[name]
    # the CSR convention and types of lv_map_radius_search: offsets, capacity and total
    radius = _prototype("lv_map_radius_search")
    paths = _prototype("lv_occ_plan_paths")
    assert paths[6] == radius[5] == "size_t* offsets" and paths[8:] == radius[8:] == ["size_t capacity", "size_t* total"]


def test_struct_layouts_match_c(capi, tmp_path):
    pf = [f for f, _ in capi.PlanParams._fields_]
    inf = [f for f, _ in capi.PlanInfo._fields_]
    assert pf == ["connectivity", "min_clear_s2"]
    assert inf == ["built", "planar", "nx", "ny", "nz", "stale", "rounds", "params"]
    exprs = (["sizeof(lv_plan_params)"] + [f"offsetof(lv_plan_params, {f})" for f in pf] + ["sizeof(lv_plan_info)"] +
             [f"offsetof(lv_plan_info, {f})" for f in inf] + ["LV_PLAN_UNREACHED"])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = ([C.sizeof(capi.PlanParams)] + [getattr(capi.PlanParams, f).offset for f in pf] + [C.sizeof(capi.PlanInfo)] +
            [getattr(capi.PlanInfo, f).offset for f in inf] + [capi.LV_PLAN_UNREACHED])
    assert got == want


def test_default_params(capi):
    p = capi.PlanParams(99, 99)
    capi.load_library().lv_default_plan_params(C.byref(p))
    assert (p.connectivity, p.min_clear_s2) == (8, 1)
    q = capi.default_plan_params(connectivity=26, min_clear_s2=5)
    assert (q.connectivity, q.min_clear_s2) == (26, 5)
    capi.load_library().lv_default_plan_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    goals = np.zeros((65537, 3), np.float32)
    gp = goals.ctypes.data_as(C.c_void_p)
    u8 = C.POINTER(C.c_uint8)

    def refused(table, n_cost=None, n_goals=1, gptr=gp, stride=12, **kw):
        p = capi.default_plan_params(**kw)
        t = np.asarray(table, np.uint8)
        rc = lib.lv_occ_plan_build(None, C.byref(p), t.ctypes.data_as(u8), len(t) if n_cost is None else n_cost, gptr, stride, n_goals, stats)
        return rc, lib.lv_last_error().decode()

    ones = np.ones(1026, np.uint8)
    for kw in (dict(), dict(connectivity=4), dict(connectivity=6), dict(connectivity=18), dict(connectivity=26), dict(min_clear_s2=3 * 1023 ** 2)):
        for table, n_goals in (([1], 1), (ones[:1025], 65536), ([255, 1, 50], 5)):
            rc, why = refused(table, n_goals=n_goals, **kw)
            assert rc == LV_EINVAL and "null context" in why, (kw, why)   # (good arguments: only the context is missing)
    bad = [(dict(connectivity=0), {}, "connectivity"), (dict(connectivity=5), {}, "connectivity"), (dict(connectivity=27), {}, "connectivity"),
           (dict(min_clear_s2=0), {}, "min_clear_s2"), (dict(min_clear_s2=-4), {}, "min_clear_s2"), (dict(min_clear_s2=3 * 1023 ** 2 + 1), {}, "min_clear_s2"),
           ({}, dict(n_cost=0), "n_cost"), ({}, dict(table=ones, n_cost=1026), "n_cost"), ({}, dict(table=[50, 0, 50]), "every entry"),
           ({}, dict(n_goals=0), "n_goals"), ({}, dict(n_goals=65537), "n_goals"), ({}, dict(gptr=None), "goal array"),
           ({}, dict(stride=8), "goal array")]
    for kw, args, what in bad:
        args = dict(dict(table=[50, 60]), **args)
        rc, why = refused(args.pop("table"), **args, **kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, args, why)
    t = np.ones(4, np.uint8)
    assert lib.lv_occ_plan_build(None, None, t.ctypes.data_as(u8), 4, gp, 12, 1, stats) == LV_EINVAL and "null params" in lib.lv_last_error().decode()
    p = capi.default_plan_params()
    assert lib.lv_occ_plan_build(None, C.byref(p), None, 4, gp, 12, 1, stats) == LV_EINVAL and "null cost table" in lib.lv_last_error().decode()
    assert lib.lv_occ_plan_fetch(None, None, None, 8) == LV_EINVAL and "both null" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7]


def test_a_null_context_is_refused_by_every_call(capi):
    lib = capi.load_library()
    p = capi.default_plan_params()
    info = capi.PlanInfo(5, 5, 5, 5, 5, 5, 5)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    pot = (C.c_uint32 * 1)(3)
    cc = (C.c_uint8 * 1)(4)
    table = (C.c_uint8 * 2)(50, 60)
    pts = (C.c_float * 3)(0.0, 0.0, 0.0)
    status = (C.c_int32 * 1)(9)
    cost = (C.c_uint32 * 1)(9)
    off = (C.c_size_t * 2)(9, 9)
    cells = (C.c_int32 * 4)(9, 9, 9, 9)
    total = C.c_size_t(9)
    for rc in (lib.lv_occ_plan_build(None, C.byref(p), table, 2, pts, 12, 1, stats), lib.lv_occ_plan_fetch(None, pot, cc, 1),
               lib.lv_occ_plan_fetch(None, pot, None, 1), lib.lv_occ_plan_fetch(None, None, cc, 1),
               lib.lv_occ_plan_paths(None, pts, 12, 1, status, cost, off, None, 0, C.byref(total)),
               lib.lv_occ_plan_paths(None, pts, 12, 1, status, cost, off, cells, 4, C.byref(total)),
               lib.lv_occ_plan_info(None, C.byref(info)), lib.lv_occ_plan_clear(None)):
        assert rc == LV_EINVAL and "null context" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7] and pot[0] == 3 and cc[0] == 4 and info.built == 5 and info.rounds == 5   # (nothing written)
    assert status[0] == 9 and cost[0] == 9 and list(off) == [9, 9] and list(cells) == [9] * 4 and total.value == 9
