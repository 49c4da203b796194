"""CPU checks of the lattice planner's entry points (include/limovelo_hip.h "Lattice planner"): the built library exports them, the
ctypes signatures and the layout of the three structs capi installs agree with the header, the defaults are as documented, and every
refusal that needs no GPU shows: lv_occ_lattice_build judges parameters, table and counts before the context and names the record
it refuses, every call refuses a NULL context, and a refused call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lattice_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_lattice_params", "lv_occ_lattice_build", "lv_occ_lattice_fetch", "lv_occ_lattice_paths", "lv_occ_lattice_info",
           "lv_occ_lattice_clear")
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
    src = open(HEADER).read()
    for name, value in (("LV_LATTICE_REACH", "8"), ("LV_LATTICE_MAX_SWEEP", "10"), ("LV_LATTICE_UNREACHED", "0xFFFFFFFFu")):
        assert re.search(r"#define\s+" + name + r"\s+" + value + r"\b", src)
    assert (capi.LV_LATTICE_REACH, capi.LV_LATTICE_MAX_SWEEP, capi.LV_LATTICE_UNREACHED) == (8, 10, 0xFFFFFFFF)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "lv_lattice_params*": C.POINTER(capi.LatticeParams), "lv_lattice_info*": C.POINTER(capi.LatticeInfo),
             "lv_lattice_prim*": C.POINTER(capi.LatticePrim), "void*": C.c_void_p, "uint8_t*": C.POINTER(C.c_uint8), "int32_t*": C.POINTER(C.c_int32),
             "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64), "size_t*": C.POINTER(C.c_size_t)}
    counts = {"lv_default_lattice_params": 1, "lv_occ_lattice_build": 8, "lv_occ_lattice_fetch": 3, "lv_occ_lattice_paths": 11, "lv_occ_lattice_info": 2,
              "lv_occ_lattice_clear": 1}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = p.replace("stats[4]", "*stats")   # (uint64_t stats[4] is a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_lattice_params" else C.c_int)
        assert len(want) == counts[name]
    # the CSR convention of lv_occ_plan_paths, with the primitives beside the states
    plan, lat = _prototype("lv_occ_plan_paths"), _prototype("lv_occ_lattice_paths")
    assert lat[:7] == plan[:7] and lat[7:9] == ["int32_t* states", "uint8_t* prims"] and lat[9:] == plan[8:]


def test_struct_layouts_match_c(capi, tmp_path):
    rf = [f for f, _ in capi.LatticePrim._fields_]
    pf = [f for f, _ in capi.LatticeParams._fields_]
    inf = [f for f, _ in capi.LatticeInfo._fields_]
    assert rf == ["di", "dj", "h_to", "n_sweep", "length", "reserved", "penalty", "sweep"] and pf == ["H", "P"]
    assert inf == ["built", "nx", "ny", "H", "P", "stale", "rounds", "tile", "reach", "params"]
    exprs = (["sizeof(lv_lattice_prim)"] + [f"offsetof(lv_lattice_prim, {f})" for f in rf] + ["sizeof(lv_lattice_params)"] +
             [f"offsetof(lv_lattice_params, {f})" for f in pf] + ["sizeof(lv_lattice_info)"] + [f"offsetof(lv_lattice_info, {f})" for f in inf])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = ([C.sizeof(capi.LatticePrim)] + [getattr(capi.LatticePrim, f).offset for f in rf] + [C.sizeof(capi.LatticeParams)] +
            [getattr(capi.LatticeParams, f).offset for f in pf] + [C.sizeof(capi.LatticeInfo)] + [getattr(capi.LatticeInfo, f).offset for f in inf])
    assert got == want and got[0] == 32
    # the numpy records: the same bytes, and the reference's
    assert capi.LATTICE_PRIM_DTYPE == lr.PRIM_DTYPE and capi.LATTICE_POSE_DTYPE == lr.POSE_DTYPE
    assert [capi.LATTICE_PRIM_DTYPE.fields[f][1] for f in rf] == [getattr(capi.LatticePrim, f).offset for f in rf]


def test_default_params(capi):
    p = capi.LatticeParams(99, 99)
    capi.load_library().lv_default_lattice_params(C.byref(p))
    assert (p.H, p.P) == (16, 3)
    q = capi.default_lattice_params(H=8, P=5)
    assert (q.H, q.P) == (8, 5)
    capi.load_library().lv_default_lattice_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    goals = np.zeros(65537, capi.LATTICE_POSE_DTYPE)
    gp = goals.ctypes.data_as(C.c_void_p)

    def refused(t, H=2, P=2, n_prims=None, n_goals=1, gptr=gp, stride=16, tptr=True):
        p = capi.LatticeParams(H, P)
        t = np.ascontiguousarray(t)
        rc = lib.lv_occ_lattice_build(None, C.byref(p), t.ctypes.data_as(C.POINTER(capi.LatticePrim)) if tptr else None, t.size if n_prims is None else n_prims,
                                      gptr, stride, n_goals, stats)
        return rc, lib.lv_last_error().decode()

    good = lr.table(2, 2)
    good[0, 0] = lr.prim(1, 0, 0, 10, 0, [(1, 0)])
    for n_goals in (1, 65536):
        rc, why = refused(good, n_goals=n_goals)
        assert rc == LV_EINVAL and "null context" in why   # (good arguments: only the context is missing)
    full = lr.table(16, 16)
    full[:, :] = lr.prim(8, -8, 15, 65535, 1 << 24, [(8, -8)] * 10)
    rc, why = refused(full, H=16, P=16)
    assert rc == LV_EINVAL and "null context" in why
    bad = [(dict(H=0), "H:"), (dict(H=17), "H:"), (dict(P=0), "P:"), (dict(P=17), "P:"), (dict(tptr=False), "null primitive table"), (dict(n_prims=3), "n_prims"),
           (dict(n_goals=0), "n_goals"), (dict(n_goals=65537), "n_goals"), (dict(gptr=None), "goal array"), (dict(stride=12), "goal array")]
    for kw, what in bad:
        rc, why = refused(good, **kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, why)
    rc, why = refused(lr.table(2, 2))
    assert rc == LV_EINVAL and "no non-empty record" in why
    for field, value, what in (("di", 9, "di, dj"), ("dj", -9, "di, dj"), ("h_to", 2, "h_to"), ("n_sweep", 11, "n_sweep"), ("reserved", 1, "reserved"),
                               ("penalty", (1 << 24) + 1, "penalty")):
        t = good.copy()
        t[1, 0][field] = value
        rc, why = refused(t)
        assert rc == LV_EINVAL and "record 2 (heading 1, primitive 0)" in why and what in why and "null context" not in why, (field, why)
    t = good.copy()
    t[1, 1] = lr.prim(0, 0, 1, 10)
    rc, why = refused(t)
    assert rc == LV_EINVAL and "record 3 (heading 1, primitive 1)" in why and "self loop" in why
    t[1, 1] = lr.prim(0, 0, 0, 10)   # a turn on the spot is allowed
    assert "null context" in refused(t)[1]
    p = capi.LatticeParams(2, 2)
    assert lib.lv_occ_lattice_build(None, None, good.ctypes.data_as(C.POINTER(capi.LatticePrim)), 4, gp, 16, 1, stats) == LV_EINVAL
    assert "null params" in lib.lv_last_error().decode()
    assert lib.lv_occ_lattice_fetch(None, None, 8) == LV_EINVAL and "null V" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7]


def test_a_null_context_is_refused_by_every_call(capi):
    lib = capi.load_library()
    p = capi.LatticeParams(1, 1)
    info = capi.LatticeInfo(5, 5, 5, 5, 5, 5, 5, 5, 5)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    t = lr.table(1, 1)
    t[0, 0] = lr.prim(1, 0, 0, 10)
    V = (C.c_uint32 * 1)(3)
    pose = np.zeros(1, capi.LATTICE_POSE_DTYPE)
    pp = pose.ctypes.data_as(C.c_void_p)
    status, cost, off = (C.c_int32 * 1)(9), (C.c_uint32 * 1)(9), (C.c_size_t * 2)(9, 9)
    states, taken, total = (C.c_int32 * 4)(9, 9, 9, 9), (C.c_uint8 * 4)(9, 9, 9, 9), C.c_size_t(9)
    for rc in (lib.lv_occ_lattice_build(None, C.byref(p), t.ctypes.data_as(C.POINTER(capi.LatticePrim)), 1, pp, 16, 1, stats), lib.lv_occ_lattice_fetch(None, V, 1),
               lib.lv_occ_lattice_paths(None, pp, 16, 1, status, cost, off, None, None, 0, C.byref(total)),
               lib.lv_occ_lattice_paths(None, pp, 16, 1, status, cost, off, states, taken, 4, C.byref(total)),
               lib.lv_occ_lattice_info(None, C.byref(info)), lib.lv_occ_lattice_clear(None)):
        assert rc == LV_EINVAL and "null context" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7] and V[0] == 3 and info.built == 5 and info.reach == 5   # (nothing written)
    assert status[0] == 9 and cost[0] == 9 and list(off) == [9, 9] and list(states) == [9] * 4 and list(taken) == [9] * 4 and total.value == 9
