"""CPU checks of the localisation entry points (include/limovelo_hip.h "Localisation"): the built library exports them, the ctypes
signatures and the layout of the struct capi installs agree with the header, the defaults are as documented, and every refusal that
needs no GPU shows: every limit is judged before the context, a NULL context comes last, and a refused call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_mcl_params", "lv_occ_mcl_weigh")
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
    assert "/* ---- Localisation" in text and text.index("/* ---- Rollouts") < text.index("/* ---- Localisation") < text.index("/* ---- TSDF and mesh")
    assert capi.MCL_NO_SCORE == 2 ** 64 - 1


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "float*": C.POINTER(C.c_float), "lv_mcl_params*": C.POINTER(capi.MclParams),
             "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64), "int64_t*": C.POINTER(C.c_int64)}
    counts = {"lv_default_mcl_params": 1, "lv_occ_mcl_weigh": 11}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_mcl_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layout_matches_c(capi, tmp_path):
    assert [f for f, _ in capi.MclParams._fields_] == ["out_cost", "min_inside"]
    exprs = ["sizeof(lv_mcl_params)"] + [f"offsetof(lv_mcl_params, {f})" for f, _ in capi.MclParams._fields_]
    want = [C.sizeof(capi.MclParams)] + [getattr(capi.MclParams, f).offset for f, _ in capi.MclParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want == [8, 0, 4]


def test_default_params(capi):
    p = capi.MclParams(99, 99)
    capi.load_library().lv_default_mcl_params(C.byref(p))
    assert (p.out_cost, p.min_inside) == (0, 1)
    assert capi.default_mcl_params(out_cost=7).out_cost == 7 and capi.default_mcl_params(min_inside=0).min_inside == 0
    capi.load_library().lv_default_mcl_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    fptr, uptr = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    poses = np.zeros((4, 4), F)
    beams = np.ones((5, 3), F)
    table = np.arange(6, dtype=np.uint32)
    over = np.array([0, 1, 2 ** 24 + 1], np.uint32)
    score = np.full(4, 9, np.uint64)
    n_in = np.full(4, 9, np.uint32)
    best = np.full(2, 9, np.int64)
    X, E, T = poses.ctypes.data_as(fptr), beams.ctypes.data_as(fptr), table.ctypes.data_as(uptr)
    SC, N, BE = score.ctypes.data_as(C.POINTER(C.c_uint64)), n_in.ctypes.data_as(uptr), best.ctypes.data_as(C.POINTER(C.c_int64))

    def call(p, x=X, K=4, e=E, B=5, t=T, nt=6, sc=SC, n=N, b=BE):
        rc = lib.lv_occ_mcl_weigh(None, None if p is None else C.byref(p), x, K, e, B, t, nt, sc, n, b)
        return rc, lib.lv_last_error().decode()

    prm = capi.default_mcl_params
    # good arguments: only the context is missing
    for kw in (dict(), dict(K=0, x=None), dict(sc=None, n=None), dict(sc=None, b=None), dict(n=None, b=None), dict(K=2 ** 20, B=1024),
               dict(B=65536, K=2 ** 14), dict(nt=1), dict(p=prm(out_cost=2 ** 24, min_inside=5)), dict(p=prm(min_inside=0))):
        rc, why = call(**dict(dict(p=prm()), **kw))
        assert rc == LV_EINVAL and "null context" in why, (kw, why)
    bad = [(dict(p=None), "null params"), (dict(K=2 ** 20 + 1), "K: 0..2^20"), (dict(K=2 ** 40), "K: 0..2^20"), (dict(B=0), "B: 1..65536"),
           (dict(B=65537), "B: 1..65536"), (dict(K=2 ** 20, B=1025), "K * B"), (dict(K=2 ** 14 + 1, B=65536), "K * B"), (dict(nt=0), "n_table: 1..4096"),
           (dict(nt=4097), "n_table: 1..4096"), (dict(p=prm(out_cost=2 ** 24 + 1)), "out_cost"), (dict(p=prm(out_cost=2 ** 32 - 1)), "out_cost"),
           (dict(p=prm(min_inside=-1)), "min_inside: 0..B"), (dict(p=prm(min_inside=6)), "min_inside: 0..B"), (dict(x=None), "null poses"),
           (dict(e=None), "null beams"), (dict(t=None), "null table"), (dict(t=over.ctypes.data_as(uptr), nt=3), "table: every entry"),
           (dict(sc=None, n=None, b=None), "all null")]
    for kw, what in bad:
        rc, why = call(**dict(dict(p=prm()), **kw))
        assert rc == LV_EINVAL and what in why and "null context" not in why and why.startswith("lv_occ_mcl_weigh: "), (what, why)
    # (nothing written)
    assert np.all(score == 9) and np.all(n_in == 9) and np.all(best == 9)
