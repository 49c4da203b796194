"""CPU checks of the resident localisation filter's entry points (include/limovelo_hip.h "Resident localisation filter"): the built
library exports them, the ctypes signatures and the layouts of the structs capi installs agree with the header, the defaults are as
documented, and every refusal that needs no GPU shows: every limit is judged before the context, a NULL context comes last, and a
refused call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_mcl_resample_params", "lv_occ_mcl_filter_set", "lv_occ_mcl_filter_move", "lv_occ_mcl_filter_weigh",
           "lv_occ_mcl_filter_resample", "lv_occ_mcl_filter_get", "lv_occ_mcl_filter_info", "lv_occ_mcl_filter_clear")
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
    assert text.index("/* ---- Localisation") < text.index("/* ---- Resident localisation filter") < text.index("/* ---- TSDF and mesh")


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "float*": C.POINTER(C.c_float), "lv_mcl_params*": C.POINTER(capi.MclParams),
             "lv_mcl_resample_params*": C.POINTER(capi.MclResampleParams), "lv_mcl_filter_stats*": C.POINTER(capi.MclFilterStats),
             "lv_mcl_filter_info*": C.POINTER(capi.MclFilterInfo), "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64),
             "int64_t*": C.POINTER(C.c_int64)}
    counts = dict(zip(SYMBOLS, (1, 4, 3, 7, 6, 5, 2, 1)))
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_mcl_resample_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = (("lv_mcl_resample_params", capi.MclResampleParams), ("lv_mcl_filter_stats", capi.MclFilterStats), ("lv_mcl_filter_info", capi.MclFilterInfo))
    assert [f for f, _ in capi.MclResampleParams._fields_] == ["shift", "mode", "below_num", "below_den"]
    assert [f for f, _ in capi.MclFilterStats._fields_] == ["W", "sum_w2", "s_min", "S", "n_eligible", "n_clamped", "resampled", "epoch", "since_resample",
                                                            "origin", "resolution"]
    assert [f for f, _ in capi.MclFilterInfo._fields_] == ["K", "seed", "set", "epoch", "since_resample"]
    exprs, want = [], []
    for cname, cls in structs:
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f, _ in cls._fields_]
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want
    assert got[:5] == [16, 0, 4, 8, 12] and got[5] == 104 and got[-6:] == [32, 0, 8, 16, 20, 24]


def test_default_params(capi):
    p = capi.MclResampleParams(9, 9, 9, 9)
    capi.load_library().lv_default_mcl_resample_params(C.byref(p))
    assert (p.shift, p.mode, p.below_num, p.below_den) == (0, 1, 1, 2)
    assert capi.default_mcl_resample_params(mode=2).mode == 2 and capi.default_mcl_resample_params(shift=3).shift == 3
    capi.load_library().lv_default_mcl_resample_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    fptr, uptr = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    poses, beams = np.full((4, 4), 9, F), np.ones((5, 3), F)
    table, wtable = np.arange(6, dtype=np.uint32), np.array([4, 2, 1], np.uint32)
    over_t, over_w = np.array([0, 1, 2 ** 24 + 1], np.uint32), np.array([0, 2 ** 20 + 1], np.uint32)
    delta, sigma = np.array([0.1, 0.2, 0.1], F), np.array([0.01, 0.0, 0.01], F)
    best, anc, acc, n_in = np.full(2, 9, np.int64), np.full(4, 9, np.uint32), np.full(4, 9, np.uint64), np.full(4, 9, np.uint32)
    stats, info = capi.MclFilterStats(), capi.MclFilterInfo()
    C.memset(C.byref(stats), 9, C.sizeof(stats))
    C.memset(C.byref(info), 9, C.sizeof(info))
    X, E, T, WT = poses.ctypes.data_as(fptr), beams.ctypes.data_as(fptr), table.ctypes.data_as(uptr), wtable.ctypes.data_as(uptr)
    D, S = delta.ctypes.data_as(fptr), sigma.ctypes.data_as(fptr)
    BE, AN, AC, NI = best.ctypes.data_as(C.POINTER(C.c_int64)), anc.ctypes.data_as(uptr), acc.ctypes.data_as(C.POINTER(C.c_uint64)), n_in.ctypes.data_as(uptr)
    mp, rp = capi.default_mcl_params, capi.default_mcl_resample_params

    def f3(*v):
        a = np.array(v, F)
        return a, a.ctypes.data_as(fptr)

    def ref(p):
        return None if p is None else C.byref(p)

    calls = {
        "set": lambda x=X, K=4, seed=1: lib.lv_occ_mcl_filter_set(None, x, K, seed),
        "move": lambda d=D, s=S: lib.lv_occ_mcl_filter_move(None, d, s),
        "weigh": lambda p=mp(), e=E, B=5, t=T, nt=6, b=BE: lib.lv_occ_mcl_filter_weigh(None, ref(p), e, B, t, nt, b),
        "resample": lambda p=rp(), t=WT, nw=3, st=stats, a=AN: lib.lv_occ_mcl_filter_resample(None, ref(p), t, nw, ref(st), a),
        "get": lambda x=X, a=AC, n=NI, cap=4: lib.lv_occ_mcl_filter_get(None, x, a, n, cap),
        "info": lambda o=info: lib.lv_occ_mcl_filter_info(None, ref(o)),
        "clear": lambda: lib.lv_occ_mcl_filter_clear(None),
    }
    keep = []   # (the arrays behind the pointers)

    def arr(*v):
        keep.append(f3(*v))
        return keep[-1][1]

    # good arguments: only the context is missing
    good = [("set", {}), ("set", dict(K=1)), ("set", dict(K=2 ** 20)), ("set", dict(seed=2 ** 64 - 1)), ("move", {}), ("move", dict(s=arr(0, 0, 0))),
            ("weigh", {}), ("weigh", dict(b=None)), ("weigh", dict(B=65536)), ("weigh", dict(nt=1)), ("weigh", dict(p=mp(out_cost=2 ** 24, min_inside=5))),
            ("resample", {}), ("resample", dict(a=None)), ("resample", dict(nw=1)), ("resample", dict(p=rp(shift=63, mode=2, below_num=65536, below_den=65536))),
            ("resample", dict(p=rp(mode=0, below_num=1, below_den=1))), ("get", {}), ("get", dict(x=None, a=None)), ("get", dict(a=None, n=None)),
            ("get", dict(x=None, n=None, cap=0)), ("info", {}), ("clear", {})]
    for name, kw in good:
        rc = calls[name](**kw)
        why = lib.lv_last_error().decode()
        assert rc == LV_EINVAL and "null context" in why, (name, kw, why)
    bad = [("set", dict(K=0), "K: 1..2^20"), ("set", dict(K=2 ** 20 + 1), "K: 1..2^20"), ("set", dict(K=2 ** 40), "K: 1..2^20"), ("set", dict(x=None), "null poses"),
           ("move", dict(d=None), "null delta"), ("move", dict(s=None), "null sigma"), ("move", dict(d=arr(np.nan, 0, 0)), "delta: finite"),
           ("move", dict(d=arr(0, 0, -np.inf)), "delta: finite"), ("move", dict(s=arr(0, -1e-6, 0)), "sigma"), ("move", dict(s=arr(0, 0, np.inf)), "sigma"),
           ("move", dict(s=arr(np.nan, 0, 0)), "sigma"),
           ("weigh", dict(p=None), "null params"), ("weigh", dict(B=0), "B: 1..65536"), ("weigh", dict(B=65537), "B: 1..65536"), ("weigh", dict(nt=0), "n_table: 1..4096"),
           ("weigh", dict(nt=4097), "n_table: 1..4096"), ("weigh", dict(p=mp(out_cost=2 ** 24 + 1)), "out_cost"), ("weigh", dict(p=mp(min_inside=-1)), "min_inside: 0..B"),
           ("weigh", dict(p=mp(min_inside=6)), "min_inside: 0..B"), ("weigh", dict(e=None), "null beams"), ("weigh", dict(t=None), "null table"),
           ("weigh", dict(t=over_t.ctypes.data_as(uptr), nt=3), "table: every entry"),
           ("resample", dict(p=None), "null params"), ("resample", dict(p=rp(shift=-1)), "shift: 0..63"), ("resample", dict(p=rp(shift=64)), "shift: 0..63"),
           ("resample", dict(p=rp(mode=-1)), "mode"), ("resample", dict(p=rp(mode=3)), "mode"), ("resample", dict(p=rp(below_num=0)), "below"),
           ("resample", dict(p=rp(below_num=3, below_den=2)), "below"), ("resample", dict(p=rp(below_num=1, below_den=65537)), "below"),
           ("resample", dict(nw=0), "n_w: 1..4096"), ("resample", dict(nw=4097), "n_w: 1..4096"), ("resample", dict(t=None), "null wtable"),
           ("resample", dict(t=over_w.ctypes.data_as(uptr), nw=2), "wtable: every entry"), ("resample", dict(st=None), "null stats"),
           ("get", dict(x=None, a=None, n=None), "all null"), ("info", dict(o=None), "null argument")]
    for name, kw, what in bad:
        rc = calls[name](**kw)
        why = lib.lv_last_error().decode()
        assert rc == LV_EINVAL and what in why and "null context" not in why and why.startswith(f"lv_occ_mcl_filter_{name}: "), (name, what, why)
    # (nothing written)
    assert np.all(best == 9) and np.all(anc == 9) and np.all(acc == 9) and np.all(n_in == 9) and np.all(poses == 9)
    assert bytes(stats) == b"\x09" * C.sizeof(stats) and bytes(info) == b"\x09" * C.sizeof(info)
