"""CPU checks of the rollout entry points (include/limovelo_hip.h "Rollouts"): the built library exports them, the ctypes signatures
and the layout of the two structs capi installs agree with the header (lv_rollout_result is 32 bytes), the defaults are as
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
SYMBOLS = ("lv_default_rollout_params", "lv_occ_rollout")
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
    for name, value in (("LV_ROLLOUT_CLEAR", 1), ("LV_ROLLOUT_STOPPED", 2)):
        assert getattr(capi, name) == value and re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text)
    assert "/* ---- Rollouts" in text and text.index("/* ---- Elevation map") < text.index("/* ---- Rollouts") < text.index("/* ---- Localizator side")


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "float*": C.POINTER(C.c_float), "lv_rollout_params*": C.POINTER(capi.RolloutParams),
             "lv_rollout_result*": C.POINTER(capi.RolloutResult), "uint64_t*": C.POINTER(C.c_uint64), "int64_t*": C.POINTER(C.c_int64)}
    counts = {"lv_default_rollout_params": 1, "lv_occ_rollout": 11}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_rollout_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = [("lv_rollout_params", capi.RolloutParams), ("lv_rollout_result", capi.RolloutResult)]
    assert [f for f, _ in capi.RolloutParams._fields_] == ["T", "Tc", "dt", "fp_clear_s2", "w_cost", "w_goal", "w_stop", "min_steps", "goal_mode"]
    assert [f for f, _ in capi.RolloutResult._fields_] == ["status", "steps", "why", "cell_end", "p_end", "p_min", "s_min", "cost_sum"]
    exprs, want = [], []
    for cname, t in structs:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(t))
        for f, _ in t._fields_:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(t, f).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) +
                   'printf("%d %d\\n", LV_ROLLOUT_CLEAR, LV_ROLLOUT_STOPPED);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want + [1, 2]
    assert C.sizeof(capi.RolloutResult) == 32 and capi.ROLLOUT_RESULT_DTYPE.itemsize == 32 and C.sizeof(capi.RolloutParams) == 36
    assert [getattr(capi.RolloutResult, f).offset for f, _ in capi.RolloutResult._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [capi.ROLLOUT_RESULT_DTYPE.fields[f][1] for f, _ in capi.RolloutResult._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [capi.ROLLOUT_RESULT_DTYPE.fields[f][0] for f, _ in capi.RolloutResult._fields_] == [np.int32] * 4 + [np.uint32] * 2 + [np.int32, np.uint32]


def test_default_params(capi):
    p = capi.RolloutParams(*([99] * 9))
    capi.load_library().lv_default_rollout_params(C.byref(p))
    assert (p.T, p.Tc, p.fp_clear_s2, p.w_cost, p.w_goal, p.w_stop, p.min_steps, p.goal_mode) == (32, 1, 1, 1, 1, 0, 1, 0)
    assert F(p.dt) == F(0.1)
    assert capi.default_rollout_params(T=7, goal_mode=1).T == 7
    capi.load_library().lv_default_rollout_params(None)   # (a NULL target is ignored)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    fptr = C.POINTER(C.c_float)
    start = np.zeros(3, F)
    u = np.zeros((4, 3, 2), F)
    fp = np.ones((5, 2), F)
    res = np.full(4 * 32, 9, np.uint8).view(capi.ROLLOUT_RESULT_DTYPE)
    poses = np.full((4, 7, 3), 9.0, F)
    score = np.full(4, 9, np.uint64)
    best = np.full(2, 9, np.int64)
    S, U, FP = start.ctypes.data_as(fptr), u.ctypes.data_as(fptr), fp.ctypes.data_as(fptr)
    R, PO = res.ctypes.data_as(C.POINTER(capi.RolloutResult)), poses.ctypes.data_as(fptr)
    SC, B = score.ctypes.data_as(C.POINTER(C.c_uint64)), best.ctypes.data_as(C.POINTER(C.c_int64))

    def call(p, s=S, c=U, K=4, f=FP, n_fp=5, r=R, po=PO, sc=SC, b=B):
        rc = lib.lv_occ_rollout(None, None if p is None else C.byref(p), s, c, K, f, n_fp, r, po, sc, b)
        return rc, lib.lv_last_error().decode()

    def prm(**kw):
        return capi.default_rollout_params(**dict(dict(T=6, Tc=3), **kw))

    # good arguments: only the context is missing
    for kw in (dict(), dict(K=0, c=None), dict(f=None, n_fp=0), dict(r=None, po=None, sc=None), dict(r=None, po=None, b=None), dict(n_fp=64),
               dict(K=2 ** 20, po=None), dict(K=2 ** 21 // 7)):
        rc, why = call(prm(), **kw)
        assert rc == LV_EINVAL and "null context" in why, (kw, why)
    for p in (prm(T=1024, Tc=1024), prm(T=1, Tc=1, min_steps=1), prm(fp_clear_s2=3 * 1023 ** 2), prm(w_cost=65535, w_goal=65535, w_stop=65535),
              prm(min_steps=6, goal_mode=1), prm(min_steps=0), prm(dt=1e-30), prm(dt=3e38)):
        rc, why = call(p)
        assert rc == LV_EINVAL and "null context" in why, why
    bad = [(dict(p=None), "null params"), (dict(p=prm(T=0)), "T: 1..1024"), (dict(p=prm(T=1025)), "T: 1..1024"), (dict(p=prm(Tc=0)), "Tc: 1..T"),
           (dict(p=prm(Tc=7)), "Tc: 1..T"), (dict(p=prm(dt=0.0)), "dt"), (dict(p=prm(dt=-0.1)), "dt"), (dict(p=prm(dt=float("nan"))), "dt"),
           (dict(p=prm(dt=float("inf"))), "dt"), (dict(p=prm(), n_fp=65), "n_fp: 0..64"), (dict(p=prm(), f=None), "null footprint"),
           (dict(p=prm(fp_clear_s2=0)), "fp_clear_s2"), (dict(p=prm(fp_clear_s2=3 * 1023 ** 2 + 1)), "fp_clear_s2"),
           (dict(p=prm(min_steps=-1)), "min_steps: 0..T"), (dict(p=prm(min_steps=7)), "min_steps: 0..T"), (dict(p=prm(goal_mode=2)), "goal_mode"),
           (dict(p=prm(goal_mode=-1)), "goal_mode"), (dict(p=prm(w_cost=65536)), "weights"), (dict(p=prm(w_goal=2 ** 32 - 1)), "weights"),
           (dict(p=prm(w_stop=65536)), "weights"), (dict(p=prm(), K=2 ** 20 + 1), "K: 0..2^20"), (dict(p=prm(), K=2 ** 40), "K: 0..2^20"),
           (dict(p=prm(T=64, Tc=17), K=2 ** 20), "K * Tc"), (dict(p=prm(T=16, Tc=1), K=2 ** 20), "K * (T + 1)"),
           (dict(p=prm(), s=None), "null start"), (dict(p=prm(), c=None), "null controls"),
           (dict(p=prm(), r=None, po=None, sc=None, b=None), "all null")]
    for kw, what in bad:
        rc, why = call(**kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why and why.startswith("lv_occ_rollout: "), (what, why)
    # (nothing written)
    assert np.all(res.view(np.uint8) == 9) and np.all(poses == 9.0) and np.all(score == 9) and np.all(best == 9)
