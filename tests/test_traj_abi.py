"""CPU checks of the trajectory entry points (include/limovelo_hip.h "Trajectory"): the built library exports them, the ctypes
signatures and record layouts capi installs agree with the header (sizes and offsets against a compiled C program), the defaults,
and the refusals that need no GPU: every call judges its arguments before the context, so a null context shows every LV_EINVAL
path; "null context" itself comes last.  (LV_ESTATE needs a context and so a GPU: tests/test_gpu_traj.py::test_states.)"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import traj_cases as cases
import traj_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_traj_smooth_params", "lv_default_traj_register_params", "lv_traj_set", "lv_traj_fetch", "lv_traj_get_info", "lv_traj_clear",
           "lv_traj_sample", "lv_traj_smooth", "lv_traj_correct", "lv_traj_register", "lv_traj_register_cloud")
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
    m = re.search(r"\b(int|void|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in limovelo_hip.h"
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_library_exports_the_symbols(capi):
    lib = capi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "void*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "double": C.c_double,
             "lv_traj_knot*": C.POINTER(capi.TrajKnot), "lv_traj_info*": C.POINTER(capi.TrajInfo),
             "lv_traj_smooth_params*": C.POINTER(capi.TrajSmoothParams), "lv_traj_register_params*": C.POINTER(capi.TrajRegisterParams),
             "lv_graph_pose*": C.POINTER(capi.GraphPose), "uint8_t*": C.POINTER(C.c_uint8), "uint64_t*": C.POINTER(C.c_uint64),
             "size_t*": C.POINTER(C.c_size_t), "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float)}

    def ctype(p):
        p = re.sub(r"\[\d*\]$", "*", p.replace("const ", ""))                  # an array parameter is a pointer
        p = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*(\*?)$", r"\1", p)                # drop the parameter's name
        return table[p.replace(" ", "")]

    for name in SYMBOLS:
        rtype, params = _prototype(name)
        want = [ctype(p) for p in params]
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if rtype == "void" else C.c_int), name


def test_layouts_match_c(capi, tmp_path):
    records = {"lv_traj_knot": (capi.TrajKnot, capi.TRAJ_KNOT_DTYPE, 64), "lv_traj_smooth_params": (capi.TrajSmoothParams, None, 24),
               "lv_traj_register_params": (capi.TrajRegisterParams, None, 72), "lv_traj_info": (capi.TrajInfo, None, 64)}
    exprs, want = [], []
    for cname, (ct, dt, size) in records.items():
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(ct))
        assert C.sizeof(ct) == size and (dt is None or dt.itemsize == size)
        for f, _ in ct._fields_:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(ct, f).offset)
            if dt is not None:
                assert dt.fields[f][1] == getattr(ct, f).offset, (cname, f)
    assert tr.KNOT_DTYPE == capi.TRAJ_KNOT_DTYPE
    consts = {"LV_TRAJ_MAX_KNOTS": capi.TRAJ_MAX_KNOTS, "LV_TRAJ_INSIDE": capi.TRAJ_INSIDE, "LV_TRAJ_BEFORE": capi.TRAJ_BEFORE,
              "LV_TRAJ_AFTER": capi.TRAJ_AFTER, "LV_TRAJ_NONFINITE": capi.TRAJ_NONFINITE, "LV_TRAJ_CLAMP": capi.TRAJ_CLAMP,
              "LV_TRAJ_REFUSE": capi.TRAJ_REFUSE, "LV_TRAJ_WORLD": capi.TRAJ_WORLD, "LV_TRAJ_FRAME_AT": capi.TRAJ_FRAME_AT}
    exprs += list(consts)
    want += list(consts.values())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want
    assert (capi.TRAJ_INSIDE, capi.TRAJ_BEFORE, capi.TRAJ_AFTER, capi.TRAJ_NONFINITE) == (tr.INSIDE, tr.BEFORE, tr.AFTER, tr.NONFINITE) == (0, 1, 2, 3)
    assert (capi.TRAJ_CLAMP, capi.TRAJ_REFUSE, capi.TRAJ_WORLD, capi.TRAJ_FRAME_AT) == (tr.CLAMP, tr.REFUSE, tr.WORLD, tr.FRAME_AT) == (0, 1, 0, 1)
    tile = re.search(r"constexpr uint32_t TRAJ_TILE = (\d+);", open(os.path.join(ROOT, "limo-velo_amd", "csrc", "lv_traj.hpp")).read())
    assert int(tile.group(1)) == capi.TRAJ_TILE == tr.TILE


def test_defaults(capi):
    s = capi.default_traj_smooth_params()
    assert (s.sigma, s.half_window, s.iterations, s.pin_ends) == (0.1, 8, 1, 1)
    assert capi.default_traj_smooth_params(sigma=0.5, iterations=3).iterations == 3
    r = capi.default_traj_register_params()
    assert (r.extrapolate, r.frame, list(r.ext_t), list(r.ext_q), r.frame_time) == (capi.TRAJ_CLAMP, capi.TRAJ_WORLD, [0, 0, 0], [0, 0, 0, 1], 0.0)
    r = capi.default_traj_register_params(extrapolate=capi.TRAJ_REFUSE, ext_t=(1, 2, 3), frame=capi.TRAJ_FRAME_AT, frame_time=4.5)
    assert (r.extrapolate, list(r.ext_t), r.frame, r.frame_time) == (1, [1, 2, 3], 1, 4.5)
    k = capi.traj_knots([0.0, 1.0], [[1, 2, 3, 0, 0, 0, 1], [4, 5, 6, 0, 0, 1, 0]])
    assert k.dtype == capi.TRAJ_KNOT_DTYPE and list(k["time"]) == [0, 1] and list(k["t"][1]) == [4, 5, 6] and list(k["q"][1]) == [0, 0, 1, 0]


def _knots(capi, times, poses):
    k = np.ascontiguousarray(capi.traj_knots(times, poses))
    return k, k.ctypes.data_as(C.POINTER(capi.TrajKnot))


def test_set_and_correct_judge_the_records_before_the_context(capi):
    lib = capi.load_library()
    times, poses = cases.wander(12, seed=3)
    for fn, what in ((lib.lv_traj_set, "trajectory"), (lib.lv_traj_correct, "correction")):
        k, p = _knots(capi, times, poses)
        assert fn(None, p, len(k)) == LV_EINVAL and lib.lv_last_error().decode() == "null context"   # good records: only the context is missing

        def refused(change, *words, n=None, null=False):
            t, x = times.copy(), poses.copy()
            change(t, x)
            k, p = _knots(capi, t, x)
            rc, why = fn(None, None if null else p, len(k) if n is None else n), lib.lv_last_error().decode()
            assert rc == LV_EINVAL and why.startswith(what) and all(w in why for w in words) and "null context" not in why, (words, why)

        refused(lambda t, x: t.__setitem__(4, math.nan), "knot 4", "time", "non-finite")
        refused(lambda t, x: x.__setitem__((9, 1), math.inf), "knot 9", "t:", "non-finite")
        refused(lambda t, x: x.__setitem__((3, 5), math.nan), "knot 3", "q:", "non-finite")
        refused(lambda t, x: x.__setitem__((6, slice(3, 7)), x[6, 3:] * (1 + 2e-6)), "knot 6", "q:", "norm")
        refused(lambda t, x: t.__setitem__(5, t[4]), "knot 5", "time", "not above")
        refused(lambda t, x: None, "n = 0", n=0)
        refused(lambda t, x: None, "2^20", n=(1 << 20) + 1)
        refused(lambda t, x: None, "null knots", null=True)


def test_other_calls_judge_their_arguments_before_the_context(capi):
    lib = capi.load_library()

    def why():
        return lib.lv_last_error().decode()

    for kw, word in ((dict(sigma=0.0), "sigma"), (dict(sigma=math.nan), "sigma"), (dict(half_window=0), "half_window"), (dict(half_window=65), "half_window"),
                     (dict(iterations=-1), "iterations"), (dict(iterations=101), "iterations")):
        p = capi.default_traj_smooth_params(**kw)
        assert lib.lv_traj_smooth(None, C.byref(p), None) == LV_EINVAL and word in why()
    assert lib.lv_traj_smooth(None, None, None) == LV_EINVAL and "null params" in why()
    assert lib.lv_traj_fetch(None, None, 4) == LV_EINVAL and "null knots" in why()
    assert lib.lv_traj_get_info(None, None) == LV_EINVAL and "null info" in why()
    t = np.zeros(2)
    T = t.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.lv_traj_sample(None, T, 2, 2, None, None) == LV_EINVAL and "extrapolate" in why()
    assert lib.lv_traj_sample(None, None, 2, 0, None, None) == LV_EINVAL and "null times" in why()
    assert lib.lv_traj_sample(None, T, (1 << 28) + 1, 0, None, None) == LV_EINVAL and "2^28" in why()
    pts = np.zeros(2, capi.POINT_DTYPE)
    P = pts.ctypes.data_as(C.c_void_p)

    def reg(prm=None, pts=P, stride=32, toff=16, n=2):
        return lib.lv_traj_register(None, None if prm is None else C.byref(prm), pts, stride, toff, n, None, None, None)

    for kw, word in ((dict(extrapolate=2), "extrapolate"), (dict(frame=2), "frame"), (dict(ext_t=(0, math.nan, 0)), "ext_t"),
                     (dict(ext_q=(0, 0, 0, math.inf)), "ext_q"), (dict(ext_q=(0, 0, 0, 1.00001)), "norm"),
                     (dict(frame=capi.TRAJ_FRAME_AT, frame_time=math.nan), "frame_time")):
        prm = capi.default_traj_register_params(**kw)
        assert reg(prm) == LV_EINVAL and word in why() and "null context" not in why()
        n = C.c_size_t(0)
        assert lib.lv_traj_register_cloud(None, C.byref(prm), 0.0, 1.0, None, None, 0, C.byref(n), None) == LV_EINVAL and word in why()
    assert reg(pts=None) == LV_EINVAL and "null points" in why()
    assert reg(stride=23) == LV_EINVAL and "stride" in why()
    assert reg(toff=8) == LV_EINVAL and "time_offset" in why()
    assert reg(n=(1 << 28) + 1) == LV_EINVAL and "2^28" in why()
    assert lib.lv_traj_register_cloud(None, None, 0.0, 1.0, None, None, 0, None, None) == LV_EINVAL and "null n" in why()
    info, n = capi.TrajInfo(), C.c_size_t(0)
    k, p = _knots(capi, *cases.wander(3))
    s = capi.default_traj_smooth_params()
    for rc in (reg(), reg(pts=None, n=0), lib.lv_traj_register_cloud(None, None, 0.0, 1.0, None, None, 0, C.byref(n), None),
               lib.lv_traj_sample(None, T, 2, 0, None, None), lib.lv_traj_smooth(None, C.byref(s), None), lib.lv_traj_clear(None),
               lib.lv_traj_get_info(None, C.byref(info)), lib.lv_traj_fetch(None, p, 3)):
        assert rc == LV_EINVAL and why() == "null context"


def test_offline_py_records(capi):
    """limo_velo_amd.offline without a context: the knots of recorded states and the corrections of a solved graph."""
    from limo_velo_amd import graph as pg, offline, synth
    import graph_ref as gr

    times, poses = cases.wander(6, seed=2)
    states = [synth.make_state(p[:3], p[3:]) for p in poses]
    rec = offline.Recorder()
    for t, s in zip(times, states):
        rec.add_state(t, s)
    k = rec.trajectory()
    assert k.dtype == capi.TRAJ_KNOT_DTYPE and np.array_equal(k["time"], times) and np.allclose(k["t"], poses[:, :3], atol=0)
    assert np.abs(np.abs(np.sum(k["q"] * poses[:, 3:], axis=1)) - 1.0).max() <= 1e-15
    assert np.array_equal(offline.trajectory(states, times), k)
    with pytest.raises(ValueError):
        rec.add_state(times[-1], states[-1])          # times must ascend
    G = pg.PoseGraph()
    for s in states[::2]:
        G.add_keyframe(s)
    moved = np.array([pg._pose(s) for s in states[::2]])
    moved[2, :3] += [0.5, -0.25, 0.125]
    moved[2, 3:] = tr.normalise(gr.qmul(gr.qexp(np.array([0.0, 0.0, 0.1])), moved[2, 3:]))
    G.poses = moved
    D = offline.corrections(G, times[::2])
    assert D.dtype == capi.TRAJ_KNOT_DTYPE and np.array_equal(D["time"], times[::2])
    assert np.array_equal(D["t"][:2], np.zeros((2, 3))) and np.array_equal(D["q"][:2], np.tile([0, 0, 0, 1.0], (2, 1)))   # not moved: the identity, exactly
    got = tr.correct(times, poses, np.array(D["time"]), np.concatenate([D["t"], D["q"]], axis=1))
    assert tr.pose_distance(got[4:5], moved[2:3]) <= 1e-12 and np.array_equal(got[:3], poses[:3])
