"""CPU checks of lv_surf_merge's entry points (include/limovelo_hip.h "Submap merging"): the built library exports them, the
ctypes signatures and the struct layouts capi installs agree with the header, the defaults round-trip, every argument outside its
limits is refused before the context with its message (LV_EINVAL, nothing written; the null context comes last), and mesh.submap,
mesh.merge and mesh.Submaps make the calls they promise on a fake context.  LV_ESTATE before lv_tsdf_configure and the resolution
ratio need a live context: tests/test_gpu_surf_merge.py holds them on the device, tests/test_surf_merge_state_host.py on the host
against the same VolumeTools."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_surf_merge_params", "lv_surf_merge")
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
        assert not any(w in name for w in ("tsdf", "depth", "colour"))   # (those sets of names are closed: their own ABI tests)
    assert sorted(s for s in capi.ABI_SYMBOLS if "merge" in s) == sorted(SYMBOLS)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "lv_surf_submap*": C.POINTER(capi.SurfSubmap), "lv_graph_pose*": C.POINTER(capi.GraphPose),
             "lv_surf_merge_params*": C.POINTER(capi.SurfMergeParams), "uint64_t[4]": C.POINTER(C.c_uint64)}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = p.replace("const ", "")
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*(\[4\])?$", r"\1", t).replace(" ", "")
            assert t in table, (name, p, t)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_surf_merge_params" else C.c_int)


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    structs = {"lv_surf_submap": capi.SurfSubmap, "lv_surf_merge_params": capi.SurfMergeParams, "lv_graph_pose": capi.GraphPose}
    exprs, want = [], []
    for cname, s in structs.items():
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(s))
        for f, _ in s._fields_:
            exprs.append(f"offsetof({cname}, {f})")
            want.append(getattr(s, f).offset)
    exprs += ["LV_MERGE_TRILINEAR", "LV_MERGE_NEAREST"]
    want += [capi.LV_MERGE_TRILINEAR, capi.LV_MERGE_NEAREST]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want and got[-2:] == [0, 1]
    assert (C.sizeof(capi.SurfSubmap), C.sizeof(capi.SurfMergeParams), C.sizeof(capi.GraphPose)) == (48, 16, 56)
    assert [f for f, _ in capi.SurfSubmap._fields_] == ["origin", "resolution", "nx", "ny", "nz", "trunc_cells", "S", "W"]
    assert [f for f, _ in capi.SurfMergeParams._fields_] == ["min_weight", "interp", "reserved"]


def test_default_params_round_trip(capi):
    p = capi.default_surf_merge_params()
    assert (p.min_weight, p.interp, list(p.reserved)) == (1, capi.LV_MERGE_TRILINEAR, [0, 0])
    q = capi.default_surf_merge_params(min_weight=4, interp=capi.LV_MERGE_NEAREST)
    assert (q.min_weight, q.interp) == (4, 1)
    capi.load_library().lv_default_surf_merge_params(None)   # (a null pointer is ignored)


def test_arguments_are_refused_before_the_context(capi):
    lib = capi.load_library()
    T = 3 * 256

    def call(pose=(0, 0, 0, 0, 0, 0, 1), prm=None, S=None, W=None, null=(), **kw):
        geo = dict(origin=(0.0, 0.0, 0.0), resolution=0.2, trunc_cells=3)
        shape = kw.pop("shape", (2, 3, 4))
        geo.update(kw)
        m, keep = capi.surf_submap(geo["origin"], geo["resolution"], geo["trunc_cells"], np.zeros(shape, np.int32) if S is None else S,
                                   np.ones(shape, np.int32) if W is None else W)
        for f in ("nx", "ny", "nz"):
            if f in kw:
                setattr(m, f, kw[f])
        if "S" in null:
            m.S = None
        if "W" in null:
            m.W = None
        g = np.asarray(pose, np.float64)
        stats = np.full(4, 7, np.uint64)
        rc = lib.lv_surf_merge(None, None if "sub" in null else C.byref(m), None if "pose" in null else g.ctypes.data_as(C.POINTER(capi.GraphPose)),
                               C.byref(prm) if prm is not None else None, stats.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == LV_EINVAL and np.all(stats == 7)   # nothing written
        return lib.lv_last_error().decode()

    P = capi.default_surf_merge_params
    full = np.full((2, 3, 4), 1 << 18, np.int32)
    # everything holds: the context is judged last (params NULL: the defaults)
    assert call() == "null context" and call(prm=P(min_weight=1 << 18, interp=1)) == "null context"
    assert call(W=full, S=(T * full.astype(np.int64)).astype(np.int32), trunc_cells=3) == "null context" and call(W=np.zeros((2, 3, 4), np.int32)) == "null context"
    assert call(trunc_cells=16, shape=(1, 1, 1024)) == "null context" and call(pose=(1e9, -5, 2, 0.5, 0.5, 0.5, 0.5)) == "null context"
    assert call(null=("sub",)) == "lv_surf_merge: null argument" and call(null=("pose",)) == "lv_surf_merge: null argument"
    assert call(origin=(0.0, float("nan"), 0.0)) == "lv_surf_merge: submap origin: must be finite"
    assert call(resolution=0.0) == "lv_surf_merge: submap resolution = 0: finite and > 0"
    assert call(resolution=float("inf")) == "lv_surf_merge: submap resolution = inf: finite and > 0"
    assert call(nx=0) == "lv_surf_merge: submap of 0 x 3 x 2 voxels: each must be in 1..1024"
    assert call(nz=1025) == "lv_surf_merge: submap of 4 x 3 x 1025 voxels: each must be in 1..1024"
    assert call(nx=1024, ny=1024, nz=257) == "lv_surf_merge: submap of 1024 x 1024 x 257 voxels: at most 2^28"
    assert call(trunc_cells=0) == "lv_surf_merge: submap trunc_cells = 0: must be in 1..16"
    assert call(trunc_cells=17) == "lv_surf_merge: submap trunc_cells = 17: must be in 1..16"
    assert call(null=("S",)) == "lv_surf_merge: null S or W" and call(null=("W",)) == "lv_surf_merge: null S or W"
    assert call(pose=(0, float("inf"), 0, 0, 0, 0, 1)) == "lv_surf_merge: pose: t: a non-finite number"
    assert call(pose=(0, 0, 0, 0, float("nan"), 0, 1)) == "lv_surf_merge: pose: q: a non-finite number"
    assert call(pose=(0, 0, 0, 0, 0, 0, 1.00001)) == "lv_surf_merge: pose: q: norm off 1 by more than 1e-6"
    assert call(pose=(0, 0, 0, 0, 0, 0, 0)) == "lv_surf_merge: pose: q: norm off 1 by more than 1e-6"
    assert call(prm=P(min_weight=0)) == "lv_surf_merge: min_weight = 0: at least 1"
    assert call(prm=P(interp=2)) == "lv_surf_merge: interp = 2: LV_MERGE_TRILINEAR or LV_MERGE_NEAREST"
    assert call(prm=P(interp=-1)) == "lv_surf_merge: interp = -1: LV_MERGE_TRILINEAR or LV_MERGE_NEAREST"
    W = np.ones((2, 3, 4), np.int32)
    W[1, 2, 3] = -1
    assert call(W=W) == "lv_surf_merge: submap voxel 23: S = 0, W = -1: 0 <= W <= 2^18 and |S| <= T * W"
    W[1, 2, 3] = (1 << 18) + 1
    assert call(W=W) == "lv_surf_merge: submap voxel 23: S = 0, W = 262145: 0 <= W <= 2^18 and |S| <= T * W"
    S = np.zeros((2, 3, 4), np.int32)
    S[0, 0, 2] = -T - 1
    assert call(S=S) == "lv_surf_merge: submap voxel 2: S = -769, W = 1: 0 <= W <= 2^18 and |S| <= T * W"
    # the order: the submap's grid, its arrays, the pose, the parameters, the voxels
    assert call(nx=0, null=("S",), pose=(0,) * 7, prm=P(min_weight=0), W=W).startswith("lv_surf_merge: submap of 0 x")
    assert call(null=("S",), pose=(0,) * 7, prm=P(min_weight=0), W=W) == "lv_surf_merge: null S or W"
    assert call(pose=(0,) * 7, prm=P(min_weight=0), W=W).startswith("lv_surf_merge: pose: q")
    assert call(prm=P(min_weight=0), W=W).startswith("lv_surf_merge: min_weight")


class _FakeCtx:
    """what mesh.submap, mesh.merge and mesh.Submaps reach of a Context"""

    def __init__(self, capi):
        self.capi, self.calls = capi, []
        self.volume = capi.default_tsdf_params(origin=[1.0, 2.0, 3.0], resolution=0.1, nx=4, ny=3, nz=2, trunc_cells=5)

    def tsdf_params(self):
        return self.volume

    def tsdf_fetch(self, S=True, W=True, metres=False):
        return dict(S=np.arange(24, dtype=np.int32).reshape(2, 3, 4), W=np.full((2, 3, 4), 2, np.int32))

    def tsdf_clear(self):
        self.calls.append(("clear",))

    def surf_merge(self, submap, pose, params):
        n = submap.nx * submap.ny * submap.nz
        self.calls.append(("merge", [float(v) for v in submap.origin], float(submap.resolution), (submap.nz, submap.ny, submap.nx), submap.trunc_cells,
                           np.ctypeslib.as_array(submap.S, (n,)).copy(), np.ctypeslib.as_array(submap.W, (n,)).copy(), np.array(pose), params.min_weight, params.interp))
        return np.array([4, 3, 2, 1], np.uint64)


def test_helpers_on_a_fake_context(capi, tmp_path):
    from limo_velo_amd import mesh

    ctx = _FakeCtx(capi)
    m = mesh.submap(ctx)
    assert (list(m["origin"]), m["resolution"], m["trunc_cells"], m["S"].shape) == ([1.0, 2.0, 3.0], np.float32(0.1), 5, (2, 3, 4))
    st = mesh.merge(ctx, m, ([1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 1.0]))
    c = ctx.calls[-1]
    assert list(st) == [4, 3, 2, 1] and c[1:5] == ([1.0, 2.0, 3.0], float(np.float32(0.1)), (2, 3, 4), 5)
    assert np.array_equal(c[5], np.arange(24)) and np.all(c[6] == 2) and list(c[7]) == [1, 2, 3, 0, 0, 0, 1] and c[8:] == (1, capi.LV_MERGE_TRILINEAR)
    # a 4 x 4 matrix: a quarter turn about z
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [5, 6, 7]
    mesh.merge(ctx, m, T, min_weight=3, nearest=True)
    c = ctx.calls[-1]
    assert np.allclose(c[7], [5, 6, 7, 0, 0, np.sqrt(0.5), np.sqrt(0.5)]) and c[8:] == (3, capi.LV_MERGE_NEAREST)
    # Submaps: add, save, load, fuse = clear and then one merge per submap in order
    subs = mesh.Submaps()
    m2 = dict(m, S=m["S"] + 1, origin=np.array([0.5, 0.25, 0.0], np.float32), trunc_cells=2)
    assert subs.add(m, T) == 0 and subs.add(m2, np.arange(7.0) / 10) == 1 and len(subs) == 2
    subs.save(str(tmp_path / "run"))
    back = mesh.Submaps.load(str(tmp_path / "run"))
    assert len(back) == 2 and np.array_equal(back.poses, subs.poses)
    for a, b in zip(back.submaps, subs.submaps):
        assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["W"], b["W"]) and a["S"].dtype == np.int32
        assert np.array_equal(a["origin"], b["origin"]) and a["resolution"] == b["resolution"] and a["trunc_cells"] == b["trunc_cells"]
    ctx.calls.clear()
    st = back.fuse(ctx)
    assert list(st) == [8, 6, 4, 2] and [c[0] for c in ctx.calls] == ["clear", "merge", "merge"]
    assert np.allclose(ctx.calls[1][7], subs.poses[0]) and ctx.calls[2][1] == [0.5, 0.25, 0.0] and ctx.calls[2][4] == 2
    new = [np.array([1.0, 1.0, 1.0, 0, 0, 0, 1]), ([2.0, 2.0, 2.0], [0, 0, 0, 1.0])]
    ctx.calls.clear()
    back.fuse(ctx, poses=new, min_weight=2)
    assert list(ctx.calls[1][7]) == [1, 1, 1, 0, 0, 0, 1] and list(ctx.calls[2][7]) == [2, 2, 2, 0, 0, 0, 1] and ctx.calls[2][8] == 2
    with pytest.raises(ValueError):
        back.fuse(ctx, poses=new[:1])
