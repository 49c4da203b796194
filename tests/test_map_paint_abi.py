"""CPU checks of the map painting entry points (include/limovelo_hip.h "Map painting"): the built library exports
lv_default_paint_params / lv_map_paint, the ctypes signatures and struct layouts capi installs agree with the header, the defaults
round-trip; paint.py's chunk merge (with a fake context), save_ply and capi.camera_pose."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_paint_params", "lv_map_paint")


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
    table = {"lv_ctx*": C.c_void_p, "lv_camera_view*": C.POINTER(capi.LvCameraView), "size_t": C.c_size_t,
             "lv_paint_params*": C.POINTER(capi.LvPaintParams), "float*": C.POINTER(C.c_float), "uint8_t*": C.POINTER(C.c_uint8)}
    for name, restype in (("lv_map_paint", C.c_int), ("lv_default_paint_params", None)):
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is restype


def test_struct_layouts_and_formats_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fields_v = [f for f, _ in capi.LvCameraView._fields_]
    fields_p = [f for f, _ in capi.LvPaintParams._fields_]
    exprs = ["sizeof(lv_camera_view)"] + [f"offsetof(lv_camera_view, {f})" for f in fields_v] + ["sizeof(lv_paint_params)"] + \
            [f"offsetof(lv_paint_params, {f})" for f in fields_p] + ["LV_IMAGE_RGB8", "LV_IMAGE_BGR8", "LV_IMAGE_MONO8"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.LvCameraView)] + [getattr(capi.LvCameraView, f).offset for f in fields_v] + [C.sizeof(capi.LvPaintParams)] + \
           [getattr(capi.LvPaintParams, f).offset for f in fields_p] + [capi.LV_IMAGE_RGB8, capi.LV_IMAGE_BGR8, capi.LV_IMAGE_MONO8]
    assert got == want
    assert fields_v == ["R", "t", "fx", "fy", "cx", "cy", "dist", "width", "height", "format", "image", "row_stride"]


def test_default_params_round_trip(capi):
    p = capi.default_paint_params()
    assert (p.zbuf_scale, p.window, p.blend) == (4, 1, 0)
    assert (p.min_depth, p.max_depth, p.max_norm_radius) == (np.float32(0.3), 60.0, 1.5)
    assert abs(p.margin_abs - 0.1) < 1e-7 and abs(p.margin_rel - 0.01) < 1e-9
    q = capi.default_paint_params(zbuf_scale=1, blend=1)
    assert (q.zbuf_scale, q.blend, q.window) == (1, 1, 1)


def test_bad_arguments_are_refused_without_a_context(capi):
    lib = capi.load_library()
    p = capi.default_paint_params()
    views = (capi.LvCameraView * 1)()
    assert lib.lv_map_paint(None, views, 1, C.byref(p), None, None, None) != 0


def test_camera_view_takes_strided_rows_and_formats(capi):
    img = np.zeros((4, 8, 4), np.uint8)[:, :, :3]          # pixels 4 bytes apart: copied to packed rows
    v, keep = capi.camera_view(dict(R=np.eye(3), t=np.zeros(3), fx=1, fy=1, cx=0, cy=0, image=img))
    assert (v.width, v.height, v.format, v.row_stride) == (8, 4, capi.LV_IMAGE_RGB8, 24)
    big = np.zeros((4, 16), np.uint8)[:, :8]                # rows 16 bytes apart: passed as they are
    v, keep = capi.camera_view(dict(R=np.eye(3), t=np.zeros(3), fx=1, fy=1, cx=0, cy=0, image=big))
    assert (v.width, v.format, v.row_stride) == (8, capi.LV_IMAGE_MONO8, 16) and v.image == big.ctypes.data
    with pytest.raises(ValueError):
        capi.camera_view(dict(R=np.eye(3), t=np.zeros(3), fx=1, fy=1, cx=0, cy=0, image=big, format=capi.LV_IMAGE_BGR8))


class _FakeCtx:
    """map_paint of a fixed per-view table: view i sees point j with sample rgb[i, j] at depth z[i, j] when seen[i, j]."""

    def __init__(self, rgb, z, seen):
        self.rgb, self.z, self.seen = rgb, z, seen
        self.calls = []

    def map_paint(self, views, params):
        ids = [f["id"] for f in views]
        assert len(ids) <= 32
        self.calls.append(ids)
        s = self.seen[ids]
        n = s.sum(axis=0)
        if params.blend == 0:
            acc = np.zeros((self.rgb.shape[1], 3), np.float32)
            for i in ids:
                acc = acc + np.where(self.seen[i][:, None], self.rgb[i], 0).astype(np.float32)
            rgb = np.where(n[:, None] > 0, acc / np.maximum(n, 1)[:, None], 0).astype(np.float32)
        else:
            zz = np.where(s, self.z[ids], np.inf)
            k = np.argmin(zz, axis=0)
            rgb = np.where(n[:, None] > 0, self.rgb[np.asarray(ids)[k], np.arange(len(n))], 0).astype(np.float32)
        depth = np.min(np.where(s, self.z[ids], np.inf), axis=0).astype(np.float32)
        return rgb, depth, n.astype(np.uint8)


@pytest.mark.parametrize("blend", [0, 1])
def test_chunk_merge_equals_one_pass_over_all_views(lv, blend):
    from limo_velo_amd import capi, paint

    rng = np.random.default_rng(4)
    V, M = 75, 500
    rgb = rng.uniform(0, 255, (V, M, 3)).astype(np.float32)
    z = rng.integers(1, 4000, (V, M)).astype(np.float32) * np.float32(0.01)
    z[3, :50] = z[40, :50] = np.float32(0.001)               # exact ties across chunks: the earlier view wins
    seen = rng.uniform(size=(V, M)) < 0.3
    seen[:, :10] = False                                      # never seen
    seen[3, :50] = seen[40, :50] = True
    ctx = _FakeCtx(rgb, z, seen)
    buf = paint.VisionBuffer(V)
    for i in range(V + 5):                                    # the five oldest fall out
        buf.add(i * 0.1, np.zeros((2, 2, 3), np.uint8), np.eye(3), np.zeros(3), 1, 1, 0, 0)
    frames = [dict(f, id=i) for i, f in enumerate(buf.frames())]
    assert len(buf) == V and buf.frames()[0]["stamp"] == pytest.approx(0.5)
    p = capi.LvPaintParams(blend=blend)
    out_rgb, out_d, out_n = paint.paint(ctx, frames, p)
    assert [len(c) for c in ctx.calls] == [32, 32, 11]
    n = seen.sum(axis=0)
    assert np.array_equal(out_n, n)
    dref = np.min(np.where(seen, z, np.inf), axis=0)
    assert np.array_equal(out_d, dref.astype(np.float32))
    ok = n > 0
    if blend == 0:
        want = (np.where(seen[:, :, None], rgb.astype(np.float64), 0).sum(axis=0)[ok] / n[ok, None])
        assert np.abs(out_rgb[ok] - want).max() < 1e-3
    else:
        k = np.argmin(np.where(seen, z, np.inf), axis=0)      # first minimum: the lowest view index
        assert np.array_equal(out_rgb[ok], rgb[k, np.arange(M)][ok])
        assert np.array_equal(out_rgb[:50], rgb[3, :50])
    assert np.all(out_rgb[~ok] == 0) and np.all(np.isinf(out_d[~ok]))


def test_save_ply_round_trips(lv, tmp_path):
    from limo_velo_amd import paint

    rng = np.random.default_rng(2)
    xyz = rng.normal(size=(1000, 3)).astype(np.float32)
    rgb = rng.uniform(-10, 265, (1000, 3))
    mask = rng.uniform(size=1000) < 0.6
    path = tmp_path / "map.ply"
    paint.save_ply(path, xyz, rgb, mask)
    head = path.read_bytes()[:200].split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and f"element vertex {mask.sum()}" in head and "property uchar red" in head
    x2, c2 = paint.load_ply(path)
    assert np.array_equal(x2.view(np.uint32), xyz[mask].view(np.uint32))
    assert np.array_equal(c2, np.clip(np.rint(rgb[mask]), 0, 255).astype(np.uint8))
    assert path.stat().st_size == len(head) + len("end_header\n") + 15 * int(mask.sum())


def test_camera_pose_agrees_with_synth_quaternions(lv):
    from limo_velo_amd import capi, synth

    q = synth.quat_from_rpy(math.radians(3.0), math.radians(-7.0), math.radians(140.0))
    p = np.array([4.0, -2.5, 1.25])
    state = np.concatenate([p, q, synth.quat_from_rpy(0.1, 0.2, 0.3), [9.0, 9.0, 9.0], np.zeros(12)])
    R_IC = synth.quat_to_rot(synth.quat_from_rpy(-math.pi / 2, 0.0, -math.pi / 2))   # camera z forward = IMU x
    t_IC = np.array([0.1, -0.05, 0.2])
    R, t = capi.camera_pose(state, R_IC, t_IC)
    assert R.dtype == np.float32 and t.dtype == np.float32
    R_WI = synth.quat_to_rot(q)
    assert np.abs(R.astype(np.float64) - R_WI @ R_IC).max() < 1e-7
    assert np.abs(t.astype(np.float64) - (R_WI @ t_IC + p)).max() < 1e-6
    fwd = R.astype(np.float64) @ np.array([0.0, 0.0, 1.0])       # the optical axis is the IMU's x axis in the world
    assert np.abs(fwd - R_WI[:, 0]).max() < 1e-6
