"""CPU checks of the colour layer's entry points (include/limovelo_hip.h "Colour layer"): the built library exports them, the
ctypes signatures and struct layouts capi installs agree with the header, the defaults round-trip, what can be judged without a
context is refused before it; mesh.py's chunking, its parameter choice and the coloured PLY."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_colour_params", "lv_colour_integrate", "lv_colour_fetch", "lv_colour_load", "lv_colour_query", "lv_colour_clear",
           "lv_colour_info", "lv_mesh_colours")
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
        assert "tsdf" not in name
    assert sorted(s for s in capi.ABI_SYMBOLS if "colour" in s) == sorted(SYMBOLS)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "lv_camera_view*": C.POINTER(capi.LvCameraView), "size_t": C.c_size_t,
             "lv_colour_params*": C.POINTER(capi.ColourParams), "structlv_colour_info*": C.POINTER(capi.ColourInfo),
             "uint64_t[4]": C.POINTER(C.c_uint64), "uint32_t*": C.POINTER(C.c_uint32), "uint8_t*": C.POINTER(C.c_uint8), "void*": C.c_void_p}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = p.replace("const ", "")
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*(\[4\])?$", r"\1", t).replace(" ", "")
            assert t in table, (name, p, t)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_colour_params" else C.c_int)


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fp = [f for f, _ in capi.ColourParams._fields_]
    fi = [f for f, _ in capi.ColourInfo._fields_]
    fm = [f for f, _ in capi.MeshInfo._fields_]
    exprs = ["sizeof(lv_colour_params)"] + [f"offsetof(lv_colour_params, {f})" for f in fp] + ["sizeof(struct lv_colour_info)"] + \
            [f"offsetof(struct lv_colour_info, {f})" for f in fi] + ["sizeof(lv_mesh_info)"] + [f"offsetof(lv_mesh_info, {f})" for f in fm]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for cls, fields in ((capi.ColourParams, fp), (capi.ColourInfo, fi), (capi.MeshInfo, fm)):
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want
    assert fp == ["view", "band", "min_weight", "max_weight", "reserved"] and fi == ["present", "reserved", "voxels", "coloured"]
    assert fm == ["built", "stale", "min_weight", "reserved", "vertices", "triangles", "active_cells", "refused_edges"]


def test_default_params_round_trip(capi):
    p = capi.default_colour_params()
    q = capi.default_paint_params()
    assert (p.view.zbuf_scale, p.view.window, p.view.blend, p.view.margin_abs) == (8, 1, 0, 0.5)
    assert (p.view.min_depth, p.view.max_depth, p.view.max_norm_radius, p.view.margin_rel) == (q.min_depth, q.max_depth, q.max_norm_radius, q.margin_rel)
    assert (p.band, p.min_weight, p.max_weight, p.reserved) == (256, 1, 64, 0)
    r = capi.default_colour_params(zbuf_scale=16, band=300, margin_abs=0.25)
    assert (r.view.zbuf_scale, r.band, r.view.margin_abs, r.max_weight, r.view.window) == (16, 300, 0.25, 64, 1)


def test_limits_are_refused_before_the_context(capi):
    lib = capi.load_library()
    img = np.zeros((4, 6, 3), np.uint8)
    view, keep = capi.camera_view(dict(R=np.eye(3), t=np.zeros(3), fx=5.0, fy=5.0, cx=2.5, cy=1.5, image=img))
    views = (capi.LvCameraView * 1)(view)

    def why(rc):
        assert rc == LV_EINVAL
        return lib.lv_last_error().decode()

    def integrate(n=1, v=views, **kw):
        return why(lib.lv_colour_integrate(None, v, n, C.byref(capi.default_colour_params(**kw)), None))

    assert integrate() == "null context"   # everything else holds: the context is judged last
    assert "blend = 1" in integrate(blend=1)
    assert "band = 0" in integrate(band=0) and "band = 4097" in integrate(band=4097)
    assert "min_weight = 0" in integrate(min_weight=0)
    assert "max_weight = 0" in integrate(max_weight=0) and "max_weight = 65536" in integrate(max_weight=65536)
    assert "n_views = 0" in integrate(n=0) and "n_views = 33" in integrate(n=33)
    assert "zbuf_scale = 17" in integrate(zbuf_scale=17) and "window = 9" in integrate(window=9)
    assert "null argument" in integrate(v=None)
    assert "null argument" in why(lib.lv_colour_integrate(None, views, 1, None, None))
    bad = (capi.LvCameraView * 1)(view)
    bad[0].image = None
    assert "null image" in integrate(v=bad)
    bad[0].image, bad[0].R[4] = view.image, float("inf")
    assert "non-finite R" in integrate(v=bad)
    buf = np.zeros(16, np.uint32)
    u32, u8 = buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.ctypes.data_as(C.POINTER(C.c_uint8))
    assert "both null" in why(lib.lv_colour_fetch(None, None, None, 4)) and why(lib.lv_colour_fetch(None, u32, None, 4)) == "null context"
    assert "null argument" in why(lib.lv_colour_load(None, None, 4)) and why(lib.lv_colour_load(None, u32, 4)) == "null context"
    assert "bad point array" in why(lib.lv_colour_query(None, buf.ctypes.data_as(C.c_void_p), 8, 1, u8))
    assert "bad point array" in why(lib.lv_colour_query(None, None, 12, 1, u8))
    assert why(lib.lv_colour_query(None, buf.ctypes.data_as(C.c_void_p), 12, 1, u8)) == "null context"
    assert "null argument" in why(lib.lv_colour_info(None, None)) and "null argument" in why(lib.lv_mesh_colours(None, None, 4))
    assert why(lib.lv_mesh_colours(None, u8, 4)) == "null context" and why(lib.lv_colour_clear(None)) == "null context"
    assert not buf.any()


class _FakeCtx:
    def __init__(self, resolution=0.2):
        self.calls = []
        self.resolution = resolution

    def colour_integrate(self, frames, params):
        self.calls.append(([f["id"] for f in frames], params))
        return np.array([10, len(frames), 2, 1], np.uint64)

    def tsdf_params(self):
        return type("P", (), dict(resolution=self.resolution))()


def test_paint_chunks_and_parameter_choice(capi):
    from limo_velo_amd import mesh

    ctx = _FakeCtx()
    p = capi.default_colour_params(band=128)
    stats = mesh.paint(ctx, [dict(id=i) for i in range(70)], p)
    assert [c[0] for c in ctx.calls] == [list(range(32)), list(range(32, 64)), list(range(64, 70))] and all(c[1] is p for c in ctx.calls)
    assert list(stats) == [30, 70, 6, 3]
    assert mesh.paint(_FakeCtx(), []).tolist() == [0, 0, 0, 0]
    for fx, nearest, res in ((400.0, 2.0, 0.2), (400.0, 9.0, 0.5), (1400.0, 1.0, 0.2), (300.0, 50.0, 0.1), (4000.0, 0.3, 0.5)):
        q = mesh.colour_params_for(_FakeCtx(res), dict(fx=fx), nearest)
        pitch = fx * res / nearest
        cover = q.view.zbuf_scale * (2 * q.view.window + 1)
        assert 1 <= q.view.zbuf_scale <= 16 and 1 <= q.view.window <= 8
        assert cover >= min(pitch, 16 * 17) and (cover < pitch + 2 * q.view.window + 1 or cover == 3)   # covers the pitch, and no more than it must
        assert q.band == 256 and q.view.margin_abs == np.float32(2.5 * res) and q.view.blend == 0


@pytest.mark.parametrize("binary", [True, False])
def test_save_ply_with_colours(lv, tmp_path, binary):
    from limo_velo_amd import mesh

    rng = np.random.default_rng(3)
    v = rng.normal(size=(50, 3)).astype(np.float32)
    t = rng.integers(0, 50, (80, 3)).astype(np.uint32)
    c = rng.integers(0, 256, (50, 4)).astype(np.uint8)
    path = tmp_path / "m.ply"
    mesh.save_ply(path, v, t, binary=binary, colours=c)
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[2:10] == ["element vertex 50", "property float x", "property float y", "property float z", "property uchar red",
                           "property uchar green", "property uchar blue", "element face 80"]
    if binary:
        assert len(body) == 50 * 15 + 80 * 13
        rec = np.frombuffer(body[:50 * 15], dtype=[("p", "<f4", 3), ("c", "u1", 3)])
        assert np.array_equal(rec["p"].view(np.uint32), v.view(np.uint32)) and np.array_equal(rec["c"], c[:, :3])
        faces = np.frombuffer(body[50 * 15:], dtype=[("n", "u1"), ("i", "<i4", 3)])
        assert np.all(faces["n"] == 3) and np.array_equal(faces["i"], t)
    else:
        rows = body.decode().strip().split("\n")
        assert len(rows) == 130
        got = np.array([r.split() for r in rows[:50]], np.float64)
        assert np.array_equal(got[:, 3:].astype(np.uint8), c[:, :3]) and np.array_equal(got[:, :3].astype(np.float32), v)
    plain = tmp_path / "plain.ply"
    mesh.save_ply(plain, v, t, binary=binary)   # the signature of before writes the file of before
    assert b"red" not in plain.read_bytes().split(b"end_header\n")[0]
    assert plain.stat().st_size < path.stat().st_size
