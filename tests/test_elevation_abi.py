"""CPU checks of the elevation map's entry points (include/limovelo_hip.h "Elevation map"): the built library exports them, the
ctypes signatures and the layout of the two structs capi installs agree with the header, the defaults are the documented ones
(and what terrain.params_from_metres derives from metres and degrees), and every refusal that needs no GPU shows,
lv_occ_distance_build_cells included: arguments are judged before the context, every call refuses a NULL context, and a refused
call writes nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_elevation_params", "lv_elev_build", "lv_elev_fetch", "lv_elev_query", "lv_elev_info", "lv_elev_clear",
           "lv_occ_distance_build_cells")
LAYERS = ("LV_ELEV_LO", "LV_ELEV_TOP", "LV_ELEV_SPAN", "LV_ELEV_STEP", "LV_ELEV_SLOPE2", "LV_ELEV_COUNT", "LV_ELEV_BAND_COUNT", "LV_ELEV_CLASS",
          "LV_ELEV_HEIGHT")
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
    for value, name in enumerate(LAYERS):
        assert getattr(capi, name) == value and re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text)
    assert capi.LV_ELEV_NONE == 2 ** 31 - 1 and re.search(r"#define\s+LV_ELEV_NONE\s+2147483647\b", text)
    assert "/* ---- Elevation map" in text and text.index("/* ---- Elevation map") > text.index("/* ---- Ray casting")
    assert [n for n, _ in capi.ELEV_LAYERS] == ["lo", "top", "span", "step", "slope2", "count", "band_count", "cls", "height"]
    assert [np.dtype(t).itemsize for _, t in capi.ELEV_LAYERS] == [4, 4, 4, 4, 4, 4, 4, 1, 4]


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "void*": C.c_void_p, "int": C.c_int, "float*": C.POINTER(C.c_float),
             "int8_t*": C.POINTER(C.c_int8), "uint64_t": C.POINTER(C.c_uint64),   # (uint64_t stats[4]: a pointer)
             "lv_elevation_params*": C.POINTER(capi.ElevationParams), "lv_elevation_info*": C.POINTER(capi.ElevationInfo),
             "lv_distance_params*": C.POINTER(capi.DistanceParams)}
    counts = {"lv_default_elevation_params": 1, "lv_elev_build": 6, "lv_elev_fetch": 4, "lv_elev_query": 6, "lv_elev_info": 2, "lv_elev_clear": 1,
              "lv_occ_distance_build_cells": 5}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = re.sub(r"\[\d*\]$", "", p)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_elevation_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = [("lv_elevation_params", capi.ElevationParams), ("lv_elevation_info", capi.ElevationInfo)]
    assert [f for f, _ in capi.ElevationParams._fields_] == ["origin", "resolution", "nx", "ny", "min_points", "head", "max_span", "max_step",
                                                            "max_slope2"]
    assert [f for f, _ in capi.ElevationInfo._fields_] == ["built", "nx", "ny", "from_map", "n_points", "params"]
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
                   'printf("%d\\n", LV_ELEV_NONE);' + "".join(f'printf("%d\\n", {n});' for n in LAYERS) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want + [2 ** 31 - 1] + list(range(9))
    assert C.sizeof(capi.ElevationParams) == 44 and C.sizeof(capi.ElevationInfo) == 72 and capi.ElevationInfo.n_points.offset == 16


def test_default_params(capi):
    from limo_velo_amd import terrain

    p = capi.ElevationParams()
    C.memset(C.byref(p), 0x55, C.sizeof(p))
    capi.load_library().lv_default_elevation_params(C.byref(p))
    o = capi.default_occupancy_params()
    assert [F(v) for v in p.origin] == [F(-51.2), F(-51.2), F(-3.2)] == [F(v) for v in o.origin]
    assert (F(p.resolution), p.nx, p.ny) == (F(0.2), 512, 512) == (F(o.resolution), o.nx, o.ny)
    assert (p.min_points, p.head, p.max_span, p.max_step, p.max_slope2) == (3, 1920, 153, 128, 34727)
    # the documented conversions: floor(m / res * 256), floor((512 tan 20 deg)^2)
    assert [int(np.floor(m / 0.2 * 256)) for m in (1.5, 0.12, 0.10)] == [1920, 153, 128]
    assert int(np.floor((512 * np.tan(np.radians(20.0))) ** 2)) == 34727
    q = terrain.params_from_metres()
    assert bytes(q) == bytes(p)
    q = terrain.params_from_metres(origin=(1, 2, 3), resolution=0.5, nx=19, ny=13, robot_height=2.0, max_step=0.25, max_span=0.3, max_slope_deg=45.0,
                                   min_points=7)
    assert ([v for v in q.origin], q.resolution, q.nx, q.ny, q.min_points, q.head, q.max_span, q.max_step) == ([1, 2, 3], 0.5, 19, 13, 7, 1024, 153, 128)
    assert q.max_slope2 in (512 ** 2 - 1, 512 ** 2) and terrain.slope2_of(0.0) == 0 and terrain.slope2_of(89.9999999) == 2 ** 31 - 1
    assert capi.default_elevation_params(nx=7, origin=(1, 2, 3)).nx == 7
    capi.load_library().lv_default_elevation_params(None)   # (a NULL target is ignored)
    assert terrain.sub_units(1.5, float(F(0.2))) == 1920   # (the resolution as lv_occupancy_params holds it)


def test_build_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    pts = np.ones((4, 3), F)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)

    def call(p, a, stride, n, st=stats):
        rc = lib.lv_elev_build(None, C.byref(p) if p is not None else None, a, stride, n, st)
        return rc, lib.lv_last_error().decode()

    good = capi.default_elevation_params()
    A = pts.ctypes.data_as(C.c_void_p)
    for args in ((good, A, 12, 4), (good, A, 12, 0), (good, None, 0, 0), (good, None, 3, 2 ** 40),   # (a NULL array: stride and n are not looked at)
                 (capi.default_elevation_params(nx=4096, ny=4096, min_points=2 ** 20, head=2 ** 25, max_span=0, max_step=2 ** 25, max_slope2=2 ** 31 - 1), A, 40, 4),
                 (good, A, 12, 2 ** 31 - 2)):
        rc, why = call(*args)
        assert rc == LV_EINVAL and "null context" in why, (args, why)   # (good arguments: only the context is missing)
    rc, why = call(good, A, 12, 4, None)
    assert rc == LV_EINVAL and "null context" in why
    d = capi.default_elevation_params
    bad = [((None, A, 12, 4), "null params"), ((d(nx=0), A, 12, 4), "nx, ny"), ((d(nx=4097), A, 12, 4), "nx, ny"), ((d(ny=-1), A, 12, 4), "nx, ny"),
           ((d(resolution=0.0), A, 12, 4), "resolution"), ((d(resolution=float("nan")), A, 12, 4), "resolution"),
           ((d(resolution=float("inf")), A, 12, 4), "resolution"), ((d(origin=(0.0, float("inf"), 0.0)), A, 12, 4), "origin"),
           ((d(origin=(0.0, 0.0, float("nan"))), A, 12, 4), "origin"), ((d(min_points=0), A, 12, 4), "min_points"),
           ((d(min_points=2 ** 20 + 1), A, 12, 4), "min_points"), ((d(head=-1), A, 12, 4), "head"), ((d(head=2 ** 25 + 1), A, 12, 4), "head"),
           ((d(max_span=-1), A, 12, 4), "max_span"), ((d(max_span=2 ** 25 + 1), A, 12, 4), "max_span"), ((d(max_step=-1), A, 12, 4), "max_step"),
           ((d(max_step=2 ** 25 + 1), A, 12, 4), "max_step"), ((d(max_slope2=-1), A, 12, 4), "max_slope2"),
           ((good, A, 11, 4), "stride 11"), ((good, A, 0, 0), "stride 0"), ((good, A, 12, 2 ** 31 - 1), "too many"), ((good, A, 12, 2 ** 40), "too many")]
    for args, what in bad:
        rc, why = call(*args)
        assert rc == LV_EINVAL and what in why and "lv_elev_build" in why and "null context" not in why, (what, why)
    assert list(stats) == [7] * 4   # (nothing written)


def test_fetch_query_info_clear_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    out = np.full(16, 9, np.uint8)
    O = out.ctypes.data_as(C.c_void_p)

    def err():
        return lib.lv_last_error().decode()

    for layer in range(9):
        assert lib.lv_elev_fetch(None, layer, O, 4) == LV_EINVAL and "null context" in err()
    for layer in (-1, 9, 100, -2 ** 31):
        assert lib.lv_elev_fetch(None, layer, O, 4) == LV_EINVAL and "layer" in err() and "null context" not in err()
    assert lib.lv_elev_fetch(None, 0, None, 4) == LV_EINVAL and "null output" in err()
    pts = np.ones((2, 3), F)
    h = np.full(2, 9, np.uint8).repeat(4).view(F)
    k = np.full(2, 9, np.int8)
    A, H, K = pts.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.POINTER(C.c_float)), k.ctypes.data_as(C.POINTER(C.c_int8))
    for args in ((A, 12, 2, H, K), (A, 12, 2, None, K), (A, 12, 2, H, None), (A, 40, 1, H, K), (None, 0, 0, H, K), (A, 12, 2 ** 31 - 2, H, K)):
        assert lib.lv_elev_query(None, *args) == LV_EINVAL and "null context" in err(), args
    for args, what in (((A, 12, 2, None, None), "both null"), ((None, 12, 2, H, K), "bad point array"), ((A, 11, 2, H, K), "stride 11"),
                       ((A, 12, 2 ** 31 - 1, H, K), "too many"), ((None, 0, 0, None, None), "both null")):
        assert lib.lv_elev_query(None, *args) == LV_EINVAL and what in err() and "null context" not in err(), what
    info = capi.ElevationInfo()
    C.memset(C.byref(info), 0x33, C.sizeof(info))
    assert lib.lv_elev_info(None, C.byref(info)) == LV_EINVAL and "null context" in err()
    assert lib.lv_elev_info(None, None) == LV_EINVAL and "null argument" in err()
    assert lib.lv_elev_clear(None) == LV_EINVAL and "null context" in err()
    assert np.all(out == 9) and np.all(h.view(np.uint8) == 9) and np.all(k == 9) and bytes(info) == b"\x33" * C.sizeof(info)   # (nothing written)


def test_distance_from_cells_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    cells = np.zeros(12, np.int8)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    Cp = cells.ctypes.data_as(C.POINTER(C.c_int8))

    def call(p, c, n, st=stats):
        rc = lib.lv_occ_distance_build_cells(None, C.byref(p) if p is not None else None, c, n, st)
        return rc, lib.lv_last_error().decode()

    d = capi.default_distance_params
    for args in ((d(planar=1), Cp, 12), (d(planar=7, k_lo=5, k_hi=-5, max_cells=1024, signed_field=1, unknown_is_obstacle=1), Cp, 12),   # (k_lo, k_hi are not used)
                 (d(planar=1), Cp, 0), (d(planar=1), Cp, 2 ** 40)):   # (the size is judged against the configured grid)
        rc, why = call(*args)
        assert rc == LV_EINVAL and "null context" in why, why
    assert call(d(planar=1), Cp, 12, None)[1] == "null context"
    for args, what in (((None, Cp, 12), "null params"), ((d(), Cp, 12), "planar"), ((d(planar=0, k_lo=0, k_hi=3), Cp, 12), "planar"),
                       ((d(planar=1), None, 12), "null cells"), ((d(planar=1, max_cells=-1), Cp, 12), "max_cells"),
                       ((d(planar=1, max_cells=1025), Cp, 12), "max_cells")):
        rc, why = call(*args)
        assert rc == LV_EINVAL and what in why and "lv_occ_distance_build_cells" in why and "null context" not in why, (what, why)
    assert list(stats) == [7] * 4 and not cells.any()
