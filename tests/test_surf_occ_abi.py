"""CPU checks of lv_occ_from_surface's entry points (include/limovelo_hip.h "Occupancy from the surface"): the built library exports
them, the ctypes signatures and the struct layout capi installs agree with the header, the defaults round-trip, every parameter
outside its limits is refused before the context with its message (LV_EINVAL; the null context comes last), and
occupancy.from_surface, occupancy.surface_costmap and mesh.to_occupancy make the calls they promise on a fake context.  LV_ESTATE
without a grid or a volume needs a live context: tests/test_gpu_surf_occ.py holds it on the device, tests/test_surf_occ_state_host.py
on the host against the same VolumeTools."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_occ_surface_params", "lv_occ_from_surface")
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
    assert sorted(s for s in capi.ABI_SYMBOLS if "occ_surface" in s or "from_surface" in s) == sorted(SYMBOLS)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "lv_occ_surface_params*": C.POINTER(capi.OccSurfaceParams), "uint64_t[4]": C.POINTER(C.c_uint64)}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = p.replace("const ", "")
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*(\[4\])?$", r"\1", t).replace(" ", "")
            assert t in table, (name, p, t)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_occ_surface_params" else C.c_int)


def test_struct_layout_matches_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fields = [f for f, _ in capi.OccSurfaceParams._fields_]
    modes = ["LV_OCC_SURFACE_FILL", "LV_OCC_SURFACE_OVERWRITE", "LV_OCC_SURFACE_REPLACE", "LV_OCC_SURFACE_ACCUMULATE"]
    exprs = ["sizeof(lv_occ_surface_params)"] + [f"offsetof(lv_occ_surface_params, {f})" for f in fields] + modes
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.OccSurfaceParams)] + [getattr(capi.OccSurfaceParams, f).offset for f in fields]
    assert got == want + [capi.LV_OCC_SURFACE_FILL, capi.LV_OCC_SURFACE_OVERWRITE, capi.LV_OCC_SURFACE_REPLACE, capi.LV_OCC_SURFACE_ACCUMULATE]
    assert got[-4:] == [0, 1, 2, 3] and got[0] == 48
    assert fields == ["lo", "hi", "min_weight", "band", "reach", "mode", "l_solid", "l_open"]


def test_default_params_round_trip(capi):
    p = capi.default_occ_surface_params()
    assert (list(p.lo), list(p.hi)) == ([0, 0, 0], [1 << 30] * 3)
    assert (p.min_weight, p.band, p.reach, p.mode, p.l_solid, p.l_open) == (1, 0, 0, capi.LV_OCC_SURFACE_FILL, 3.5, -2.0)
    occ = capi.default_occupancy_params()
    assert (p.l_solid, p.l_open) == (occ.l_max, occ.l_min)   # the grid's own clamps: as sure as the grid can be
    q = capi.default_occ_surface_params(lo=(1, 2, 3), hi=(4, 5, 6), reach=2, mode=capi.LV_OCC_SURFACE_REPLACE, l_open=-0.5)
    assert (list(q.lo), list(q.hi), q.reach, q.mode, q.l_open, q.l_solid, q.min_weight) == ([1, 2, 3], [4, 5, 6], 2, 2, -0.5, 3.5, 1)
    capi.load_library().lv_default_occ_surface_params(None)   # (a null pointer is ignored)


def test_limits_are_refused_before_the_context(capi):
    lib = capi.load_library()

    def why(rc):
        assert rc == LV_EINVAL
        msg = lib.lv_last_error().decode()
        return msg

    def call(**kw):
        stats = np.full(4, 7, np.uint64)
        msg = why(lib.lv_occ_from_surface(None, C.byref(capi.default_occ_surface_params(**kw)), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        assert np.all(stats == 7)   # nothing written
        return msg

    assert call() == "null context"   # everything else holds: the context is judged last
    assert call(min_weight=1 << 18, band=4096, reach=4, mode=3) == "null context" and call(band=-4096, lo=(9, 9, 9), hi=(0, 0, 0)) == "null context"
    assert why(lib.lv_occ_from_surface(None, None, None)) == "lv_occ_from_surface: null params"
    assert call(min_weight=0) == "lv_occ_from_surface: min_weight = 0: must be in 1..2^18"
    assert call(min_weight=(1 << 18) + 1) == "lv_occ_from_surface: min_weight = 262145: must be in 1..2^18"
    assert call(band=4097) == "lv_occ_from_surface: band = 4097: must be in -4096..4096"
    assert call(band=-4097) == "lv_occ_from_surface: band = -4097: must be in -4096..4096"
    assert call(reach=-1) == "lv_occ_from_surface: reach = -1: must be in 0..4" and call(reach=5) == "lv_occ_from_surface: reach = 5: must be in 0..4"
    assert call(mode=-1) == "lv_occ_from_surface: mode = -1: must be in 0..3" and call(mode=4) == "lv_occ_from_surface: mode = 4: must be in 0..3"
    assert call(l_solid=0.0) == "lv_occ_from_surface: l_solid = 0: finite and > 0"
    assert call(l_solid=float("nan")) == "lv_occ_from_surface: l_solid = nan: finite and > 0"
    assert call(l_solid=float("inf")) == "lv_occ_from_surface: l_solid = inf: finite and > 0"
    assert call(l_open=0.0) == "lv_occ_from_surface: l_open = 0: finite and < 0"
    assert call(l_open=float("nan")) == "lv_occ_from_surface: l_open = nan: finite and < 0"
    assert call(l_solid=-1.0) == "lv_occ_from_surface: l_solid = -1: finite and > 0" and call(l_open=1.0) == "lv_occ_from_surface: l_open = 1: finite and < 0"


class _FakeCtx:
    """what occupancy.from_surface, surface_costmap and mesh.to_occupancy reach of a Context"""

    def __init__(self, capi, grid=None):
        self.capi, self.grid, self.calls = capi, grid, []
        self.volume = capi.default_tsdf_params(origin=[1.0, 2.0, 3.0], resolution=0.1, nx=40, ny=30, nz=20, min_range=0.5, max_range=9.0)

    def occ_from_surface(self, params):
        self.calls.append(("from_surface", params))
        return np.array([1, 2, 3, 4], np.uint64)

    def occ_project(self, k_lo, k_hi):
        self.calls.append(("project", k_lo, k_hi))
        return np.zeros((2, 3), np.int8)

    def occ_params(self):
        if self.grid is None:
            raise self.capi.LvError("limovelo_hip error -4: no occupancy grid: call lv_occ_configure first")
        return self.grid

    def tsdf_params(self):
        return self.volume

    def occ_configure(self, params):
        self.calls.append(("configure", params))
        self.grid = params


def test_helpers_on_a_fake_context(capi):
    from limo_velo_amd import mesh, occupancy

    ctx = _FakeCtx(capi)
    st = occupancy.from_surface(ctx)
    p = ctx.calls[-1][1]
    assert list(st) == [1, 2, 3, 4] and p.mode == capi.LV_OCC_SURFACE_FILL and list(p.hi) == [1 << 30] * 3 and p.reach == 0
    occupancy.from_surface(ctx, capi.LV_OCC_SURFACE_ACCUMULATE, box=((1, 2, 3), (4, 5, 6)), reach=2, band=64, min_weight=3, l_solid=0.9, l_open=-0.4)
    p = ctx.calls[-1][1]
    assert (p.mode, list(p.lo), list(p.hi), p.reach, p.band, p.min_weight) == (3, [1, 2, 3], [4, 5, 6], 2, 64, 3)
    assert (p.l_solid, p.l_open) == (np.float32(0.9), np.float32(-0.4))
    # surface_costmap: REPLACE over the whole grid, then the projection
    ctx.calls.clear()
    out = occupancy.surface_costmap(ctx, 2, 7, reach=1)
    assert out.shape == (2, 3) and [c[0] for c in ctx.calls] == ["from_surface", "project"] and ctx.calls[1][1:] == (2, 7)
    p = ctx.calls[0][1]
    assert p.mode == capi.LV_OCC_SURFACE_REPLACE and list(p.lo) == [0, 0, 0] and list(p.hi) == [1 << 30] * 3 and p.reach == 1
    # mesh.to_occupancy: no grid: one like the volume is configured first (the inverse of mesh.like_occupancy)
    ctx.calls.clear()
    st = mesh.to_occupancy(ctx, mode=capi.LV_OCC_SURFACE_REPLACE, reach=1)
    assert list(st) == [1, 2, 3, 4] and [c[0] for c in ctx.calls] == ["configure", "from_surface"]
    g, d = ctx.calls[0][1], capi.default_occupancy_params()
    assert ([np.float32(v) for v in g.origin], g.resolution, g.nx, g.ny, g.nz, g.min_range, g.max_range) == \
           ([np.float32(1.0), np.float32(2.0), np.float32(3.0)], np.float32(0.1), 40, 30, 20, 0.5, 9.0)
    assert (g.l_hit, g.l_miss, g.l_min, g.l_max, g.l_occ, g.l_free) == (d.l_hit, d.l_miss, d.l_min, d.l_max, d.l_occ, d.l_free)
    back = mesh.like_occupancy(g)
    assert (list(back.origin), back.resolution, back.nx, back.ny, back.nz) == (list(ctx.volume.origin), ctx.volume.resolution, 40, 30, 20)
    assert (ctx.calls[1][1].mode, ctx.calls[1][1].reach) == (capi.LV_OCC_SURFACE_REPLACE, 1)
    # ... and with a grid nothing is configured
    ctx.calls.clear()
    mesh.to_occupancy(ctx)
    assert [c[0] for c in ctx.calls] == ["from_surface"] and ctx.calls[0][1].mode == capi.LV_OCC_SURFACE_FILL
    # another error of occ_params is not swallowed

    class Broken(_FakeCtx):
        def occ_params(self):
            raise capi.LvError("limovelo_hip error -3: device lost")

    with pytest.raises(capi.LvError, match="device lost"):
        mesh.to_occupancy(Broken(capi))
