"""CPU checks of the TSDF's entry points (include/limovelo_hip.h "TSDF and mesh"): the built library exports them, the ctypes
signatures and the struct layouts capi installs agree with the header and a compiled C program, the defaults are as documented, and
lv_tsdf_configure refuses every parameter outside its limits before it looks at the context (so the refusal and its precedence
show without a GPU: lv_last_error names what is wrong).  Every other entry point refuses a NULL context and writes nothing; the
order of LV_ESTATE and LV_EINVAL on a live context is held by tests/test_gpu_tsdf.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_tsdf_params", "lv_tsdf_configure", "lv_tsdf_integrate", "lv_tsdf_query", "lv_tsdf_fetch", "lv_tsdf_load",
           "lv_tsdf_clear", "lv_tsdf_get_params", "lv_tsdf_mesh_build", "lv_tsdf_mesh_fetch", "lv_tsdf_mesh_info", "lv_tsdf_mesh_clear")
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
    assert sorted(n for n in capi.ABI_SYMBOLS if "tsdf" in n) == sorted(SYMBOLS)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "lv_tsdf_params*": C.POINTER(capi.TsdfParams),
             "lv_mesh_info*": C.POINTER(capi.MeshInfo), "lv_view*": C.POINTER(capi.View), "void*": C.c_void_p,
             "float*": C.POINTER(C.c_float), "int32_t*": C.POINTER(C.c_int32), "uint32_t*": C.POINTER(C.c_uint32),
             "uint64_t*": C.POINTER(C.c_uint64)}
    counts = {"lv_default_tsdf_params": 1, "lv_tsdf_configure": 2, "lv_tsdf_integrate": 4, "lv_tsdf_query": 6, "lv_tsdf_fetch": 5,
              "lv_tsdf_load": 4, "lv_tsdf_clear": 1, "lv_tsdf_get_params": 2, "lv_tsdf_mesh_build": 3, "lv_tsdf_mesh_fetch": 6,
              "lv_tsdf_mesh_info": 2, "lv_tsdf_mesh_clear": 1}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = re.sub(r"\s*\[\d*\]$", "*", re.sub(r"\b(stats|counts)\[4\]", r"*\1", p))   # (uint64_t stats[4] is a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_tsdf_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    exprs, want = [], []
    for cname, ct in (("lv_tsdf_params", capi.TsdfParams), ("lv_mesh_info", capi.MeshInfo)):
        fields = [f for f, _ in ct._fields_]
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        want += [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want
    assert [f for f, _ in capi.TsdfParams._fields_] == ["origin", "resolution", "nx", "ny", "nz", "min_range", "max_range", "trunc_cells",
                                                        "max_weight", "carve"]
    assert C.sizeof(capi.TsdfParams) == 48 and C.sizeof(capi.MeshInfo) == 48


def test_default_params_round_trip(capi):
    f = C.c_float
    p = capi.default_tsdf_params()
    o = capi.default_occupancy_params()
    assert [v for v in p.origin] == [f(-51.2).value, f(-51.2).value, f(-3.2).value] == [v for v in o.origin]
    assert (p.resolution, p.nx, p.ny, p.nz) == (f(0.2).value, 512, 512, 64) == (o.resolution, o.nx, o.ny, o.nz)
    assert (p.min_range, p.max_range) == (1.0, 80.0) == (o.min_range, o.max_range)
    assert (p.trunc_cells, p.max_weight, p.carve) == (3, 10000, 0)
    q = capi.default_tsdf_params(origin=(1.0, 2.0, 3.0), nx=33, trunc_cells=5)
    assert [v for v in q.origin] == [1.0, 2.0, 3.0] and q.nx == 33 and q.trunc_cells == 5 and q.ny == 512
    capi.load_library().lv_default_tsdf_params(None)   # (a NULL target is ignored)


def test_like_occupancy_copies_the_footprint(capi):
    from limo_velo_amd import mesh

    o = capi.default_occupancy_params(origin=(1.0, -2.0, 0.5), resolution=0.25, nx=40, ny=30, nz=20, min_range=0.5, max_range=12.0)
    p = mesh.like_occupancy(o, trunc_cells=4, carve=1)
    assert [v for v in p.origin] == [1.0, -2.0, 0.5] and (p.resolution, p.nx, p.ny, p.nz, p.min_range, p.max_range) == (0.25, 40, 30, 20, 0.5, 12.0)
    assert (p.trunc_cells, p.max_weight, p.carve) == (4, 10000, 1)


def test_limits_are_refused_before_the_context(capi):
    lib = capi.load_library()

    def refused(**kw):
        p = capi.default_tsdf_params(**kw)
        rc = lib.lv_tsdf_configure(None, C.byref(p))
        return rc, lib.lv_last_error().decode()

    rc, why = refused()
    assert rc == LV_EINVAL and "null context" in why   # (good parameters: only the context is missing)
    inf, nan = float("inf"), float("nan")
    cases = [(dict(nx=0), "nx, ny, nz"), (dict(ny=0), "nx, ny, nz"), (dict(nz=0), "nx, ny, nz"), (dict(nx=1025), "nx, ny, nz"),
             (dict(ny=1025), "nx, ny, nz"), (dict(nz=1025), "nx, ny, nz"), (dict(nx=-4), "nx, ny, nz"),
             (dict(nx=1024, ny=1024, nz=257), "2^28"), (dict(resolution=0.0), "resolution"), (dict(resolution=-0.2), "resolution"),
             (dict(resolution=inf), "resolution"), (dict(resolution=nan), "resolution"), (dict(origin=(0.0, nan, 0.0)), "origin"),
             (dict(origin=(inf, 0.0, 0.0)), "origin"), (dict(resolution=0.01, max_range=41.0), "max_range / resolution"),
             (dict(min_range=0.0), "ranges"), (dict(min_range=80.0), "ranges"), (dict(max_range=inf), "ranges"), (dict(min_range=nan), "ranges"),
             (dict(trunc_cells=0), "trunc_cells"), (dict(trunc_cells=17), "trunc_cells"), (dict(trunc_cells=-3), "trunc_cells"),
             (dict(max_weight=0), "max_weight"), (dict(max_weight=2 ** 18 + 1), "max_weight"), (dict(max_weight=-1), "max_weight"),
             (dict(carve=2), "carve"), (dict(carve=-1), "carve")]
    for kw, what in cases:
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, why)
    # precedence: the first rule broken, in the order of the struct, is the one named
    for kw, what in ((dict(nx=0, trunc_cells=0), "nx, ny, nz"), (dict(resolution=0.0, nx=0), "resolution"),
                     (dict(trunc_cells=0, max_weight=0, carve=5), "trunc_cells"), (dict(max_weight=0, carve=5), "max_weight"),
                     (dict(min_range=0.0, carve=5), "ranges")):
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and what in why, (kw, why)
    # on the limits: accepted as far as the parameters go
    for kw in (dict(nx=1024, ny=1024, nz=256), dict(nx=1, ny=1, nz=1), dict(resolution=0.01, max_range=40.0), dict(trunc_cells=1),
               dict(trunc_cells=16), dict(max_weight=1), dict(max_weight=2 ** 18), dict(carve=1)):
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and "null context" in why, (kw, why)
    assert lib.lv_tsdf_configure(None, None) == LV_EINVAL and "null params" in lib.lv_last_error().decode()


def test_a_null_context_is_refused_and_nothing_is_written(capi):
    lib = capi.load_library()
    p = capi.default_tsdf_params(nx=7)
    info = capi.MeshInfo(built=9)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    out = (C.c_float * 3)(5.0, 5.0, 5.0)
    iout = (C.c_int32 * 3)(4, 4, 4)
    uout = (C.c_uint32 * 3)(6, 6, 6)
    assert lib.lv_tsdf_integrate(None, None, 1, stats) == LV_EINVAL
    assert lib.lv_tsdf_query(None, None, 12, 1, out, iout) == LV_EINVAL
    assert lib.lv_tsdf_fetch(None, iout, iout, out, 1) == LV_EINVAL
    assert lib.lv_tsdf_load(None, iout, iout, 1) == LV_EINVAL
    assert lib.lv_tsdf_clear(None) == LV_EINVAL
    assert lib.lv_tsdf_get_params(None, C.byref(p)) == LV_EINVAL
    assert lib.lv_tsdf_mesh_build(None, 1, stats) == LV_EINVAL
    assert lib.lv_tsdf_mesh_fetch(None, out, iout, uout, 1, 1) == LV_EINVAL
    assert lib.lv_tsdf_mesh_info(None, C.byref(info)) == LV_EINVAL
    assert lib.lv_tsdf_mesh_clear(None) == LV_EINVAL
    assert "null context" in lib.lv_last_error().decode()
    assert list(stats) == [7, 7, 7, 7] and list(out) == [5.0] * 3 and list(iout) == [4] * 3 and list(uout) == [6] * 3
    assert p.nx == 7 and info.built == 9
