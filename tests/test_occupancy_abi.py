"""CPU checks of the occupancy grid's entry points (include/limovelo_hip.h "Occupancy grid"): the built library exports them, the
ctypes signatures and the struct layout capi installs agree with the header, the defaults are as documented, and lv_occ_configure
refuses every parameter outside its limits (it judges the parameters before the context, so the refusal shows without a GPU:
lv_last_error names what is wrong)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_occupancy_params", "lv_occ_configure", "lv_occ_integrate", "lv_occ_query", "lv_occ_project", "lv_occ_fetch",
           "lv_occ_load", "lv_occ_clear", "lv_occ_get_params")
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


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "lv_occupancy_params*": C.POINTER(capi.OccupancyParams),
             "lv_view*": C.POINTER(capi.View), "void*": C.c_void_p, "float*": C.POINTER(C.c_float), "int8_t*": C.POINTER(C.c_int8),
             "uint64_t*": C.POINTER(C.c_uint64)}
    counts = {"lv_default_occupancy_params": 1, "lv_occ_configure": 2, "lv_occ_integrate": 4, "lv_occ_query": 5, "lv_occ_project": 5,
              "lv_occ_fetch": 3, "lv_occ_load": 3, "lv_occ_clear": 1, "lv_occ_get_params": 2}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = re.sub(r"\s*\[\d*\]$", "*", p.replace("stats[4]", "*stats"))   # (uint64_t stats[4] is a pointer)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_occupancy_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layout_matches_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fields = [f for f, _ in capi.OccupancyParams._fields_]
    exprs = ["sizeof(lv_occupancy_params)"] + [f"offsetof(lv_occupancy_params, {f})" for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.OccupancyParams)] + [getattr(capi.OccupancyParams, f).offset for f in fields]
    assert got == want
    assert fields == ["origin", "resolution", "nx", "ny", "nz", "min_range", "max_range", "l_hit", "l_miss", "l_min", "l_max", "l_occ",
                      "l_free"]


def test_default_params_round_trip(capi):
    f = C.c_float
    p = capi.default_occupancy_params()
    assert [v for v in p.origin] == [f(-51.2).value, f(-51.2).value, f(-3.2).value]
    assert (p.resolution, p.nx, p.ny, p.nz) == (f(0.2).value, 512, 512, 64)
    assert (p.min_range, p.max_range) == (1.0, 80.0)
    assert (p.l_hit, p.l_miss, p.l_min, p.l_max) == (f(0.85).value, f(-0.4).value, -2.0, 3.5)
    assert (p.l_occ, p.l_free) == (f(0.4).value, f(-0.4).value)
    # centred on 0 in x, y
    assert abs(p.origin[0] + 0.5 * p.nx * p.resolution) < 1e-4 and abs(p.origin[1] + 0.5 * p.ny * p.resolution) < 1e-4
    q = capi.default_occupancy_params(origin=(1.0, 2.0, 3.0), nx=33, l_occ=0.5)
    assert [v for v in q.origin] == [1.0, 2.0, 3.0] and q.nx == 33 and q.l_occ == 0.5 and q.ny == 512
    capi.load_library().lv_default_occupancy_params(None)   # (a NULL target is ignored)


def test_limits_are_refused(capi):
    lib = capi.load_library()

    def refused(**kw):
        p = capi.default_occupancy_params(**kw)
        rc = lib.lv_occ_configure(None, C.byref(p))
        return rc, lib.lv_last_error().decode()

    rc, why = refused()
    assert rc == LV_EINVAL and "null context" in why   # (good parameters: only the context is missing)
    inf, nan = float("inf"), float("nan")
    cases = [(dict(nx=0), "nx, ny, nz"), (dict(ny=0), "nx, ny, nz"), (dict(nz=0), "nx, ny, nz"), (dict(nx=1025), "nx, ny, nz"),
             (dict(ny=1025), "nx, ny, nz"), (dict(nz=1025), "nx, ny, nz"), (dict(nx=-4), "nx, ny, nz"),
             (dict(nx=1024, ny=1024, nz=257), "2^28"), (dict(resolution=0.0), "resolution"), (dict(resolution=-0.2), "resolution"),
             (dict(resolution=inf), "resolution"), (dict(resolution=nan), "resolution"), (dict(origin=(0.0, nan, 0.0)), "origin"),
             (dict(resolution=0.01, max_range=41.0), "max_range / resolution"), (dict(min_range=0.0), "ranges"),
             (dict(min_range=80.0), "ranges"), (dict(max_range=inf), "ranges"), (dict(l_hit=0.0), "l_miss < 0 < l_hit"),
             (dict(l_hit=-0.85), "l_miss < 0 < l_hit"), (dict(l_miss=0.4), "l_miss < 0 < l_hit"), (dict(l_miss=nan), "l_miss < 0 < l_hit"),
             (dict(l_min=0.0), "l_min < 0 < l_max"), (dict(l_max=-1.0), "l_min < 0 < l_max"), (dict(l_max=inf), "l_min < 0 < l_max"),
             (dict(l_occ=-0.4), "l_free < l_occ"), (dict(l_free=0.5), "l_free < l_occ"), (dict(l_occ=nan), "l_free < l_occ")]
    for kw, what in cases:
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, why)
    # on the limits: accepted as far as the parameters go
    for kw in (dict(nx=1024, ny=1024, nz=256), dict(nx=1, ny=1, nz=1), dict(resolution=0.01, max_range=40.0)):
        rc, why = refused(**kw)
        assert rc == LV_EINVAL and "null context" in why, (kw, why)
    assert lib.lv_occ_configure(None, None) == LV_EINVAL and "null params" in lib.lv_last_error().decode()


def test_null_arguments_are_refused_without_a_context(capi):
    lib = capi.load_library()
    p = capi.default_occupancy_params()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    out = (C.c_float * 1)(5.0)
    g2 = (C.c_int8 * 1)(9)
    assert lib.lv_occ_integrate(None, None, 1, stats) != 0
    assert lib.lv_occ_query(None, None, 12, 1, out) != 0
    assert lib.lv_occ_project(None, 0, 0, g2, 1) != 0
    assert lib.lv_occ_fetch(None, out, 1) != 0
    assert lib.lv_occ_load(None, out, 1) != 0
    assert lib.lv_occ_clear(None) != 0
    assert lib.lv_occ_get_params(None, C.byref(p)) != 0
    assert list(stats) == [7, 7, 7, 7] and out[0] == 5.0 and g2[0] == 9   # (nothing written)
