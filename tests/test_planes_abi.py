"""CPU checks of the plane segmentation's entry points (include/limovelo_hip.h "Plane segmentation"): the built library exports
them, the ctypes signatures and both struct layouts capi installs agree with the header, the numpy record agrees with the ctypes
one, the defaults are as documented and null arguments are refused."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_plane_params", "lv_map_planes")


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
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "lv_plane_params*": C.POINTER(capi.PlaneParams), "lv_plane*": C.POINTER(capi.Plane),
             "uint8_t*": C.POINTER(C.c_uint8), "size_t*": C.POINTER(C.c_size_t), "int32_t*": C.POINTER(C.c_int32)}
    for name, restype in (("lv_map_planes", C.c_int), ("lv_default_plane_params", None)):
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is restype
    assert len(_prototype("lv_map_planes")) == 8


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    exprs, want = [], []
    for cname, T in (("lv_plane_params", capi.PlaneParams), ("lv_plane", capi.Plane)):
        fields = [f for f, _ in T._fields_]
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want
    assert [f for f, _ in capi.PlaneParams._fields_] == ["distance", "iterations", "max_planes", "min_inliers", "seed", "constraint", "axis", "max_angle", "refine"]
    assert [f for f, _ in capi.Plane._fields_] == ["normal", "anchor", "d", "rms", "inliers", "support", "hypothesis", "candidates", "n_fit", "flags"]
    assert C.sizeof(capi.PlaneParams) == 48 and C.sizeof(capi.Plane) == 64
    # the numpy record is the ctypes one
    assert capi.PLANE_DTYPE.itemsize == C.sizeof(capi.Plane) and list(capi.PLANE_DTYPE.names) == [f for f, _ in capi.Plane._fields_]
    assert [capi.PLANE_DTYPE.fields[f][1] for f in capi.PLANE_DTYPE.names] == [getattr(capi.Plane, f).offset for f in capi.PLANE_DTYPE.names]


def test_default_params_round_trip(capi):
    p = capi.default_plane_params()
    assert (p.distance, p.iterations, p.max_planes, p.min_inliers, p.seed, p.constraint, list(p.axis), p.refine) == (np.float32(0.1), 512, 1, 100, 0, 0, [0.0, 0.0, 1.0], 1)
    assert p.max_angle == np.float32(10.0 * math.pi / 180.0)
    q = capi.default_plane_params(distance=0.25, iterations=4096, max_planes=8, seed=2**64 - 1, constraint=2, axis=(1, 2, 3), max_angle=0.5, refine=0)
    assert (q.distance, q.iterations, q.max_planes, q.seed, q.constraint, list(q.axis), q.max_angle, q.refine) == (0.25, 4096, 8, 2**64 - 1, 2, [1.0, 2.0, 3.0], 0.5, 0)
    capi.load_library().lv_default_plane_params(None)   # (a NULL target is ignored)
    assert capi.PLANE_MAX_PLANES == 32


def test_bad_arguments_are_refused_without_a_context(capi):
    lib = capi.load_library()
    p = capi.default_plane_params()
    n = C.c_size_t(77)
    assert lib.lv_map_planes(None, C.byref(p), None, None, 0, None, 0, C.byref(n)) != 0
    assert lib.lv_map_planes(None, None, None, None, 0, None, 0, C.byref(n)) != 0
    assert n.value == 77   # (nothing written)
