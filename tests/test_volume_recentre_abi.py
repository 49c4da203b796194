"""CPU checks of the rolling volumes' entry points (include/limovelo_hip.h "Rolling volumes"): the built library exports them, the
ctypes signatures and the two struct layouts capi installs agree with the header and a compiled C program, the defaults are as
documented, and every argument outside its limits is refused before the context is looked at ("null context" comes last), so the
refusals and their precedence show without a GPU.  The order of LV_ESTATE and the accumulated limit on a live context is held by
tests/test_gpu_volume_recentre.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_volume_recentre", "lv_volume_shift_info", "lv_default_occ_mark_params", "lv_occ_mark")
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
        assert "tsdf" not in name   # (tests/test_tsdf_abi.py owns the names that contain it)
    assert sorted(set(capi.VOLUME_ARGTYPES) | {"lv_default_occ_mark_params"}) == sorted(SYMBOLS)


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "lv_volume_shifts*": C.POINTER(capi.VolumeShifts),
             "lv_occ_mark_params*": C.POINTER(capi.OccMarkParams), "void*": C.c_void_p, "int32_t*": C.POINTER(C.c_int32),
             "uint64_t*": C.POINTER(C.c_uint64)}
    counts = {"lv_volume_recentre": 4, "lv_volume_shift_info": 2, "lv_default_occ_mark_params": 1, "lv_occ_mark": 6}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            p = re.sub(r"\b(stats|shift)\[\d\]", r"*\1", p)   # (uint64_t stats[4], int32_t shift[3] are pointers)
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_occ_mark_params" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    exprs, want = ["LV_VOLUME_OCC", "LV_VOLUME_SURFACE"], [capi.LV_VOLUME_OCC, capi.LV_VOLUME_SURFACE]
    for cname, ct in (("lv_volume_shifts", capi.VolumeShifts), ("lv_occ_mark_params", capi.OccMarkParams)):
        fields = [f for f, _ in ct._fields_]
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        want += [C.sizeof(ct)] + [getattr(ct, f).offset for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want
    assert [f for f, _ in capi.VolumeShifts._fields_] == ["grid", "surface", "field", "plan", "frontier"]
    assert [f for f, _ in capi.OccMarkParams._fields_] == ["lo", "hi", "min_points", "only_unknown", "l_mark"]
    assert C.sizeof(capi.VolumeShifts) == 60 and C.sizeof(capi.OccMarkParams) == 36


def test_default_mark_params(capi):
    p = capi.default_occ_mark_params()
    assert list(p.lo) == [0, 0, 0] and all(v >= 1024 for v in p.hi)          # the whole of any grid
    assert (p.min_points, p.only_unknown, p.l_mark) == (1, 1, C.c_float(0.85).value)
    q = capi.default_occ_mark_params(lo=(1, 2, 3), hi=(4, 5, 6), min_points=7, only_unknown=0, l_mark=-0.4)
    assert list(q.lo) == [1, 2, 3] and list(q.hi) == [4, 5, 6] and (q.min_points, q.only_unknown) == (7, 0)
    capi.load_library().lv_default_occ_mark_params(None)   # (a NULL target is ignored)


def test_recentre_refuses_its_arguments_before_the_context(capi):
    lib = capi.load_library()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)

    def refused(volume, shift):
        d = (C.c_int32 * 3)(*shift) if shift is not None else None
        rc = lib.lv_volume_recentre(None, volume, d, stats)
        return rc, lib.lv_last_error().decode()

    for volume in (capi.LV_VOLUME_OCC, capi.LV_VOLUME_SURFACE):
        for shift in ((0, 0, 0), (1, -2, 3), (2 ** 20, -2 ** 20, 2 ** 20)):   # good arguments: only the context is missing
            rc, why = refused(volume, shift)
            assert rc == LV_EINVAL and "null context" in why, (volume, shift, why)
        for a in range(3):
            for v in (2 ** 20 + 1, -2 ** 20 - 1, 2 ** 31 - 1, -2 ** 31):
                shift = [0, 0, 0]
                shift[a] = v
                rc, why = refused(volume, shift)
                assert rc == LV_EINVAL and "2^20" in why and "null context" not in why, (shift, why)
        rc, why = refused(volume, None)
        assert rc == LV_EINVAL and "null shift" in why
    for volume in (-1, 2, 99):
        rc, why = refused(volume, (0, 0, 0))
        assert rc == LV_EINVAL and "volume" in why and "null context" not in why
        rc, why = refused(volume, (2 ** 21, 0, 0))   # precedence: the volume is judged first
        assert rc == LV_EINVAL and "volume" in why
    assert list(stats) == [7, 7, 7, 7]
    info = capi.VolumeShifts()
    info.grid[0] = 9
    assert lib.lv_volume_shift_info(None, None) == LV_EINVAL and "null argument" in lib.lv_last_error().decode()
    assert lib.lv_volume_shift_info(None, C.byref(info)) == LV_EINVAL and "null context" in lib.lv_last_error().decode()
    assert info.grid[0] == 9


def test_mark_refuses_its_arguments_before_the_context(capi):
    lib = capi.load_library()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    pts = (C.c_float * 3)(0.0, 0.0, 0.0)

    def refused(p, points=pts, stride=12, n=1):
        rc = lib.lv_occ_mark(None, C.byref(p) if p is not None else None, points, stride, n, stats)
        return rc, lib.lv_last_error().decode()

    inf, nan = float("inf"), float("nan")
    for kw in (dict(), dict(min_points=2 ** 20), dict(l_mark=-0.4), dict(only_unknown=0), dict(lo=(5, 5, 5), hi=(1, 1, 1))):
        rc, why = refused(capi.default_occ_mark_params(**kw))
        assert rc == LV_EINVAL and "null context" in why, (kw, why)
    rc, why = refused(capi.default_occ_mark_params(), None, 0, 0)   # (the map as the source)
    assert rc == LV_EINVAL and "null context" in why
    cases = [(dict(min_points=0), "min_points"), (dict(min_points=-3), "min_points"), (dict(min_points=2 ** 20 + 1), "min_points"),
             (dict(l_mark=0.0), "l_mark"), (dict(l_mark=inf), "l_mark"), (dict(l_mark=-inf), "l_mark"), (dict(l_mark=nan), "l_mark")]
    for kw, what in cases:
        rc, why = refused(capi.default_occ_mark_params(**kw))
        assert rc == LV_EINVAL and what in why and "null context" not in why, (kw, why)
    rc, why = refused(capi.default_occ_mark_params(min_points=0, l_mark=0.0))   # precedence: in the order of the struct
    assert rc == LV_EINVAL and "min_points" in why
    rc, why = refused(capi.default_occ_mark_params(), pts, 11, 1)
    assert rc == LV_EINVAL and "stride" in why and "null context" not in why
    rc, why = refused(capi.default_occ_mark_params(), pts, 12, 2 ** 31)
    assert rc == LV_EINVAL and "too many" in why
    rc, why = refused(None)
    assert rc == LV_EINVAL and "null params" in why
    assert list(stats) == [7, 7, 7, 7]
