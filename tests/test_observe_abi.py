"""CPU checks of the aiding-observation entry points (include/limovelo_hip.h "Aiding observations"): the built library exports
them, the ctypes signatures and the layouts of the structs capi installs agree with the header, and lv_default_observation gives
the documented values."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_observation", "lv_observe", "lv_observe_results")


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
    assert "/* ---- Aiding observations" in text
    assert text.index("/* ---- resident filter") < text.index("/* ---- Aiding observations") < text.index("/* ---- multi-GPU")


def test_constants_agree_with_the_header(capi):
    text = open(HEADER).read()
    enum = dict(re.findall(r"(LV_OBS_[A-Z_]+) = (\d+)", text))
    assert enum == {"LV_OBS_POSITION": "1", "LV_OBS_VELOCITY_WORLD": "2", "LV_OBS_VELOCITY_BODY": "3", "LV_OBS_ATTITUDE": "4"}
    assert (capi.OBS_POSITION, capi.OBS_VELOCITY_WORLD, capi.OBS_VELOCITY_BODY, capi.OBS_ATTITUDE) == (1, 2, 3, 4)
    assert int(re.search(r"#define LV_OBSERVE_BATCH (\d+)", text).group(1)) == capi.OBSERVE_BATCH == 8


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "size_t*": C.POINTER(C.c_size_t),
             "lv_observation*": C.POINTER(capi.Observation), "lv_observe_result*": C.POINTER(capi.ObserveResult)}
    counts = {"lv_default_observation": 2, "lv_observe": 4, "lv_observe_results": 4}
    for name in SYMBOLS:
        want = []
        for p in _prototype(name):
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is (None if name == "lv_default_observation" else C.c_int)
        assert len(want) == counts[name]


def test_struct_layouts_match_c(capi, tmp_path):
    structs = (("lv_observation", capi.Observation, ["kind", "mask", "z", "R", "lever", "gate"]),
               ("lv_observe_result", capi.ObserveResult, ["status", "rows", "nis", "y"]))
    exprs, want = [], []
    for cname, cls, fields in structs:
        assert [f for f, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == want == [144, 0, 4, 8, 40, 112, 136, 40, 0, 4, 8, 16]


def test_default_observation(capi):
    lib = capi.load_library()
    for kind in (1, 2, 3, 4):
        o = capi.Observation()
        C.memset(C.byref(o), 0xFF, C.sizeof(o))
        lib.lv_default_observation(C.byref(o), kind)
        assert (o.kind, o.mask, o.gate) == (kind, 7, 0.0)
        assert list(o.z) == [0, 0, 0, 1.0 if kind == capi.OBS_ATTITUDE else 0.0]
        assert list(o.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(o.lever) == [0, 0, 0]
    lib.lv_default_observation(None, 1)   # (a NULL target is ignored)
    o = capi.default_observation(capi.OBS_POSITION, z=(1, 2, 3), lever=(0.1, 0.2, 0.3), gate=9.0, mask=5)
    assert (list(o.z), list(o.lever), o.gate, o.mask) == ([1, 2, 3, 0], [0.1, 0.2, 0.3], 9.0, 5)


def test_refusals_that_need_no_gpu(capi):
    lib = capi.load_library()
    o = capi.default_observation(capi.OBS_POSITION)
    out = (capi.ObserveResult * 8)()
    assert lib.lv_observe(None, C.byref(o), 1, out) == -1 and b"null context" in lib.lv_last_error()
    assert lib.lv_observe_results(None, out, 8, None) == -1 and b"null context" in lib.lv_last_error()
