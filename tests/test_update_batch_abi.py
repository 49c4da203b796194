"""CPU checks of the multi-hypothesis entry points (include/limovelo_hip.h "Multi-hypothesis updates"): the built library exports
lv_iterate_batch / lv_update_batch, the ctypes signatures capi installs agree with the header's prototypes parameter by
parameter, and the host half of prelocalisation (candidate_grid, rank) orders hand-made inputs as documented."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
CALLS = ("lv_iterate_batch", "lv_update_batch")


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return c


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in limovelo_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    p = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", param.strip()).strip().replace("const ", "").replace(" ", "")
    table = {"lv_ctx*": C.c_void_p, "lv_state*": C.c_void_p, "lv_sums*": C.c_void_p, "size_t": C.c_size_t,
             "double*": C.POINTER(C.c_double), "int*": C.POINTER(C.c_int)}
    assert p in table, (param, p)
    return table[p]


def test_library_exports_the_batch_calls(capi):
    lib = capi.load_library()
    for name in CALLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS


@pytest.mark.parametrize("name", CALLS)
def test_argtypes_agree_with_the_header(capi, name):
    lib = capi.load_library()
    want = [_ctype_of(p) for p in _prototype(name)]
    got = getattr(lib, name).argtypes
    assert got is not None, f"capi sets no argtypes for {name}"
    assert len(got) == len(want), (name, got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name} parameter {i}: {g} vs {w}"
    assert getattr(lib, name).restype is C.c_int


def test_null_context_is_refused(capi):
    lib = capi.load_library()
    assert lib.lv_iterate_batch(None, None, 1, None) != 0
    assert lib.lv_update_batch(None, None, 1, None, None, None, None) != 0


def test_candidate_grid_shape_and_rotations():
    from limo_velo_amd import prelocalise as pl, synth

    x0 = synth.make_state([1.0, 2.0, 0.5], synth.quat_from_rpy(0.0, 0.0, 0.3))
    g = pl.candidate_grid(x0, xy_radius=1.0, xy_step=0.5, yaw_span=math.radians(30), yaw_step=math.radians(15), z_offsets=(0.0, 0.2))
    assert g.shape == (2 * 5 * 5 * 5, 26)
    assert np.allclose(g[:, 7:], x0[7:])
    # rows: z, then yaw, then x, then y
    assert np.allclose(g[0, :3], x0[:3] + [-1.0, -1.0, 0.0])
    assert np.allclose(g[1, :3], x0[:3] + [-1.0, -0.5, 0.0])
    assert np.allclose(g[-1, :3], x0[:3] + [1.0, 1.0, 0.2])
    yaws = [math.atan2(2 * (q[3] * q[2] + q[0] * q[1]), 1 - 2 * (q[1] ** 2 + q[2] ** 2)) for q in g[::25, 3:7]]
    assert np.allclose(yaws[:5], 0.3 + np.radians([-30, -15, 0, 15, 30]))
    assert np.allclose(g[50, 3:7], synth.quat_mul(synth.quat_from_rpy(0, 0, 0.0), x0[3:7]))
    assert pl.candidate_grid(x0, 0.0, 0.5, 0.0, 0.1).shape == (1, 26)


def test_rank_orders_by_matches_then_residual_with_ties_and_empty_last():
    from limo_velo_amd import prelocalise as pl

    last = [dict(n_valid=0, sum_h2=0.0), dict(n_valid=10, sum_h2=1.0), dict(n_valid=12, sum_h2=6.0), dict(n_valid=12, sum_h2=3.0),
            dict(n_valid=10, sum_h2=1.0), dict(n_valid=0, sum_h2=5.0), dict(n_valid=12, sum_h2=3.0)]
    order = pl.rank(np.zeros(len(last), np.int32), last)
    assert order.tolist() == [3, 6, 2, 1, 4, 0, 5]
    assert pl.rank([], []).tolist() == []
