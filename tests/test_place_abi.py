"""CPU checks of the place-recognition entry points (include/limovelo_hip.h "Place recognition"): the built library exports them,
the ctypes signatures and the lv_place_params layout capi installs agree with the header, the defaults; places.py's candidate
states against the rule (a fake hit list) and save_places / load_places through a fake context."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import place_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "limovelo_hip.h")
SYMBOLS = ("lv_default_place_params", "lv_place_configure", "lv_place_describe", "lv_place_add_scan", "lv_place_add_map",
           "lv_place_query", "lv_place_count", "lv_place_clear", "lv_place_fetch", "lv_place_load")


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    if not os.path.exists(c.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return c


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|void|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in limovelo_hip.h"
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_library_exports_the_symbols(capi):
    lib = capi.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {capi.LIB_PATH}"
        assert name in capi.ABI_SYMBOLS


def test_argtypes_agree_with_the_header(capi):
    lib = capi.load_library()
    table = {"lv_ctx*": C.c_void_p, "lv_state*": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int,
             "lv_place_params*": C.POINTER(capi.PlaceParams), "float*": C.POINTER(C.c_float), "double*": C.POINTER(C.c_double),
             "uint32_t*": C.POINTER(C.c_uint32), "int32_t*": C.POINTER(C.c_int32), "size_t*": C.POINTER(C.c_size_t)}
    ret = {"int": C.c_int, "void": None, "size_t": C.c_size_t}
    for name in SYMBOLS:
        rtype, params = _prototype(name)
        want = []
        for p in params:
            t = re.sub(r"\b[A-Za-z_][A-Za-z_0-9]*$", "", p).replace("const ", "").replace(" ", "")
            assert t in table, (name, p)
            want.append(table[t])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is ret[rtype], name


def test_params_layout_matches_c(capi, tmp_path):
    src = tmp_path / "layout.c"
    fields = [f for f, _ in capi.PlaceParams._fields_]
    assert fields == ["n_rings", "n_sectors", "rmin", "rmax", "z_offset"]
    exprs = ["sizeof(lv_place_params)"] + [f"offsetof(lv_place_params, {f})" for f in fields]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "limovelo_hip.h"\nint main(void){' +
                   "".join(f'printf("%zu\\n", (size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.PlaceParams)] + [getattr(capi.PlaceParams, f).offset for f in fields]


def test_defaults(capi):
    p = capi.default_place_params()
    assert (p.n_rings, p.n_sectors, p.rmin, p.rmax, p.z_offset) == (20, 60, 0.0, 80.0, 2.0)
    assert pr.DEFAULTS == dict(n_rings=20, n_sectors=60, rmin=0.0, rmax=80.0, z_offset=2.0)
    q = capi.default_place_params(n_sectors=32)
    assert (q.n_rings, q.n_sectors) == (20, 32)


def _state(synth, pos, rpy, offR=(0, 0, 0, 1), offT=(0, 0, 0)):
    return synth.make_state(pos, synth.quat_from_rpy(*rpy), offR, offT)


def test_candidate_states_follow_the_rule(lv):
    """A fake hit list: every candidate grid is centred on rotation Rz(s 2pi/S) R_x and position centre - R t_off."""
    from limo_velo_amd import places, synth

    offR = synth.quat_from_rpy(0.0, 0.0, math.radians(1.5))
    offT = (-0.17, 0.0, -0.04)
    x = _state(synth, (55.0, -3.0, 9.0), (math.radians(2.0), math.radians(-1.0), math.radians(70.0)), offR, offT)
    centres = np.array([[1.0, 2.0, 1.5], [-10.0, 4.0, 1.2], [30.0, -7.5, 0.8]])
    S = 60
    ids, shifts = np.array([2, 0, 1]), np.array([0, 17, 45])
    for i, s in zip(ids, shifts):
        st = places.hit_state(x, centres[i], s, S)
        yaw = pr.shift_yaw(s, S)
        assert -math.pi < yaw <= math.pi
        R = synth.quat_to_rot(synth.quat_from_rpy(0.0, 0.0, yaw)) @ synth.quat_to_rot(x[3:7])
        assert np.allclose(synth.quat_to_rot(st[3:7]), R, atol=1e-12)
        assert np.allclose(st[0:3], centres[i] - R @ np.asarray(offT), atol=1e-12)
        assert np.array_equal(st[7:], x[7:])
        # the LiDAR origin of the candidate is the place's centre (place_ref.frame's centre = R_x t_off + pos)
        _, c = pr.frame(st)
        assert np.allclose(c, centres[i], atol=1e-12)
    assert abs(pr.shift_yaw(30, 60) - math.pi) < 1e-12 and abs(pr.shift_yaw(45, 60) + math.pi / 2) < 1e-12
    xs, hit = places.candidates(x, ids, shifts, centres, S, xy_radius=1.0, xy_step=0.5)
    per = 5 * 5 * 5   # xy +-1 m by 0.5, yaw +-1 sector by half a sector
    assert xs.shape == (3 * per, 26) and np.array_equal(hit, np.repeat([0, 1, 2], per))
    for h in range(3):
        block = xs[hit == h]
        st = places.hit_state(x, centres[ids[h]], shifts[h], S)
        assert np.any(np.all(np.abs(block - st) < 1e-12, axis=1)), "the hit's own state is among its candidates"
        assert np.allclose(block[:, 2], st[2])


class _FakeCtx:
    def __init__(self, capi, prm, desc, centres):
        self.capi, self.prm, self.desc, self.centres = capi, prm, desc, centres
        self.calls = []

    def place_params(self):
        return self.prm

    def place_fetch(self):
        return self.desc.copy(), self.centres.copy()

    def place_configure(self, p):
        self.calls.append(("configure", (p.n_rings, p.n_sectors, p.rmin, p.rmax, p.z_offset)))
        self.prm, self.desc, self.centres = p, np.zeros((0, p.n_rings, p.n_sectors), np.float32), np.zeros((0, 3))

    def place_load(self, desc, centres):
        self.calls.append(("load", len(centres)))
        self.desc = np.concatenate([self.desc, np.asarray(desc, np.float32).reshape(len(centres), self.prm.n_rings, -1)])
        self.centres = np.concatenate([self.centres, centres])


def test_save_load_round_trip(capi, tmp_path):
    from limo_velo_amd import places

    prm = capi.default_place_params(n_rings=7, n_sectors=12, rmin=1.5, rmax=40.0, z_offset=1.25)
    rng = np.random.default_rng(3)
    desc = rng.uniform(0, 5, (9, 7, 12)).astype(np.float32)
    centres = rng.normal(0, 50, (9, 3))
    a = _FakeCtx(capi, prm, desc, centres)
    path = tmp_path / "places.npz"
    places.save_places(a, path)
    b = _FakeCtx(capi, capi.default_place_params(), np.zeros((0, 20, 60), np.float32), np.zeros((0, 3)))
    places.load_places(b, path)
    assert b.calls == [("configure", (7, 12, 1.5, 40.0, 1.25)), ("load", 9)]
    assert np.array_equal(b.desc.view(np.uint32), desc.view(np.uint32))
    assert np.array_equal(b.centres, centres)


def test_map_grid_centres():
    from limo_velo_amd import places

    rng = np.random.default_rng(5)
    ground = np.column_stack([rng.uniform(0, 20, 20000), rng.uniform(0, 12, 20000), rng.uniform(-0.02, 0.02, 20000)])
    roof = np.column_stack([rng.uniform(8, 12, 4000), rng.uniform(4, 8, 4000), np.full(4000, 3.0)])
    hole = (ground[:, 0] > 12.5) & (ground[:, 1] > 8)
    corners = np.array([[0.0, 0.0, 0.0], [20.0, 12.0, 0.0]])
    pts = np.concatenate([ground[~hole], roof, corners]).astype(np.float32)
    c = places.map_grid_centres(pts, 4.0, 1.5)
    # a 5 x 3 grid of cell centres (2, 6, ..., 18) x (2, 6, 10); the two cells inside the hole have no point within 0.5 m
    assert len(c) == 13
    assert set(map(tuple, c[:, :2])) == {(x, y) for x in (2.0, 6.0, 10.0, 14.0, 18.0) for y in (2.0, 6.0, 10.0)} - {(14.0, 10.0),
                                                                                                                    (18.0, 10.0)}
    for x, y, z in c:
        near = (np.abs(pts[:, 0] - x) <= 0.5) & (np.abs(pts[:, 1] - y) <= 0.5)
        assert z == pytest.approx(float(pts[near, 2].min()) + 1.5)
