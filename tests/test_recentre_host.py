"""The rolling-volume part of limo-velo_amd/csrc/lv_grid.hpp (the source cell of a shifted voxel, its mirror, the origin at an
accumulated shift, the limits of a recentre, the box clip and the rule of lv_occ_mark: what the kernels and the entry points run)
compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h: tests/emu/recentre_emu.cpp runs one case
per call.  Held to numpy (tests/recentre_ref.py) by equality of bits, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import recentre_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
LIMIT = 1 << 20


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recentre_host") / "recentre_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "recentre_emu.cpp"), "-o", str(exe)])

    def run(case, text):
        out = subprocess.run([str(exe), case], input=(text + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
        return [ln.split() for ln in out.strip().split("\n")]

    return run


def _volume(dims, seed):
    """Log-odds bits [nz, ny, nx]: about a third never observed, the rest distinct values, and one NaN with another payload (it
    is no evidence, and its bits must survive a move)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    L = rng.uniform(-2.0, 3.5, (nz, ny, nx)).astype(F)
    L[rng.random(L.shape) < 0.35] = np.nan
    bits = L.view(np.uint32).copy()
    bits.reshape(-1)[-1] = 0x7FC00001
    return bits


@pytest.mark.parametrize("dims", rr.GRIDS + rr.ALIGNED_GRIDS)
def test_shift_equals_the_slice_assignment(emu, dims):
    bits = _volume(dims, 5)
    evidence = ~np.isnan(bits.view(F))
    for d in rr.shift_list(dims):
        out = emu("shift", _ints(dims) + " " + _ints(d) + " " + _ints(bits))
        want = rr.shifted(bits, d, rr.NAN_BITS)
        got = np.array([int(ln[0]) for ln in out[1:]], np.uint32).reshape(bits.shape)
        assert np.array_equal(got, want), d
        assert [int(v) for v in out[0][1:]] == rr.stats(evidence, d)[:3], d
        if any(abs(d[a]) >= dims[a] for a in range(3)):
            assert np.all(got == rr.NAN_BITS) and int(out[0][3]) == int(evidence.sum())   # everything left
        if d == (0, 0, 0):
            assert np.array_equal(got, bits)


def test_limits_of_one_shift_and_of_the_accumulated_one(emu):
    o0, res = (-51.2, -51.2, -3.2), 0.2

    def check(s, d, origin0=o0, resolution=res):
        out = emu("check", " ".join([_bits(origin0), _bits([resolution]), _ints(s), _ints(d)]))[0]
        ok, s_new, o_new = rr.check(origin0, resolution, s, d)
        assert (out[0] == "ok") == ok, (s, d)
        assert [int(v) for v in out[1:4]] == [int(v) for v in s_new]
        if ok:
            assert [int(v) for v in out[4:]] == [int(v) for v in o_new.view(np.uint32)]
        return ok

    for a in range(3):
        for sgn in (1, -1):
            d = [0, 0, 0]
            d[a] = sgn * LIMIT
            assert check((0, 0, 0), d)                       # 2^20: accepted
            d[a] = sgn * (LIMIT + 1)
            assert not check((0, 0, 0), d)                   # 2^20 + 1: refused
            d[a] = sgn * (2 ** 31 - 1)
            assert not check((0, 0, 0), d)
            s = [5, -7, 9]
            s[a] = sgn * (LIMIT - 3)
            d[a] = sgn * 3
            assert check(s, d)                               # the accumulated shift reaches the limit ...
            d[a] = sgn * 4
            assert not check(s, d)                           # ... and may not pass it: the state stays as it was
            d[a] = -sgn * LIMIT
            assert check(s, d)
    assert not check((0, 0, 0), (0, -2 ** 31, 0))
    assert not check((0, 0, 0), (LIMIT, 0, 0), origin0=(3e38, 0.0, 0.0), resolution=1e33)   # origin' would be inf
    assert check((0, 0, 0), (1, 0, 0), origin0=(3e38, 0.0, 0.0), resolution=1e30)


def test_the_origin_depends_on_the_accumulated_shift_alone(emu):
    o0, res = (-51.2, -51.2, -3.2), 0.2
    s = np.zeros(3, np.int64)
    rng = np.random.default_rng(2)
    path = [(32, 0, 0), (1, -7, 3), (-33, 7, -3)] + [tuple(int(v) for v in rng.integers(-5000, 5000, 3)) for _ in range(20)]
    path.append(tuple(-int(v) for v in np.sum(path, axis=0)))   # ... and home again
    for d in path:
        out = emu("check", " ".join([_bits(o0), _bits([res]), _ints(s), _ints(d)]))[0]
        assert out[0] == "ok"
        s = s + np.array(d)
        assert [int(v) for v in out[1:4]] == list(s)
        assert [int(v) for v in out[4:]] == [int(v) for v in rr.origin_at(o0, s, res).view(np.uint32)]
    assert not s.any() and [int(v) for v in out[4:]] == [int(v) for v in np.asarray(o0, F).view(np.uint32)]   # origin0, bit for bit
    # +d then -d from anywhere
    for d in ((1, 1, 1), (32, -32, 8), (LIMIT, -LIMIT, 77)):
        a = emu("check", " ".join([_bits(o0), _bits([res]), _ints((0, 0, 0)), _ints(d)]))[0]
        b = emu("check", " ".join([_bits(o0), _bits([res]), _ints(a[1:4]), _ints([-v for v in d])]))[0]
        assert b[1:4] == ["0", "0", "0"] and [int(v) for v in b[4:]] == [int(v) for v in np.asarray(o0, F).view(np.uint32)]


def test_clip_box(emu):
    dims = (33, 5, 3)
    boxes = [((0, 0, 0), (32, 4, 2)), ((-5, -5, -5), (2 ** 30, 2 ** 30, 2 ** 30)), ((3, 1, 1), (3, 1, 1)), ((33, 0, 0), (40, 4, 2)),
             ((0, 0, 0), (-1, 4, 2)), ((5, 3, 0), (4, 4, 2)), ((0, 5, 0), (32, 9, 2)), ((-9, 2, 2), (0, 2, 7)), ((0, 0, 3), (1, 1, 3))]
    for lo, hi in boxes:
        out = emu("clip", _ints(dims) + " " + _ints(lo) + " " + _ints(hi))[0]
        want = rr.clip_box(dims, lo, hi)
        assert (out == ["0"]) if want is None else ([int(v) for v in out] == [1] + want[0] + want[1]), (lo, hi)


@pytest.mark.parametrize("only_unknown", [1, 0])
@pytest.mark.parametrize("l_mark", [0.85, -0.4, 9.0, -9.0])
def test_mark_rule(emu, only_unknown, l_mark):
    l_min, l_max, min_points = -2.0, 3.5, 3
    Ls = np.array([np.nan, -2.0, -0.4, 0.0, 0.4, 3.5, 3.0], F)
    counts = [0, 2, 3, 4, 1 << 20]
    rows = [(c, L) for c in counts for L in Ls]
    text = " ".join(["%d %d" % (min_points, only_unknown), _bits([l_mark, l_min, l_max]), str(len(rows))] +
                    ["%d %s" % (c, _bits([L])) for c, L in rows])
    out = emu("mark", text)
    for (c, L), ln in zip(rows, out):
        # one voxel through the numpy rule: a 1 x 1 x 1 grid holding c points at its centre
        prm = dict(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=1, ny=1, nz=1, l_min=l_min, l_max=l_max)
        pts = np.full((c if c < 100 else 0, 3), 0.5, F)
        if c >= 100:   # (2^20 points: the count alone matters)
            want_L, st = rr.mark(prm, np.array([[[L]]], F), np.full((3, 3), 0.5, F), (0, 0, 0), (0, 0, 0), 3, only_unknown, l_mark)
        else:
            want_L, st = rr.mark(prm, np.array([[[L]]], F), pts, (0, 0, 0), (0, 0, 0), min_points, only_unknown, l_mark)
        assert [int(v) for v in ln[:3]] == [st[2], st[1], st[3]], (c, L)
        assert int(ln[3]) == int(want_L.view(np.uint32)[0, 0, 0]), (c, L)
