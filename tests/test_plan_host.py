"""The rule of lv_plan.hpp (plan_isqrt, plan_cell_cost, plan_move_allowed, plan_edge, plan_relax, plan_next: what the kernels of
lv_plan.hip run) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to
tests/plan_ref.py: tests/emu/plan_emu.cpp builds the potential of a given distance field by plain sweeps to the fixpoint and walks
the paths.  Cost bytes, P, stats, status, path cells and path costs are equal, no tolerance."""
import math
import os
import subprocess

import numpy as np
import pytest

import occupancy_ref as ocr
import plan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
TABLE6 = np.array([254, 180, 110, 70, 55, 50], np.uint8)
TABLE1 = np.array([1], np.uint8)


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_host") / "plan_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "plan_emu.cpp"), "-o", str(exe)])

    def run(text):
        return subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")

    def plan(prm, s2, pp, table, goals, starts=()):
        s2 = np.asarray(s2)
        planar = s2.ndim == 2
        goals = np.asarray(goals, F).reshape(-1, 3)
        starts = np.asarray(starts, F).reshape(-1, 3)
        nz = 1 if planar else s2.shape[0]
        lines = ["0", " ".join([_bits(prm["origin"]), _bits([prm["resolution"]]), str(s2.shape[-1]), str(s2.shape[-2]), str(nz), str(int(planar))]),
                 f"{pp['connectivity']} {pp['min_clear_s2']}", f"{len(table)} {_ints(table)}", _ints(s2), f"{len(goals)} {_bits(goals)}",
                 f"{len(starts)} {_bits(starts)}"]
        out = run("\n".join(lines) + "\n")
        if out[0] != "params ok":
            return out[0]
        assert out[1].split() == ["field", str(s2.shape[-1]), str(s2.shape[-2]), str(nz)]
        cost = np.array(out[2].split(), np.uint8).reshape(s2.shape)
        P = np.array(out[3].split(), np.uint32).reshape(s2.shape)
        st = out[4].split()
        assert st[0] == "stats"
        rows = [[int(v) for v in ln.split()] for ln in out[5:5 + len(starts)]]
        assert all(r[2] == len(r) - 3 for r in rows)
        return cost, P, np.array(st[1:], np.uint64), rows

    plan.run = run
    return plan


def _points(prm, dims, rng, n):
    """World points for goals and starts: cell centres, random ones in and round the field, non-finite and far ones."""
    lo = np.array(prm["origin"], np.float64)
    res = prm["resolution"]
    d = np.array(dims)
    centres = lo + (rng.integers(0, d, (n, 3)) + 0.5) * res
    odd = [[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]], [1e30, 0, 0], lo - 0.25 * res, lo + d * res + 0.25 * res]
    return np.concatenate([centres, rng.uniform(lo - res, lo + (d + 1) * res, (n // 2, 3)), odd]).astype(F)


def _hold(emu, prm, s2, pp, table, goals, starts):
    cost, P, st, rows = emu(prm, s2, pp, table, goals, starts)
    rc, rP, rst, adj = pr.build(prm, s2, pp, table, goals)
    assert np.array_equal(cost, rc)
    assert np.array_equal(P, rP), f"{np.sum(P != rP)} cells differ"
    assert list(st) == list(rst)
    status, pcost, off, cells = pr.paths(prm, rc, rP, adj, starts)
    for s, row in enumerate(rows):
        assert row[0] == status[s] and row[1] == pcost[s] and row[3:] == list(cells[int(off[s]):int(off[s + 1])]), s
    return P, status


@pytest.mark.parametrize("dims", [(12, 9, 7), (33, 5, 3), (1, 6, 5), (65, 1, 2), (1, 1, 1)])
def test_random_grids_3d(emu, dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx + 7 * ny)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=nz)
    pts = _points(prm, dims, rng, 16)
    seen = set()
    for density in (0.0, 0.2, 0.45):
        s2 = pr.random_s2(rng, (nz, ny, nx), density)
        for conn in (6, 18, 26):
            for table, clear in ((TABLE6, 1), (TABLE1, 2)):
                _, status = _hold(emu, prm, s2, pr.pparams(connectivity=conn, min_clear_s2=clear), table, pts[:5], pts)
                seen |= set(status.tolist())
    assert 2 in seen and (nx * ny * nz == 1 or 0 in seen)


@pytest.mark.parametrize("dims", [(12, 9), (33, 5), (1, 6), (65, 1), (1, 1), (34, 34)])
def test_random_grids_planar(emu, dims):
    nx, ny = dims
    rng = np.random.default_rng(3 * nx + ny)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=4)
    pts = _points(prm, (nx, ny, 1), rng, 16)
    pts[::3, 2] = np.nan   # (a planar field does not look at z)
    for density in (0.0, 0.2, 0.45):
        s2 = pr.random_s2(rng, (ny, nx), density)
        for conn in (4, 8):
            for table, clear in ((TABLE6, 1), (TABLE1, 5)):
                _hold(emu, prm, s2, pr.pparams(connectivity=conn, min_clear_s2=clear), table, pts[:5], pts)
        _hold(emu, prm, s2, pr.pparams(), TABLE6, pts[-5:], pts)   # every goal unusable


def test_limits_are_refused(emu):
    prm = ocr.params(nx=3, ny=2, nz=2)
    s3, s2 = np.full((2, 2, 3), pr.FAR, np.int32), np.full((2, 3), pr.FAR, np.int32)
    g = np.zeros((1, 3), F)
    bad = [(s3, dict(connectivity=8), TABLE6, g), (s3, dict(connectivity=4), TABLE6, g), (s2, dict(connectivity=6), TABLE6, g),
           (s2, dict(connectivity=26), TABLE6, g), (s2, dict(connectivity=5), TABLE6, g), (s2, dict(min_clear_s2=0), TABLE6, g),
           (s2, dict(min_clear_s2=pr.MAX_CLEAR + 1), TABLE6, g), (s2, dict(), np.zeros(0, np.uint8), g), (s2, dict(), np.ones(1026, np.uint8), g),
           (s2, dict(), np.array([5, 0, 5], np.uint8), g), (s2, dict(), TABLE6, np.zeros((0, 3), F)), (s2, dict(), TABLE6, np.zeros((65537, 3), F))]
    for field, kw, table, goals in bad:
        out = emu(prm, field, pr.pparams(**kw), table, goals)
        assert isinstance(out, str) and out.startswith("params bad"), kw
    good = [(s3, dict(connectivity=6)), (s3, dict(connectivity=18)), (s3, dict(connectivity=26)), (s2, dict(connectivity=4)), (s2, dict()),
            (s2, dict(min_clear_s2=pr.MAX_CLEAR))]
    for field, kw in good:
        assert not isinstance(emu(prm, field, pr.pparams(**kw), np.ones(1025, np.uint8), g), str), kw


def test_relax_at_the_overflow_edge(emu):
    U = pr.UNREACHED
    cases = [(0, 1, 1, 10), (U - 1 - 20, 1, 1, 10), (U - 20, 1, 1, 10), (U - 19, 1, 1, 10), (U - 1, 255, 255, 17), (U - 8670, 255, 255, 17),
             (U - 8671, 255, 255, 17), (U - 8669, 255, 255, 17), (U, 1, 1, 10), (U, 255, 255, 17), (12345, 7, 9, 14), (U - 2, 1, 1, 10)]
    want = []
    for pu, cu, cv, w in cases:
        s = pu + w * (cu + cv)   # (Python integers: the 64-bit sum)
        want.append(U if pu == U or s >= U else s)
    assert U - 1 in want and want.count(U) >= 6   # sums of 0xFFFFFFFE, 0xFFFFFFFF and above are all there
    out = emu.run("1\n%d\n%s\n" % (len(cases), "\n".join(" ".join(str(v) for v in c) for c in cases)))
    assert [int(v) for v in out[:len(cases)]] == want


def test_isqrt_at_every_perfect_square(emu):
    vals = sorted({v for r in range(0, 1773) for v in (r * r - 1, r * r, r * r + 1) if 0 <= v <= pr.MAX_CLEAR} | {pr.MAX_CLEAR, 2 ** 31 - 2, 2 ** 32 - 1})
    assert 1771 ** 2 <= pr.MAX_CLEAR < 1772 ** 2
    out = emu.run("2\n%d\n%s\n" % (len(vals), " ".join(str(v) for v in vals)))
    assert [int(v) for v in out[:len(vals)]] == [math.isqrt(v) for v in vals]
