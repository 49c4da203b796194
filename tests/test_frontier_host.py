"""The rule of lv_frontier.hpp (fr_state_*, fr_is_frontier, fr_neighbour, fr_order_key, fr_cluster_record, fr_rep_key,
fr_rank_window over lv_cluster.hpp's union-find: what the kernels of lv_frontier.hip run) compiled with g++ and
-fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to tests/frontier_ref.py: tests/emu/frontier_emu.cpp labels
a given grid cell after cell.  Labels, clusters, stats and ranks are equal, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import frontier_ref as fr
import occupancy_ref as ocr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("frontier_host") / "frontier_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "frontier_emu.cpp"), "-o", str(exe)])

    def run(prm, L, fp, P=None, reaches=()):
        nz, ny, nx = L.shape
        lines = [f"{_bits([prm['l_free'], prm['l_occ']])} {nx} {ny} {nz}", " ".join(str(fp[f]) for f in fr.FIELDS), _bits(L),
                 "0" if P is None else f"{P.size} {_ints(P)}", f"{len(reaches)} {_ints(reaches)}"]
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        if out[0] != "params ok":
            return out[0]
        shape = (ny, nx) if fp["planar"] else (nz, ny, nx)
        assert out[1].split() == ["field", str(nx), str(ny), str(1 if fp["planar"] else nz)]
        labels = np.array(out[2].split(), np.int32).reshape(shape)
        st = out[3].split()
        assert st[0] == "stats"
        C = int(st[4])
        cl = np.zeros(C, fr.CLUSTER_DTYPE)
        for c in range(C):
            v = [int(x) for x in out[4 + c].split()]
            cl[c] = (v[0], v[1], v[2], v[3:6], v[6:9], v[9:12], v[12:15])
        ranks = [(np.array(out[4 + C + 2 * r].split(), np.uint32), np.array(out[5 + C + 2 * r].split(), np.int32)) for r in range(len(reaches))]
        return labels, cl, np.array(st[1:], np.uint64), ranks

    return run


def _hold(emu, prm, L, fp, rng=None, reaches=(0, 1, 3)):
    rl, rcl, rst = fr.build(prm, L, fp)
    P = None
    if rng is not None:
        P = rng.integers(0, 5000, rl.shape).astype(np.uint32)
        P[rng.uniform(size=rl.shape) < 0.7] = fr.UNREACHED
    labels, cl, st, ranks = emu(prm, L, fp, P, reaches if P is not None else ())
    assert np.array_equal(labels, rl), (fp, f"{np.sum(labels != rl)} labels differ")
    assert np.array_equal(cl, rcl), fp
    assert list(st) == list(rst), fp
    for reach, (p, c) in zip(reaches, ranks):
        rp, rc = fr.rank(rl, len(rcl), P, reach)
        assert np.array_equal(p, rp) and np.array_equal(c, rc), (fp, reach)
    return rcl


@pytest.mark.parametrize("dims", [(12, 9, 7), (33, 5, 3), (1, 6, 5), (65, 1, 2), (1, 1, 1)])
def test_random_grids_3d(emu, dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx + 7 * ny)
    prm = ocr.params(nx=nx, ny=ny, nz=nz)
    for p_unknown in (0.1, 0.4):
        L = fr.random_logodds(rng, (nz, ny, nx), prm, p_unknown)
        for conn in (6, 18, 26):
            for min_size in (1, 3):
                _hold(emu, prm, L, fr.fparams(connectivity=conn, min_size=min_size), rng)


@pytest.mark.parametrize("dims", [(12, 9), (33, 5), (1, 6), (65, 1), (1, 1), (34, 34)])
def test_random_grids_planar(emu, dims):
    nx, ny = dims
    rng = np.random.default_rng(3 * nx + ny)
    prm = ocr.params(nx=nx, ny=ny, nz=4)
    for p_unknown in (0.3, 0.7):
        L = fr.random_logodds(rng, (4, ny, nx), prm, p_unknown)
        for conn in (4, 8):
            for k_lo, k_hi in ((0, 3), (1, 2), (-5, 0), (3, 9), (7, 9)):
                _hold(emu, prm, L, fr.fparams(planar=1, k_lo=k_lo, k_hi=k_hi, connectivity=conn, min_size=1 + (k_lo == 1)), rng)


def test_serpentine_and_thresholds(emu):
    prm = ocr.params(nx=9, ny=11, nz=2)
    L = fr.serpentine(prm, 9, 11, 2)
    for fp in (fr.fparams(connectivity=6), fr.fparams(connectivity=26), fr.fparams(planar=1, k_lo=0, k_hi=0, connectivity=4)):
        assert len(_hold(emu, prm, L, fp)) == 1
    prm = ocr.params(nx=4, ny=1, nz=1)
    between = F(0.5) * (F(prm["l_free"]) + F(prm["l_occ"]))
    for row in ([prm["l_free"], np.nan, prm["l_occ"], between], [np.nextafter(F(prm["l_free"]), F(0)), np.nan, between, np.nan]):
        L = np.array([[row]], F)
        _hold(emu, prm, L, fr.fparams(connectivity=6))
        _hold(emu, prm, L, fr.fparams(planar=1, connectivity=4))


def test_limits_are_refused(emu):
    prm = ocr.params(nx=3, ny=2, nz=2)
    L = np.full((2, 2, 3), np.nan, F)
    bad = [dict(connectivity=8), dict(connectivity=4), dict(planar=1, connectivity=6), dict(planar=1, connectivity=26), dict(connectivity=5),
           dict(min_size=0), dict(min_size=2 ** 28 + 1), dict(planar=1, connectivity=8, k_lo=2, k_hi=1)]
    for kw in bad:
        out = emu(prm, L, fr.fparams(**kw))
        assert isinstance(out, str) and out.startswith("params bad"), kw
    good = [dict(connectivity=6), dict(connectivity=18), dict(), dict(planar=1, connectivity=4), dict(planar=1, connectivity=8, k_lo=1, k_hi=1),
            dict(min_size=2 ** 28), dict(k_lo=2, k_hi=1)]
    for kw in good:
        assert not isinstance(emu(prm, L, fr.fparams(**kw)), str), kw
