"""tests/mcl_ref.py pinned on cases worked out by hand: one particle, three beams, a 4 x 4 field of unit cells at the origin.  What
holds the host build of lv_mcl.hpp and the kernel is this reference, so it is held to the rule's text first; and the host side of
limo_velo_amd.mcl (tables, resampling, estimate), which needs no device."""
import numpy as np
import pytest

import mcl_ref as mr

F = np.float32
FAR = 2147483647
NO = np.uint64(mr.NO_SCORE)
S2 = np.array([[0, 1, 4, 9],
               [1, 2, 5, 10],
               [4, 5, 8, FAR],
               [-3, 10, 13, 18]], np.int32)     # [j, i]
FIELD = dict(origin=(0.0, 0.0, 0.0), resolution=1.0, s2=S2)
TABLE = np.array([10, 20, 30, 40, 50, 60], np.uint32)   # idx = 0 for s2 <= 0, else min(s2, 5)


def _one(pose, beams, field=FIELD, table=TABLE, **mp):
    out = mr.weigh(field, mr.mparams(**mp), np.array([pose], F), np.array(beams, F), table)
    return int(out["score"][0]), int(out["n_in"][0]), list(out["best"])


def test_heading_zero():
    # (0.5, 0.5) + (1, 0) = (1.5, 0.5): cell (1, 0), s2 1 -> 20; + (2, 2) = (2.5, 2.5): cell (2, 2), s2 8 -> entry 5 = 60;
    # + (5, 0) = (5.5, 0.5): outside -> out_cost 7
    assert _one((0.5, 0.5, 0.0, 0.0), [(1, 0, 0), (2, 2, 0), (5, 0, 0)], out_cost=7) == (87, 2, [0, 87])
    # LV_OCC_FAR at (3, 2) -> the last entry 60; -3 at (0, 3) -> entry 0 = 10; s2 0 at (0, 0) -> entry 0 = 10
    assert _one((0.5, 0.5, 0.0, 0.0), [(3, 2, 0), (0, 3, 0), (0, 0, 0)]) == (80, 3, [0, 80])
    # z is not looked at in a planar field
    assert _one((0.5, 0.5, np.nan, 0.0), [(3, 2, np.inf), (0, 3, -5.0), (0, 0, 0)]) == (80, 3, [0, 80])


def test_heading_quarter_turn():
    # th = f32(pi / 2): sn = 1, cs = -4.371139e-08.  Beam (1, 0): px = 0.5 + (cs - 0) = 0.49999997 -> i 0; py = 0.5 + (1 + cs * 0) = 1.5
    # -> j 1: s2 1 -> 20.  Beam (2, -2): px = 0.5 + (2 cs + 2) = 2.5, py = 0.5 + (2 - 2 cs) = 2.5: cell (2, 2) -> 60.  Beam (0, -3):
    # px = 0.5 + (0 + 3) = 3.5, py = 0.5 + (0 - 3 cs) = 0.5000001: cell (3, 0), s2 9 -> 60.
    th = float(F(np.pi / 2))
    sn, cs = mr.rr.sincos(F(th))
    assert sn == F(1.0) and cs == F(-4.371139e-08)
    assert _one((0.5, 0.5, 0.0, th), [(1, 0, 0), (2, -2, 0), (0, -3, 0)]) == (140, 3, [0, 140])
    # a quarter turn the other way sends (1, 0) to (0.5, -0.5): outside, out_cost 0 by default; one beam inside meets min_inside 1
    assert _one((0.5, 0.5, 0.0, -th), [(1, 0, 0), (0, 0, 0)]) == (10, 1, [0, 10])
    assert _one((0.5, 0.5, 0.0, -th), [(1, 0, 0), (0, 0, 0)], min_inside=2) == (int(NO), 1, [-1, -1])


def test_volume_and_table_sizes():
    vol = dict(FIELD, s2=np.stack([S2, np.where(S2 == FAR, FAR, S2 + (S2 != FAR))]))   # layer 1: every finite value one more
    # pz = 0.25 + 1 = 1.25: layer 1; cell (1, 0): 1 + 1 = 2 -> 30.  pz = 0.25 - 1 < 0: outside.  pz = 0.25 + 0.5: layer 0, (2, 1): 5 -> 60
    assert _one((0.5, 0.5, 0.25, 0.0), [(1, 0, 1), (1, 0, -1), (2, 1, 0.5)], field=vol, out_cost=3) == (93, 2, [0, 93])
    assert _one((0.5, 0.5, 0.25, 0.0), [(1, 0, np.nan)], field=vol, out_cost=3, min_inside=0) == (3, 0, [0, 3])
    # n_table 1: everything inside costs table[0]; n_table 2: s2 <= 0 -> 0, the rest -> 1
    beams = [(0, 0, 0), (1, 0, 0), (3, 2, 0), (0, 3, 0)]   # s2 0, 1, FAR, -3
    assert _one((0.5, 0.5, 0.0, 0.0), beams, table=np.array([7], np.uint32)) == (28, 4, [0, 28])
    assert _one((0.5, 0.5, 0.0, 0.0), beams, table=np.array([1, 100], np.uint32)) == (202, 4, [0, 202])


def test_unusable_headings_best_and_the_sum():
    beams = np.array([(1, 0, 0), (2, 2, 0), (0, 0, 0)], F)   # at heading 0 from (0.5, 0.5): 20 + 60 + 10
    poses = np.array([(0.5, 0.5, 0, 1048576.0), (0.5, 0.5, 0, 0), (0.5, 0.5, 0, np.nan), (0.5, 0.5, 0, 0), (1.5, 0.5, 0, 0)], F)
    out = mr.weigh(FIELD, mr.mparams(), poses, beams, TABLE)
    # particle 4: (2.5, 0.5) s2 4 -> 50; (3.5, 2.5) FAR -> 60; (1.5, 0.5) s2 1 -> 20
    assert list(out["score"]) == [NO, 90, NO, 90, 130] and list(out["n_in"]) == [0, 3, 0, 3, 3] and list(out["best"]) == [1, 90]
    assert list(mr.weigh(FIELD, mr.mparams(min_inside=3), poses[[0, 2]], beams, TABLE)["best"]) == [-1, -1]
    # 300 beams of 2^24: the sum passes 2^32
    big = mr.weigh(FIELD, mr.mparams(), poses[1:2], np.zeros((300, 3), F), np.array([2 ** 24], np.uint32))
    assert int(big["score"][0]) == 300 * 2 ** 24 == 5033164800 and list(big["best"]) == [0, 5033164800]


# ---- the host side of limo_velo_amd.mcl
@pytest.fixture(scope="module")
def mcl(lv):
    from limo_velo_amd import mcl as m

    return m


def test_tables(mcl):
    t = mcl.likelihood_table(0.25, 0.2, 0.95, 0.05, 8.0, 16.0, 1024)
    assert t.dtype == np.uint32 and len(t) == 1024 and t[0] == 0 and np.all(np.diff(t.astype(np.int64)) >= 0)
    p = 0.95 * np.exp(-np.arange(3) * 0.0625 / 0.08) + 0.05 / 8.0
    assert list(t[:3]) == [int(np.rint(16.0 * (-np.log(p[k]) + np.log(p[0])))) for k in range(3)]
    assert t[-1] == int(np.rint(16.0 * (-np.log(0.05 / 8.0) + np.log(p[0]))))   # far away only the random part is left
    w = mcl.weight_table(16.0, 2.0, 64, shift=1)
    assert w[0] == 2 ** 20 and list(w[:3]) == [int(np.rint(2 ** 20 * np.exp(-2 * d / 32.0))) for d in range(3)] and w.max() <= mcl.MAX_WEIGHT


def test_resample_is_the_integer_rule(mcl):
    wt = np.array([8, 4, 2, 1], np.uint32)
    score = np.array([105, 100, mr.NO_SCORE, 102, 200, 100], np.uint64)
    # s_min 100, shift 1: d = 2, 0, -, 1, 50 -> 3, 0: w = 2, 8, 0, 4, 1, 8; C = 2, 10, 10, 14, 15, 23; W = 23
    anc, W, sw2, s_min = mcl.resample(score, wt, 1, 23 * 5 + 7, 4)
    assert (W, sw2, s_min) == (23, 4 + 64 + 16 + 1 + 64, 100)
    # r = 7; t_j = (23 j + 7) // 4 = 1, 7, 13, 19; the smallest i with C_i > t: 0, 1, 3, 5
    assert list(anc) == [0, 1, 3, 5]
    assert list(mcl.weights(score, wt, 1)) == [2, 8, 0, 4, 1, 8]
    assert mcl.n_eff(W, sw2) == 23 * 23 / 149
    anc, W, sw2, s_min = mcl.resample(np.full(3, mr.NO_SCORE, np.uint64), wt, 0, 5, 4)
    assert list(anc) == [-1] * 4 and (W, sw2, s_min) == (0, 0, -1)
    anc, W, _, _ = mcl.resample(np.array([0, 9], np.uint64), np.array([0], np.uint32), 0, 5, 2)
    assert list(anc) == [-1, -1] and W == 0
    # every particle drawn in proportion: M = W gives each i exactly w_i times
    anc, W, _, _ = mcl.resample(score, wt, 1, 12345, 23)
    assert list(np.bincount(anc, minlength=6)) == [2, 8, 0, 4, 1, 8]


def test_estimate_particles_and_motion(mcl):
    poses = np.array([(0, 0, 1, np.pi - 0.1), (2, 4, 1, -np.pi + 0.1), (9, 9, 9, 0)], F)
    e = mcl.estimate(poses, [1, 1, 0])
    assert np.allclose(e[:3], [1, 2, 1]) and abs(abs(e[3]) - np.pi) < 1e-6      # the circular mean, not the arithmetic one
    assert np.all(np.isnan(mcl.estimate(poses, [0, 0, 0])))
    rng = np.random.default_rng(3)
    g = mcl.gaussian_particles((1.0, 2.0, 0.3, 0.5), 0.1, 0.05, 4000, rng)
    assert g.dtype == F and g.shape == (4000, 4) and np.all(g[:, 2] == F(0.3))
    assert np.allclose(g.mean(axis=0), [1.0, 2.0, 0.3, 0.5], atol=0.01) and np.allclose(g[:, [0, 1, 3]].std(axis=0), [0.1, 0.1, 0.05], atol=0.01)
    f = dict(origin=(0.0, 0.0, 0.0), resolution=1.0, s2=S2)
    u = mcl.uniform_particles(None, 2000, rng, z=0.2, min_clear_s2=9, field=f)
    ij = np.floor(u[:, :2]).astype(int)
    assert set(map(tuple, ij)) == {(3, 0), (3, 1), (3, 2), (1, 3), (2, 3), (3, 3)} and np.all(u[:, 2] == F(0.2)) and np.all(np.abs(u[:, 3]) <= np.pi)
    # noise-free motion is the odometry step itself
    d = mcl.odometry_delta((0.0, 0.0, 0.0), (1.0, 1.0, np.pi / 2))
    assert np.allclose(d, (np.pi / 4, np.sqrt(2.0), np.pi / 4))
    m = mcl.move(np.array([(1, 1, 0.3, np.pi / 2)], F), d, (0, 0, 0, 0), rng)
    assert np.allclose(m[0], [0.0, 2.0, 0.3, -np.pi], atol=1e-6) or np.allclose(m[0], [0.0, 2.0, 0.3, np.pi], atol=1e-6)
    b = mcl.beams_from_scan(np.array([(1, 0, 0), (np.inf, 0, 0), (0, 2, 0), (0, 0, 0), (9, 0, 0), (0, 3, 0), (np.nan, 1, 1), (4, 0, 0)]), 2, 8.0)
    assert b.dtype == F and b.tolist() == [[1, 0, 0], [0, 3, 0]]   # (the returns: 1, 2, 3, 4 m; two of four, evenly)
