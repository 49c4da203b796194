"""The resident localisation filter's rule as tests/mcl_filter_ref.py states it, on the CPU alone: the pinned draws, the moments of
the normals, the resampling against limo_velo_amd.mcl.resample as it stands, the decision at its boundary, the heading's wrap at
+-pi, and mcl.estimate_from_stats against a direct f64 mean."""
import math

import numpy as np
import pytest

import mcl_cases as cases
import mcl_filter_ref as fr
import mcl_ref as mr

F = np.float32
NO = np.uint64(mr.NO_SCORE)


@pytest.fixture(scope="module")
def mcl(lv):
    from limo_velo_amd import mcl as m

    return m


def test_pinned_draws():
    assert fr.mix(0) == 0xe220a8397b1dcdaf
    assert fr.word(0, 0, 0, 0) == 0x238275bc38fcbe91
    assert fr.word(1, 2, 3, 4) == 0x4c6229bfb481eb4c
    assert fr.normals_g(0, 0, 1)[0].tolist() == [-49358, -160660, -194366]
    assert int(fr.normals_g(7, 1, 1, first=5)[0, 2]) == -3608
    assert int(fr.mix_np(np.array([0], np.uint64))[0]) == fr.mix(0)
    assert fr.resample_draw(3, 9) == fr.mix(fr.mix(fr.mix(3) ^ 9) ^ (2 ** 64 - 1))
    # the vectorised words are the scalar ones
    b = np.uint64(fr.base(5, 6))
    for i, j in ((0, 0), (1, 8), (2 ** 20 - 1, 3)):
        assert int(fr.mix_np(b ^ np.array([(i << 8) | j], np.uint64))[0]) == fr.word(5, 6, i, j)


def test_normals_bound_and_moments():
    g = fr.normals_g(11, 0, 40000)   # 120 000 normals from one seed
    assert g.size == 120000 and np.abs(g).max() <= 786420 and 12 * 65535 == 786420
    z = g.astype(np.float64).reshape(-1) / 2.0 ** 17
    assert np.array_equal((g.astype(F) * F(2.0 ** -17)).astype(np.float64).reshape(-1), z)   # exact in f32
    print("mean", z.mean(), "std", z.std(), "fourth moment", (z ** 4).mean())
    assert abs(z.mean()) <= 0.02 and abs(z.std() - 1.0) <= 0.02 and 2.8 <= (z ** 4).mean() <= 3.05
    # the three normals of a particle are not one another's copies, nor are two epochs or two seeds
    assert np.mean(g[:, 0] == g[:, 1]) < 0.001 and np.mean(g[:, 1] == g[:, 2]) < 0.001 and abs(np.corrcoef(z[0::3], z[1::3])[0, 1]) < 0.02
    assert not np.array_equal(g, fr.normals_g(11, 1, 40000)) and not np.array_equal(g, fr.normals_g(12, 0, 40000))


def _resample_both(mcl, acc, wtable, shift, draw):
    K = len(acc)
    anc, W, sw2, s_min = mcl.resample(acc, wtable, shift, draw, K)
    w, s_min_ref = fr.weights(acc, wtable, shift)
    assert (int(w.sum()), int((w * w).sum()), s_min_ref) == (W, sw2, s_min)
    assert np.array_equal(w, mcl.weights(acc, wtable, shift))
    if W:
        assert np.array_equal(fr.ancestors(w, draw), anc)
    else:
        assert np.all(anc == -1)
    return anc, W


def test_resampling_equals_mcl_resample(mcl):
    rng = np.random.default_rng(0)
    wt = mcl.weight_table(16.0, 4.0, 4096)
    for K in (1, 2, 255, 256, 257, 5000):
        for shift in (0, 3):
            acc = rng.integers(0, 3000, K).astype(np.uint64) + np.uint64(10 ** 9)
            acc[rng.uniform(size=K) < 0.2] = NO
            for draw in (0, 1, int(rng.integers(0, 2 ** 63)), 2 ** 64 - 1):
                _resample_both(mcl, acc, wt, shift, draw)
    # one heavy particle; all weights equal; all zero; none eligible; K = 1
    acc = np.full(300, 10 ** 6, np.uint64)
    acc[123] = 5
    anc, W = _resample_both(mcl, acc, np.array([7, 0], np.uint32), 0, 12345)
    assert W == 7 and np.all(anc == 123)
    anc, W = _resample_both(mcl, np.full(300, 42, np.uint64), np.array([3], np.uint32), 0, 2 ** 64 - 1)
    assert W == 900 and np.array_equal(anc, np.arange(300))
    anc, W = _resample_both(mcl, np.arange(300, dtype=np.uint64), np.zeros(5, np.uint32), 0, 99)
    assert W == 0
    anc, W = _resample_both(mcl, np.full(300, NO, np.uint64), wt, 0, 99)
    assert W == 0 and fr.weights(np.full(300, NO, np.uint64), wt, 0)[1] == -1
    anc, W = _resample_both(mcl, np.array([17], np.uint64), wt, 0, 99)
    assert list(anc) == [0]
    anc, W = _resample_both(mcl, np.array([NO], np.uint64), wt, 0, 99)
    assert W == 0


def test_the_decision_at_its_boundary():
    # W^2 * den = 72 against num * K * sum_w2 = 71, 72, 73
    assert [fr.decide(1, 6, s, 1, 1, 2) for s in (71, 72, 73)] == [False, False, True]
    # beyond 64 bits: 2^96 on both sides
    W, K, s = 2 ** 40, 2 ** 20, 2 ** 60
    assert [fr.decide(1, W, s + d, K, 65536, 65536) for d in (-1, 0, 1)] == [False, False, True]
    assert not fr.decide(0, W, 10 * s, K, 1, 1) and fr.decide(2, 1, 1, K, 1, 65536) and not fr.decide(2, 0, 0, K, 1, 1) and not fr.decide(1, 0, 0, K, 1, 1)


def test_the_heading_wrap_at_pi():
    """sigma = 0 and rot1 = 0: th = (th0 + 0) + rot2, so th0 = 0 puts rot2 itself through the wrap."""
    pi = fr.PI_F
    inside, beyond = np.nextafter(pi, F(0)), np.nextafter(pi, F(4))
    for rot2, want in ((pi, pi - fr.TWO_PI_F), (inside, inside), (beyond, beyond - fr.TWO_PI_F), (-pi, -pi), (-inside, -inside),
                       (-beyond, -beyond + fr.TWO_PI_F)):
        x = fr.move(np.array([[1.0, 2.0, 0.5, 0.0]], F), 3, 0, (0.0, 0.0, rot2), (0.0, 0.0, 0.0))
        assert x[0, 3].view(np.uint32) == F(want).view(np.uint32), (rot2, x[0, 3], want)
        assert x[0, :3].tolist() == [1.0, 2.0, 0.5]
    assert F(pi - fr.TWO_PI_F) < 0 and F(-beyond + fr.TWO_PI_F) > 0
    # each step happens once: a heading far beyond pi is not brought all the way back
    x = fr.move(np.array([[0.0, 0.0, 0.0, 0.0]], F), 3, 0, (0.0, 0.0, 20.0), (0.0, 0.0, 0.0))
    assert x[0, 3] == F(F(20.0) - fr.TWO_PI_F)


def test_the_move_is_the_motion_model():
    """With sigma = 0 every particle makes the noise-free step; with noise the spread of the steps is sigma's."""
    x0 = np.tile(np.array([[1.0, -1.0, 0.3, 0.5]], F), (20000, 1))
    d = (0.1, 0.3, 0.05)
    x = fr.move(x0, 1, 0, d, (0.0, 0.0, 0.0))
    assert np.allclose(x[0], [1.0 + 0.3 * math.cos(0.6), -1.0 + 0.3 * math.sin(0.6), 0.3, 0.65], atol=1e-6) and np.all(x == x[0])
    y = fr.move(x0, 1, 0, d, (0.02, 0.03, 0.01))
    step = np.hypot(y[:, 0] - 1.0, y[:, 1] + 1.0)
    assert abs(step.mean() - 0.3) < 1e-3 and abs(step.std() - 0.03) < 1e-3
    assert abs((y[:, 3] - 0.65).std() - math.hypot(0.02, 0.01)) < 1e-3 and np.all(y[:, 2] == F(0.3))
    assert not np.array_equal(y, fr.move(x0, 2, 0, d, (0.02, 0.03, 0.01))) and not np.array_equal(y, fr.move(x0, 1, 1, d, (0.02, 0.03, 0.01)))


def test_estimate_from_stats(mcl):
    """Against a direct f64 weighted mean: within half a sub-unit (resolution / 512) per axis plus the quantisation's own half, and
    the heading within the 2^-20 of its sine and cosine."""
    rng = np.random.default_rng(4)
    f = cases.field("planar")
    K = 3000
    x = mcl.gaussian_particles((3.0, 1.0, 0.3, 0.5), 0.3, 0.2, K, rng)
    ctx = fr.RefFilterContext(f)
    ctx.occ_mcl_filter_set(x, 0)
    ctx.acc = rng.integers(0, 400, K).astype(np.uint64)
    wt = mcl.weight_table(16.0, 4.0, 4096)
    st, _ = ctx.occ_mcl_filter_resample(wt, fr.rparams(mode=0))
    got = mcl.estimate_from_stats(st)
    w = fr.weights(ctx.acc, wt, 0)[0].astype(np.float64)
    want = mcl.estimate(x, w)
    sub = f["resolution"] / 256.0
    assert st.n_clamped == 0 and st.n_eligible == K and st.W == int(w.sum())
    assert np.all(np.abs(got[:3] - want[:3]) <= 0.5 * sub + 1e-9), (got, want)
    assert abs(got[3] - want[3]) <= 4.0 / 1048576.0
    # no weight: NaN
    st0, _ = ctx.occ_mcl_filter_resample(np.zeros(3, np.uint32), fr.rparams(mode=2))
    assert st0.W == 0 and st0.resampled == 0 and np.all(np.isnan(mcl.estimate_from_stats(st0)))
    # particles far outside are clamped and counted
    far = x.copy()
    far[:5, 0] = [1.0e9, -1.0e9, np.nan, np.inf, 4.0]
    far[5, 3] = np.nan
    ctx.occ_mcl_filter_set(far, 0)
    st1, _ = ctx.occ_mcl_filter_resample(wt, fr.rparams(mode=0))
    assert st1.n_clamped == 4
    q, _ = fr.terms(f, far)
    assert q[:4, 0].tolist() == [1 << 22, -(1 << 22), 0, 0] and q[5, 3:].tolist() == [0, 0]


def test_motion_sigmas_and_the_below_fraction(mcl):
    d, a = (0.1, 0.3, -0.05), (0.02, 0.03, 0.04, 0.05)
    s = mcl.motion_sigmas(d, a)
    assert s.dtype == F and np.allclose(s, [math.sqrt(0.02 * 0.01 + 0.03 * 0.09), math.sqrt(0.04 * 0.09 + 0.05 * 0.01 + 0.05 * 0.0025),
                                            math.sqrt(0.02 * 0.0025 + 0.03 * 0.09)])
    assert mcl.below_fraction(0.5) == (32768, 65536) and mcl.below_fraction(0.0) == (1, 65536) and mcl.below_fraction(2.0) == (65536, 65536)


def test_the_reference_filter_tracks(mcl):
    """The reference filter alone over the ten cycles of mcl_cases, seeds 0..4: the figures the GPU test's bound is taken from
    (DESIGN.md "Resident localisation filter")."""
    truth = cases.true_poses()
    scans = [cases.scan_beams(cases.ref_ranges(p)) for p in truth[1:]]
    table, wtable = cases.tables()
    worst_m = worst_rad = 0.0
    for seed in range(5):
        p0 = mcl.gaussian_particles(cases.TRUE_START, 0.3, 0.15, cases.TRACK_K, np.random.default_rng(seed))
        h = mcl.DeviceFilter(fr.RefFilterContext(cases.field("planar")), p0, seed).track(cases.ODOMETRY, scans, table, wtable, alphas=cases.ALPHAS)
        err_m, err_rad = cases.track_error(h)
        print("seed", seed, "error", err_m, "m", err_rad, "rad", "resamplings", sum(s["resampled"] for s in h))
        assert sum(s["resampled"] for s in h) >= 3
        worst_m, worst_rad = max(worst_m, err_m), max(worst_rad, err_rad)
    # twice the worst stays below the floor of one cell and 10 degrees, so the floor is the GPU test's bound
    assert 2.0 * worst_m <= 0.25 and 2.0 * worst_rad <= math.radians(10.0)
