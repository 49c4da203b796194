"""tests/distance_ref.py, the numpy statement of the distance field's rule, against an O(N^2) brute force over all voxel pairs and
(where scipy is importable) against scipy.ndimage.distance_transform_edt; and occupancy.costmap_from_distance on a hand-made array."""
import numpy as np
import pytest

import distance_ref as dr
import occupancy_ref as ocr

F = np.float32


def _masks(rng, shape):
    n = int(np.prod(shape))
    one = np.zeros(n, bool)
    one[rng.integers(n)] = True
    return [np.zeros(shape, bool), one.reshape(shape), rng.uniform(size=shape) < 0.05, rng.uniform(size=shape) < 0.5, np.ones(shape, bool)]


@pytest.mark.parametrize("shape", [(7, 9, 12), (1, 9, 12), (5, 1, 3), (1, 1, 1), (3, 4, 1)])
def test_transform_against_brute_force(shape):
    rng = np.random.default_rng(sum(shape))
    for mask in _masks(rng, shape):
        out, inn = dr.brute(mask), dr.brute(~mask)
        assert np.array_equal(dr.edt2(mask), out) and np.array_equal(dr.edt2(~mask), inn)
        for signed in (0, 1):
            for mc in (0, 1, 3):
                s2 = dr.field(mask, dr.dparams(signed_field=signed, max_cells=mc))
                want = np.where(mask, -inn if signed else 0, out)
                want = np.where(np.abs(want) >= dr.BIG, np.sign(want) * dr.FAR, want)
                if mc:
                    want = np.where(np.abs(want) > mc * mc, np.sign(want) * dr.FAR, want)
                assert s2.dtype == np.int32 and np.array_equal(s2, want)
                st = dr.stats(s2, mask.sum())
                fin = np.abs(want) != dr.FAR
                assert st[0] == mask.sum() and st[1] == fin.sum()
                assert st[2] == max([0] + list(want[fin & (want > 0)])) and st[3] == max([0] + list(-want[fin & (want < 0)]))
    assert np.all(dr.field(np.zeros(shape, bool), dr.dparams(signed_field=1)) == dr.FAR)
    assert np.all(dr.field(np.ones(shape, bool), dr.dparams(signed_field=1)) == -dr.FAR)
    assert np.all(dr.field(np.ones(shape, bool), dr.dparams()) == 0)


def test_transform_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for density in (0.002, 0.05, 0.5):
        mask = rng.uniform(size=(17, 33, 40)) < density
        assert mask.any()
        want = np.round(ndi.distance_transform_edt(~mask) ** 2).astype(np.int64)
        assert np.array_equal(dr.edt2(mask), want)


def test_mask_metres_and_query():
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=6, ny=5, nz=4)
    L = np.full((4, 5, 6), np.nan, F)
    L[1, 2, 3] = 0.4      # exactly l_occ: an obstacle
    L[2, 2, 3] = 0.39     # between l_free and l_occ: not one
    L[3, 0, 0] = -0.4     # free
    m = dr.obstacle_mask(prm, L, dr.dparams())
    assert m.sum() == 1 and m[1, 2, 3]
    assert dr.obstacle_mask(prm, L, dr.dparams(unknown_is_obstacle=1)).sum() == 4 * 5 * 6 - 2
    # planar over the layers 2..9 (clipped to 2..3): column (2, 3) is -1 (0.39 decides nothing), column (0, 0) is free, no cell is 100
    assert dr.obstacle_mask(prm, L, dr.dparams(planar=1, k_lo=2, k_hi=9)).sum() == 0
    pm = dr.obstacle_mask(prm, L, dr.dparams(planar=1, k_lo=2, k_hi=9, unknown_is_obstacle=1))
    assert pm.shape == (1, 5, 6) and pm.sum() == 29 and not pm[0, 0, 0]
    s2, st = dr.build(prm, L, dr.dparams())
    assert s2[1, 2, 3] == 0 and s2[1, 2, 0] == 9 and s2[0, 0, 0] == 9 + 4 + 1 and list(st) == [1, 120, 9 + 4 + 4, 0]
    met = dr.metres(np.array([0, 4, -9, dr.FAR, -dr.FAR, 2], np.int32), 0.25)
    assert dr.same_bits(met, np.array([0.0, 0.5, -0.75, np.inf, -np.inf, F(0.25) * np.sqrt(F(2))], F)) and not np.signbit(met[0])
    # the voxel (0, 2, 1): dx = 3 to the obstacle; its x neighbours are the border (one-sided) and (1, 2, 1) at dx = 2
    pts = np.array([[-0.9, 1.1, 2.3], [-0.9, 1.1, np.nan], [5.0, 1.1, 2.3], [np.inf, 1.1, 2.3]], F)
    dist, grad = dr.query(prm, dr.dparams(), s2, pts)
    assert dist[0] == F(0.75) and grad[0, 0] == F(-1.0) and grad[0, 1] == (np.sqrt(F(10)) * F(0.25) - np.sqrt(F(10)) * F(0.25)) / F(0.5)
    assert np.isnan(dist[1:]).all() and not grad[1:].any()
    p2, _ = dr.build(prm, L, dr.dparams(planar=1, k_lo=0, k_hi=3))
    dist, grad = dr.query(prm, dr.dparams(planar=1), p2, pts)
    assert dist[0] == F(0.75) and dist[1] == F(0.75) and np.isnan(dist[2:]).all() and not grad[:, 2].any()


def test_costmap_from_distance(lv):
    from limo_velo_amd import occupancy

    d = np.array([[0.0, 0.1, 0.3, 0.30001, 0.5], [1.0, 1.0001, np.inf, np.nan, -0.2]])
    c = occupancy.costmap_from_distance(d, 0.3, 1.0, cost_scaling_factor=3.0)
    assert c.dtype == np.uint8 and c.shape == d.shape
    assert list(c[0]) == [254, 253, 253, int(252 * np.exp(-3.0 * (0.30001 - 0.3))), int(252 * np.exp(-3.0 * 0.2))]
    assert list(c[1]) == [int(252 * np.exp(-3.0 * 0.7)), 0, 0, 0, 254]
    assert c[0, 3] == 251 and c[0, 4] == 138 and c[1, 0] == 30
    assert occupancy.costmap_from_distance(np.array([0.35]), 0.3, 1.0)[0] == int(252 * np.exp(-10.0 * (0.35 - 0.3)))
