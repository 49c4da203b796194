"""CPU checks of the reference itself (tests/surf_occ_ref.py, the numpy statement of lv_occ_from_surface's rule) and of the scene
(tests/surf_occ_cases.py): every one of the 27 combinations reaches every class, the coarse grid sticks out of the volume, REPLACE
is idempotent, FILL after REPLACE changes nothing and never touches an observed voxel, `reach` is a binary dilation of the solid
set in volume space, and on grids made like the volume (mesh.like_occupancy) every centre quantises back into its own voxel."""
import numpy as np
import pytest

import surf_occ_cases as sc
import surf_occ_ref as sr

F = np.float32


@pytest.fixture(scope="module")
def vol():
    return sc.volume()


def test_the_volume_is_loadable(vol):
    S, W = vol
    assert S.shape == (sc.NZ, sc.NY, sc.NX) and W.min() == 0 and W.max() == 5 and set(np.unique(W)) == {0, 1, 2, 5}
    assert (np.abs(S.astype(np.int64)) <= sc.T * W.astype(np.int64)).all() and W.max() <= sc.MAX_WEIGHT   # lv_tsdf_load's check
    solid, _ = sr.voxel_classes(S, W, 1, 0)
    wall = solid[:, :, 20:]
    i = np.nonzero(wall.any(axis=(0, 1)))[0] + 20
    assert i.min() == 28 and i.max() == 35   # across the 31 | 32 word boundary


@pytest.mark.parametrize("name,min_weight,band,reach", sc.combinations())
def test_every_combination_reaches_every_class(vol, name, min_weight, band, reach):
    cls, outside = sr.classify(sc.grid_geometry(name), sc.vol_geometry(), *vol, min_weight, band, reach)
    counts = [int((cls == c).sum()) for c in (sr.NONE, sr.FREE, sr.OCCUPIED)]
    print(f"{name} min_weight {min_weight} band {band} reach {reach}: NONE {counts[0]}, FREE {counts[1]}, OCCUPIED {counts[2]}, OUTSIDE {int(outside.sum())}")
    assert min(counts) >= 50
    assert not (outside & (cls != sr.NONE)).any()
    if name == "coarse":
        assert outside.sum() > 3000
    if name == "same":
        assert not outside.any()


@pytest.mark.parametrize("name", list(sc.GRIDS))
def test_replace_is_idempotent_and_fill_respects_evidence(vol, name):
    grid, v = sc.grid_geometry(name), sc.vol_geometry()
    L0 = sc.random_grid(grid["shape"], 5)
    kw = dict(min_weight=1, band=0, reach=1)
    L1, st1 = sr.from_surface(L0, grid, v, *vol, mode=sr.REPLACE, **kw)
    L2, st2 = sr.from_surface(L1, grid, v, *vol, mode=sr.REPLACE, **kw)
    assert st1[2] > 0 and st2[2] == 0 and np.array_equal(L1.view(np.uint32), L2.view(np.uint32)) and np.array_equal(st1[[0, 1, 3]], st2[[0, 1, 3]])
    L3, st3 = sr.from_surface(L1, grid, v, *vol, mode=sr.FILL, **kw)
    assert st3[2] == 0 and np.array_equal(L1.view(np.uint32), L3.view(np.uint32))
    # FILL on the random grid: observed voxels keep their bits, unknown ones of a class are written
    L4, st4 = sr.from_surface(L0, grid, v, *vol, mode=sr.FILL, **kw)
    seen = ~np.isnan(L0)
    assert np.array_equal(L4[seen].view(np.uint32), L0[seen].view(np.uint32)) and 0 < st4[2] < st1[2]
    cls, _ = sr.classify(grid, v, *vol, **kw)
    assert st4[2] == (~seen & (cls != sr.NONE)).sum()
    # every value written is NaN or inside the clamps
    for L in (L1, L4, sr.from_surface(L0, grid, v, *vol, mode=sr.ACCUMULATE, **kw)[0], sr.from_surface(L0, grid, v, *vol, mode=sr.OVERWRITE, **kw)[0]):
        ok = np.isnan(L) | ((L >= F(sc.L_MIN)) & (L <= F(sc.L_MAX)))
        assert ok.all()


@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_reach_is_a_dilation_in_volume_space(vol, reach):
    """on the volume's own geometry every occupancy voxel is its own TSDF voxel, so the OCCUPIED set is the grown solid set: held
    here to a dilation written another way (the voxels within Chebyshev distance `reach` of a solid one, by brute force)"""
    grid = v = sc.vol_geometry()
    base, _ = sr.classify(grid, v, *vol, 1, 0, 0)
    grown, _ = sr.classify(grid, v, *vol, 1, 0, reach)
    k, j, i = np.nonzero(base == sr.OCCUPIED)
    want = np.zeros(base.shape, bool)
    for kk, jj, ii in zip(k, j, i):
        want[max(kk - reach, 0):kk + reach + 1, max(jj - reach, 0):jj + reach + 1, max(ii - reach, 0):ii + reach + 1] = True
    assert np.array_equal(grown == sr.OCCUPIED, want) and want.sum() > (base == sr.OCCUPIED).sum()
    # free space is never grown: FREE shrinks exactly by what became OCCUPIED
    assert np.array_equal(grown == sr.FREE, (base == sr.FREE) & ~want)


@pytest.mark.parametrize("shift", [0, 37, -1000, 1 << 20])
def test_a_like_made_grid_maps_onto_its_own_voxels(shift):
    """the default grids (512 x 512 x 64 at 0.2 m from (-51.2, -51.2, -3.2)) at one shift on every axis: u = v, and the remainder
    of the quantised centre stays within 8 sub-units of 128"""
    origin0, res, shape = (-51.2, -51.2, -3.2), 0.2, (64, 512, 512)
    g = sr.geometry(sr.origin_at(origin0, (shift,) * 3, res), res, shape)
    for a, (inside, u) in enumerate(sr.voxel_of(g, g)):
        n = shape[2 - a]
        assert inside.all() and np.array_equal(u, np.arange(n))
        _, q = sr.quantise(sr.centres(g["origin"][a], res, n), g["origin"][a], res)
        assert np.abs((q & 255) - 128).max() <= 8


def test_the_box_is_clipped_as_marks():
    assert sr.clip_box((4, 5, 6), (-3, 1, 0), (2, 99, 3)) == (slice(0, 4), slice(1, 5), slice(0, 3))
    assert sr.clip_box((4, 5, 6), (6, 0, 0), (9, 9, 9)) is None and sr.clip_box((4, 5, 6), (2, 0, 0), (1, 9, 9)) is None
