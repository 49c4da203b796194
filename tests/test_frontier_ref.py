"""tests/frontier_ref.py, the numpy statement of the frontier rule (include/limovelo_hip.h "Frontiers"), against hand-worked cases
and against a plain Python flood fill in place of scipy.ndimage.label."""
import numpy as np
import pytest

import frontier_ref as fr
import occupancy_ref as ocr

F = np.float32


def _room(prm, shape, box, value):
    """Unknown space [nz, ny, nx] with `value` inside box = (k0, k1, j0, j1, i0, i1), ends exclusive."""
    L = np.full(shape, np.nan, F)
    k0, k1, j0, j1, i0, i1 = box
    L[k0:k1, j0:j1, i0:i1] = value
    return L


@pytest.mark.parametrize("conn", [4, 8])
def test_a_free_room_in_unknown_space_has_a_ring(conn):
    prm = ocr.params(nx=9, ny=8, nz=1)
    L = _room(prm, (1, 8, 9), (0, 1, 2, 7, 1, 6), prm["l_min"])   # 5 x 5 cells: i 1..5, j 2..6
    labels, cl, stats = fr.build(prm, L, fr.fparams(planar=1, connectivity=conn))
    ring = np.zeros((8, 9), bool)
    ring[2:7, 1:6] = True
    ring[3:6, 2:5] = False
    assert np.array_equal(labels >= 0, ring) and np.all(labels[ring] == 0)
    assert list(stats) == [25, 72 - 25, 16, 1] and len(cl) == 1
    c = cl[0]
    assert (c["size"], c["first"]) == (16, 2 * 9 + 1)
    assert list(c["sum"]) == [16 * 3, 16 * 4, 0] and list(c["centre"]) == [3, 4, 0]   # the centre is the room's, not a member
    assert list(c["lo"]) == [1, 2, 0] and list(c["hi"]) == [5, 6, 0]
    # rep: the members nearest (3, 4) are at squared distance 4: (3, 2), (1, 4), (5, 4), (3, 6); the smallest index wins
    assert c["rep"] == 2 * 9 + 3


def test_the_border_is_not_unknown():
    prm = ocr.params(nx=5, ny=5, nz=1)
    L = np.full((1, 5, 5), prm["l_min"], F)   # all free, up to the border
    labels, cl, stats = fr.build(prm, L, fr.fparams(planar=1, connectivity=8))
    assert np.all(labels == -1) and len(cl) == 0 and list(stats) == [25, 0, 0, 0]


def test_a_room_with_one_occupied_wall():
    prm = ocr.params(nx=9, ny=8, nz=1)
    L = _room(prm, (1, 8, 9), (0, 1, 2, 7, 1, 6), prm["l_min"])
    L[0, 2:7, 0] = prm["l_max"]   # the wall at i = 0 shields the room's i = 1 side
    labels, cl, stats = fr.build(prm, L, fr.fparams(planar=1, connectivity=4))
    want = np.zeros((8, 9), bool)
    want[2, 1:6] = want[6, 1:6] = want[2:7, 5] = True   # a U: the side along the wall has no unknown neighbour but at its ends
    assert np.array_equal(labels >= 0, want) and len(cl) == 1 and cl[0]["size"] == 13
    assert list(stats) == [25, 72 - 25 - 5, 13, 1]
    # 3-D: the same room one layer thick in a 3-layer grid has unknown above and below: every free cell is a frontier cell
    prm3 = ocr.params(nx=9, ny=8, nz=3)
    L3 = np.full((3, 8, 9), np.nan, F)
    L3[1] = L[0]
    labels3, cl3, stats3 = fr.build(prm3, L3, fr.fparams(connectivity=6))
    assert np.array_equal(labels3[1] >= 0, L3[1] == F(prm["l_min"])) and np.all(labels3[[0, 2]] == -1) and cl3[0]["size"] == 25


def test_the_thresholds_themselves():
    prm = ocr.params(nx=4, ny=1, nz=1)
    between = F(0.5) * (F(prm["l_free"]) + F(prm["l_occ"]))
    L = np.array([[[prm["l_free"], np.nan, prm["l_occ"], between]]], F)
    assert list(fr.states(prm, L, fr.fparams())[0, 0]) == [fr.FREE, fr.UNKNOWN, fr.OCCUPIED, fr.OTHER]
    L2 = np.array([[[between, np.nan, np.nextafter(F(prm["l_free"]), F(0)), np.nan]]], F)
    assert list(fr.states(prm, L2, fr.fparams())[0, 0]) == [fr.OTHER, fr.UNKNOWN, fr.OTHER, fr.UNKNOWN]
    labels, _, stats = fr.build(prm, L, fr.fparams(connectivity=6))
    assert list(labels.reshape(-1)) == [0, -1, -1, -1] and list(stats) == [1, 1, 1, 1]   # l_occ beside unknown is no frontier
    # planar: a value between the thresholds projects to unknown (-1)
    assert list(fr.states(prm, L, fr.fparams(planar=1, connectivity=4))[0, 0]) == [fr.FREE, fr.UNKNOWN, fr.OCCUPIED, fr.UNKNOWN]


def test_numbering_ties_and_min_size():
    prm = ocr.params(nx=12, ny=1, nz=1)
    L = np.full((1, 1, 12), np.nan, F)
    L[0, 0, [1, 2, 5, 6, 9]] = prm["l_min"]   # components {1, 2}, {5, 6}, {9}
    labels, cl, stats = fr.build(prm, L, fr.fparams(planar=1, connectivity=4))
    assert list(labels[0]) == [-1, 0, 0, -1, -1, 1, 1, -1, -1, 2, -1, -1] and list(cl["first"]) == [1, 5, 9] and list(cl["size"]) == [2, 2, 1]
    assert list(cl["centre"][:, 0]) == [2, 6, 9] and list(cl["rep"]) == [2, 6, 9]   # 1.5 rounds half up to 2
    labels, cl, stats = fr.build(prm, L, fr.fparams(planar=1, connectivity=4, min_size=2))
    assert list(labels[0]) == [-1, 0, 0, -1, -1, 1, 1, -1, -1, -1, -1, -1] and list(stats) == [5, 7, 5, 2]


@pytest.mark.parametrize("shape,planar,conns", [((4, 9, 11), 0, (6, 18, 26)), ((3, 13, 17), 1, (4, 8)), ((1, 1, 1), 0, (6,)), ((1, 7, 1), 1, (4,))])
def test_scipy_components_equal_a_flood_fill(shape, planar, conns):
    nz, ny, nx = shape
    prm = ocr.params(nx=nx, ny=ny, nz=nz)
    rng = np.random.default_rng(nx + ny)
    L = fr.random_logodds(rng, shape, prm)
    for conn in conns:
        fp = fr.fparams(planar=planar, k_lo=0, k_hi=nz - 1, connectivity=conn)
        mask = fr.frontier_mask(fr.states(prm, L, fp))
        a = fr.canonical(*fr.components(mask, conn), 1)
        b = fr.canonical(*fr.flood_fill(mask, conn), 1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # the frontier predicate cell by cell
        st = fr.states(prm, L, fp)
        for k, j, i in np.ndindex(st.shape):
            nb = [(k, j, i - 1), (k, j, i + 1), (k, j - 1, i), (k, j + 1, i)] + ([] if planar else [(k - 1, j, i), (k + 1, j, i)])
            want = st[k, j, i] == fr.FREE and any(all(0 <= v[a] < st.shape[a] for a in range(3)) and st[v] == fr.UNKNOWN for v in nb)
            assert mask[k, j, i] == want


def test_rank_by_hand():
    labels = np.full((1, 9), -1, np.int32)
    labels[0, [1, 2]] = 0
    labels[0, 7] = 1
    P = np.array([[50, fr.UNREACHED, fr.UNREACHED, 30, 30, 10, fr.UNREACHED, fr.UNREACHED, fr.UNREACHED]], np.uint32)
    p, c = fr.rank(labels, 2, P, 0)
    assert list(p) == [fr.UNREACHED] * 2 and list(c) == [-1, -1]
    p, c = fr.rank(labels, 2, P, 1)
    assert list(p) == [30, fr.UNREACHED] and list(c) == [3, -1]   # (cell 0 is in reach too, but dearer)
    p, c = fr.rank(labels, 2, P, 2)
    assert list(p) == [30, 10] and list(c) == [3, 5]   # ties to the smaller cell


def test_the_serpentine_is_one_component():
    prm = ocr.params(nx=7, ny=9, nz=2)
    L = fr.serpentine(prm, 7, 9, 2)
    for fp in (fr.fparams(connectivity=6), fr.fparams(planar=1, k_lo=0, k_hi=1, connectivity=4)):
        labels, cl, stats = fr.build(prm, L, fp)
        assert len(cl) == 1 and cl[0]["size"] == stats[0] == stats[2] == 4 * 5 + 3
