"""tests/colour_ref.py, the numpy statement of the colour layer's rule, held to hand-made cases; and the condition the GPU tests
put on their scene (tests/colour_cases.py): the reference alone leaves fewer than 1 % of the possible decisions undecided."""
import numpy as np
import pytest

import colour_cases as cc
import colour_ref as cr
import tsdf_cases as tc
import tsdf_ref as tr


def test_candidates_by_hand():
    S = np.array([[[0, 256, -256, 257, -513, 512, 0, 100]]])
    W = np.array([[[1, 1, 1, 1, 2, 2, 0, 1]]])
    assert cr.candidates(S, W, 1, 256).ravel().tolist() == [True, True, True, False, False, True, False, True]
    assert cr.candidates(S, W, 2, 256).ravel().tolist() == [False, False, False, False, False, True, False, False]
    assert cr.candidates(S, W, 1, 1).ravel().tolist() == [True, False, False, False, False, False, False, False]


def test_centres_by_hand():
    c = cr.centres((-6.4, 1.0, 0.0), 0.2, (4, 3, 5), [0, 1, 5, 15, 59])
    assert c.dtype == np.float32
    f = np.float32
    want = [[f(-6.4) + f(0.2) * f(0.5), f(1.0) + f(0.2) * f(0.5), f(0.2) * f(0.5)],
            [f(-6.4) + f(0.2) * f(1.5), f(1.0) + f(0.2) * f(0.5), f(0.2) * f(0.5)],
            [f(-6.4) + f(0.2) * f(0.5), f(1.0) + f(0.2) * f(1.5), f(0.2) * f(0.5)],
            [f(-6.4) + f(0.2) * f(0.5), f(1.0) + f(0.2) * f(0.5), f(0.2) * f(1.5)],
            [f(-6.4) + f(0.2) * f(4.5), f(1.0) + f(0.2) * f(2.5), f(0.2) * f(3.5)]]
    assert np.array_equal(c, np.array(want, f))


def test_fold_and_colours_by_hand():
    assert cr.quantise([0.0, 0.49, 0.5, 254.5, 255.0]).tolist() == [0, 0, 1, 255, 255]
    e = np.array([[0, 0, 0, 0], [100, 200, 30, 2], [100, 200, 30, 2], [255 * 3, 0, 9, 3], [7, 7, 7, 1]], np.uint32)
    n = np.array([2, 1, 2, 3, 0])
    dC = np.array([[20, 41, 510], [50, 0, 255], [50, 0, 255], [255 * 3, 3, 0], [99, 99, 99]])
    out = cr.fold(e, n, dC, 3)
    assert out.tolist() == [[20, 41, 510, 2],                     # below the cap
                            [150, 200, 285, 3],                   # Wn == max_weight: no rescale
                            [150 * 3 // 4, 200 * 3 // 4, 285 * 3 // 4, 3],   # Wn = 4 > 3
                            [255 * 6 * 3 // 6, 3 * 3 // 6, 9 * 3 // 6, 3],  # C = 255 * Wc stays at 255 * max_weight
                            [7, 7, 7, 1]]                         # n = 0: untouched
    assert np.all(out[:, :3] <= 255 * out[:, 3:4])
    assert cr.voxel_colour(np.array([[0, 0, 0, 0], [3, 4, 5, 2], [765, 0, 1, 3], [1, 2, 3, 6]])).tolist() == \
        [[0, 0, 0, 0], [2, 2, 3, 255], [255, 0, 0, 255], [0, 0, 1, 255]]   # halves round up
    corners = np.zeros((3, 8, 4), np.uint32)
    corners[1, 2] = [10, 20, 30, 1]
    corners[2, 0], corners[2, 5], corners[2, 7] = [10, 20, 30, 1], [11, 20, 33, 1], [0, 0, 510, 2]
    assert cr.vertex_colour(corners).tolist() == [[0, 0, 0, 0], [10, 20, 30, 255], [7, 13, 106, 255]]   # (21 / 3, 40 / 3 -> 13, 318 / 3)


def test_shift_by_hand():
    a = np.arange(2 * 3 * 4).reshape(2, 3, 4) + 1
    s = cr.shift_layer(a, (1, 0, 0))
    assert np.array_equal(s[:, :, :3], a[:, :, 1:]) and not s[:, :, 3].any()
    s = cr.shift_layer(a, (0, -1, 1))
    assert np.array_equal(s[0, 1:], a[1, :2]) and not s[1].any() and not s[0, 0].any()
    assert not cr.shift_layer(a, (4, 0, 0)).any() and np.array_equal(cr.shift_layer(a, (0, 0, 0)), a)
    layer = np.stack([a] * 4, axis=-1)
    assert np.array_equal(cr.shift_layer(layer, (-2, 1, 0))[..., 2], cr.shift_layer(a, (-2, 1, 0)))


def test_one_voxel_seen_and_one_behind_it():
    """Two candidate voxels on the optical axis, 0.6 m apart: the near one takes the image's colour, the far one is occluded
    with a margin of 0.25 m and seen with one of 1 m."""
    S = np.zeros((1, 1, 8), np.int32)
    W = np.zeros((1, 1, 8), np.int32)
    W[0, 0, 2] = W[0, 0, 5] = 1
    img = np.full((9, 9, 3), (10, 20, 30), np.uint8)
    R = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)   # z forward = world x
    frame = dict(R=R, t=np.array([-1.0, 0.1, 0.1], np.float32), fx=10.0, fy=10.0, cx=4.0, cy=4.0, image=img)
    p = cc.colour_params(zbuf_scale=4, window=1, min_weight=1, margin_abs=0.25)
    out = cr.integrate(S, W, None, (0.0, 0.0, 0.0), 0.2, [frame, frame], p)
    assert out["flat"].tolist() == [2, 5] and out["decided"].all() and out["lo"].tolist() == [2, 0]
    assert out["after"][0, 0, 2].tolist() == [20, 40, 60, 2] and not out["after"][0, 0, 5].any()
    assert out["stats_lo"].tolist() == [2, 4, 2, 1] == out["stats_hi"].tolist()
    p.view.margin_abs = 1.0
    out = cr.integrate(S, W, out["after"], (0.0, 0.0, 0.0), 0.2, [frame], p)
    assert out["after"][0, 0, 2].tolist() == [30, 60, 90, 3] and out["after"][0, 0, 5].tolist() == [10, 20, 30, 1]


def test_active_cells_are_the_mesh_rule_s():
    case = tc.sphere_case(**tc.SPHERE_SMALL)
    ref = tc.reference(case)
    act = cr.active_cells(ref["S"], ref["W"], 1)
    assert int(act.sum()) == int(ref["mesh"]["counts"][0]) > 100
    layer = np.zeros(ref["S"].shape + (4,), np.uint32)
    layer[..., :] = [40, 50, 60, 1]
    rgba = cr.mesh_colours(ref["S"], ref["W"], layer, 1)
    assert len(rgba) == act.sum() and np.all(rgba == [40, 50, 60, 255])


@pytest.mark.parametrize("scale,window,width,height,focal", cc.SETTINGS)
def test_the_scene_leaves_the_reference_decided(scale, window, width, height, focal):
    S, W = cc.volume()
    assert (W == 0).mean() > 0.02 and (W == 1).mean() > 0.05 and np.all(np.abs(S) <= cc.T * W)
    out = cr.integrate(S, W, None, cc.ORIGIN, cc.RES, cc.frames(width, height, focal), cc.colour_params(scale, window))
    print(f"{scale} x {window}: {out['possible']} possible decisions, {out['undecided']} undecided")
    assert out["undecided"] < 0.01 * out["possible"] and out["possible"] > 3000
    assert (out["after"][..., 3] > 0).sum() > 1000 and out["hi"].max() == 3
