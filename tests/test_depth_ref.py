"""CPU checks of the depth fusion's reference (tests/depth_ref.py) and of the scene the GPU test runs (tests/depth_cases.py): every
class of the rule is met by the cases as committed, so a later edit of the scene cannot hollow tests/test_gpu_depth.py out; and the
reference's own invariances: the order of the views, and their split over two calls below max_weight."""
import numpy as np
import pytest

import depth_cases as dc
import depth_ref as dr

MAX_WEIGHT = 10000


def _empty():
    return np.zeros((dc.NZ, dc.NY, dc.NX), np.int32), np.zeros((dc.NZ, dc.NY, dc.NX), np.int32)


def _run(frames, prm, S=None, W=None, max_weight=MAX_WEIGHT):
    if S is None:
        S, W = _empty()
    return dr.integrate(S, W, dc.ORIGIN, dc.RES, dc.TRUNC_CELLS, max_weight, frames, prm)


@pytest.mark.parametrize("carve", [0, 1])
def test_the_scene_reaches_every_class(carve):
    r = _run([dc.frame()], dc.params(carve=carve))
    v = r["views"][0]
    n = {k: int(v[k].sum()) for k in ("ok", "valid", "far", "behind", "band", "adds")}
    n["unprojected"] = int((~v["ok"]).sum())
    n["invalid"] = int((v["ok"] & ~v["valid"]).sum())
    n["negative"] = int((v["band"] & (v["q"] < 0)).sum())
    n["positive"] = int((v["band"] & (v["q"] > 0)).sum())
    print(carve, n, r["stats"])
    assert all(n[k] > 0 for k in n), n
    assert n["ok"] == n["valid"] + n["invalid"] and n["valid"] == n["far"] + n["behind"] + n["band"]
    assert n["adds"] == n["band"] + (n["far"] if carve else 0)
    assert list(r["stats"]) == [n["ok"], n["valid"], n["adds"], n["adds"]]   # (one view: a voxel adds at most once)
    T = dc.TRUNC_CELLS * 256
    assert np.array_equal(r["W"], v["adds"].astype(np.int32)) and np.array_equal(r["S"], v["s"].astype(np.int32))
    assert r["S"].min() >= -T and r["S"].max() == (T if carve else r["S"][v["band"]].max()) and np.all(np.abs(r["S"]) <= T * r["W"])
    # the band's ends themselves: q = -T and q = T contribute, the values next to them do not (or carve)
    assert v["q"][v["band"]].min() >= -T and v["q"][v["band"]].max() <= T and v["q"][v["behind"]].max() < -T and v["q"][v["far"]].min() > T


def test_the_variants_differ_where_they_should():
    base = _run([dc.frame()], dc.params())
    pad = _run([dc.frame_padded()], dc.params())
    assert np.array_equal(base["S"], pad["S"]) and np.array_equal(base["W"], pad["W"]) and np.array_equal(base["stats"], pad["stats"])
    f32 = _run([dc.frame_f32()], dc.params())
    assert f32["stats"][0] == base["stats"][0] and 0 < f32["stats"][1] < base["stats"][1]   # (more pixels without a measurement)
    m = dc.frame_f32()["depth"]
    assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any() and (m == 0).any() and (m < 0).any()
    dist = _run([dc.frame_distorted()], dc.params())
    assert dist["stats"][0] != base["stats"][0] and not np.array_equal(dist["S"], base["S"])
    assert _run([dc.frame_pixel()], dc.params())["stats"][3] > 0
    corner = _run([dc.frame_corner()], dc.params(max_depth=1.2))
    k, j, i = np.nonzero(corner["W"])
    assert len(k) > 50 and i.min() > dc.NX // 2 and j.min() > dc.NY // 2 and k.min() > dc.NZ // 2
    nothing = _run([dc.frame_nothing()], dc.params())
    assert not nothing["stats"].any() and not nothing["W"].any()
    many = _run(dc.frames32(), dc.params())
    assert len(many["views"]) == 32 and many["W"].max() > 16


def test_view_order_and_split_below_max_weight():
    fr = dc.frames3()
    prm = dc.params(carve=1)
    one = _run(fr, prm)
    back = _run(fr[::-1], prm)
    assert np.array_equal(one["S"], back["S"]) and np.array_equal(one["W"], back["W"]) and np.array_equal(one["stats"], back["stats"])
    S, W = _empty()
    pairs = valid = adds = 0
    for f in fr:
        r = _run([f], prm, S, W)
        S, W = r["S"], r["W"]
        pairs, valid, adds = pairs + int(r["stats"][0]), valid + int(r["stats"][1]), adds + int(r["stats"][2])
    assert np.array_equal(S, one["S"]) and np.array_equal(W, one["W"]) and one["W"].max() == 3
    assert [pairs, valid, adds] == [int(x) for x in one["stats"][:3]]


def test_the_split_matters_at_max_weight():
    """max_weight = 2, a call of three views and a call of one: both folds rescale, and one call of four views rescales otherwise."""
    fr = dc.frames3() + [dc.frame()]
    prm = dc.params()
    a = _run(fr[:3], prm, max_weight=2)
    b = _run(fr[3:], prm, a["S"], a["W"], max_weight=2)
    whole = _run(fr, prm, max_weight=2)
    assert b["W"].max() == 2 and whole["W"].max() == 2 and np.array_equal(b["W"], whole["W"])
    assert not np.array_equal(b["S"], whole["S"])
    assert (dr.fold(np.array([700]), np.array([3]), np.array([-5]), np.array([1]), 3)[0] == [(695 * 3) // 4]).all()
    assert (dr.fold(np.array([-700]), np.array([3]), np.array([-5]), np.array([1]), 3)[0] == [-529]).all()   # floor, not truncation
