"""The map source (pts == NULL) of lv_elev_build, lv_ndt_build and lv_occ_mark behind a background rebuild (lv_maptools.hpp
"the map source"): a 4096-point map built from the scene of tests/elevation_cases.py loses a box, gains 512 points, starts
lv_map_relinearise_async, loses a second box while that rebuild is in flight and waits for its adoption.  What the three calls
then read must be lv_map_fetch's living points: the elevation map and the NDT target are held to their numpy references with the
helpers and tolerances of tests/test_gpu_elevation.py and tests/test_gpu_ndt.py, the mark's counts to those of the same call
given the fetched points.  The same again after a further lv_map_add with no rebuild pending."""
import numpy as np
import pytest

import elevation_cases as cases
import elevation_ref as er
import ndt_ref as nr
from test_gpu_elevation import _held, _params
from test_gpu_ndt import _check_against_reference, _fetch, _prm, _same_bits

pytestmark = pytest.mark.gpu

NDT_PRM = nr.params(origin=(-7.0, -3.7, -1.0), resolution=1.0, nx=14, ny=8, nz=6, min_points=5, reg=0.01)
OCC_PRM = dict(origin=(-7.0, -3.7, -1.0), resolution=0.2, nx=70, ny=37, nz=26)
BOX_1 = ((-0.5, -3.7, -5.0), (2.1, -0.9, 5.0))   # the slab with the table in it
BOX_2 = ((3.0, 0.0, -5.0), (7.0, 3.7, 5.0))      # a corner of the ramp


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _outside(pts, box):
    return ~np.all((pts >= np.array(box[0], np.float32)) & (pts <= np.array(box[1], np.float32)), axis=1)


def _map_source_is_the_living_points(capi, ctx, ref, what):
    living = ctx.map_fetch()
    assert np.array_equal(_bits(living), _bits(ref)), what
    # the elevation map
    prm = cases.scene_params()
    stats = ctx.elev_build(_params(capi, prm), None)
    _held(capi, ctx, stats, er.build(prm, living), what)
    i = ctx.elev_info()
    assert (i.built, i.from_map, i.n_points) == (1, 1, len(living)), what
    # the NDT target
    p = _prm(capi, NDT_PRM)
    T = nr.build(NDT_PRM, living)
    s_map = ctx.ndt_build(p, None)
    from_map = _fetch(ctx, capi)
    assert ctx.ndt_info().from_map == 1 and s_map.tolist() == nr.stats(T), what
    _check_against_reference(from_map, T)
    s_pts = ctx.ndt_build(p, living)
    assert s_pts.tolist() == s_map.tolist() and _same_bits(_fetch(ctx, capi), from_map), what
    # the mark: a fresh grid each time
    m = capi.default_occ_mark_params(min_points=2)
    ctx.occ_clear()
    st_map = ctx.occ_mark(m, None)
    grid_map = ctx.occ_fetch()
    ctx.occ_clear()
    st_pts = ctx.occ_mark(m, living)
    assert st_map.tolist() == st_pts.tolist() and int(st_map[0]) > len(living) - 10 and int(st_map[2]) > 100, (what, st_map, st_pts)
    assert np.array_equal(_bits(grid_map), _bits(ctx.occ_fetch())), what
    assert np.array_equal(_bits(ctx.map_fetch()), _bits(living)), what   # (read-only)


def test_map_source_behind_a_background_rebuild(capi):
    pts = cases.scene()
    ref, more, last = pts[:4096], pts[4096:4608], pts[4608:4864]
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**OCC_PRM))
        ctx.map_build(ref)
        keep = _outside(ref, BOX_1)
        assert ctx.map_evict_box(*BOX_1, keep_inside=False) == int((~keep).sum()) > 100
        ref = ref[keep]
        ctx.map_add(more)
        ref = np.concatenate([ref, more])
        st0 = ctx.map_rebuild_status()
        ctx.map_relinearise_async()
        assert ctx.map_rebuild_status()["started"] == st0["started"] + 1
        keep = _outside(ref, BOX_2)
        assert ctx.map_evict_box(*BOX_2, keep_inside=False) == int((~keep).sum()) > 100   # (journaled, or on the adopted copy)
        ref = ref[keep]
        s = ctx.map_rebuild_status(wait=True)
        assert s["state"] == 0 and s["adopted"] == st0["adopted"] + 1 and s["journal"] == 0
        _map_source_is_the_living_points(capi, ctx, ref, "adopted")
        ctx.map_add(last)   # no rebuild pending
        assert ctx.map_rebuild_status()["state"] == 0
        _map_source_is_the_living_points(capi, ctx, np.concatenate([ref, last]), "after a further add")
