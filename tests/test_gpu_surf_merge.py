"""GPU tests of lv_surf_merge (lv_surf_merge.hip; include/limovelo_hip.h "Submap merging") against the numpy statement of the rule
in tests/surf_merge_ref.py, by EQUALITY on S, W and all four stats: one f64 step, integers after it, so there is no tolerance and
no undecided share.  The cases are tests/surf_merge_cases.py's (tests/test_surf_merge_ref.py holds that each exercises what it
claims): destination 24 x 20 x 12, submaps around 16 x 12 x 10."""
import numpy as np
import pytest

import surf_merge_cases as mc
import surf_merge_ref as mr

pytestmark = pytest.mark.gpu

CASES = mc.cases()
LV_EINVAL, LV_ESTATE = -1, -4


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def mesh(lv):
    from limo_velo_amd import mesh as m

    return m


def _open(capi, dest):
    """a context whose volume is the destination, loaded"""
    nz, ny, nx = dest["S"].shape
    ctx = capi.Context()
    ctx.tsdf_configure(capi.default_tsdf_params(origin=[float(v) for v in dest["origin"]], resolution=float(dest["resolution"]), nx=nx, ny=ny, nz=nz,
                                                trunc_cells=dest["trunc_cells"], max_weight=dest["max_weight"]))
    if dest["W"].any():
        ctx.tsdf_load(dest["S"], dest["W"])
    return ctx


def _merge(mesh, ctx, dest, sub, pose, what, min_weight=1, interp=mr.TRILINEAR):
    """One lv_surf_merge on ctx, whose volume holds dest, held to the reference of that call; returns the destination after."""
    st = mesh.merge(ctx, sub, pose, min_weight=min_weight, nearest=interp == mr.NEAREST)
    got = ctx.tsdf_fetch()
    want = mr.merge(dest, sub, pose, min_weight, interp)
    diff = int(((got["S"] != want["S"]) | (got["W"] != want["W"])).sum())
    print(f"{what}: stats {st} (reference {want['stats']}), {diff} voxels differ")
    assert np.array_equal(st, want["stats"]), (what, st, want["stats"])
    assert diff == 0, what
    return mr.merged(dest, want)


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_reference(capi, mesh, name):
    """the identity, a whole-voxel shift, a skew rotation with an off-lattice translation (both interpolations), resolution ratios
    0.5, 1.25 and 2, a wider and a narrower source band, min_weight above some source weights, a pre-filled destination that folds at
    max_weight, a submap that grazes the volume and one that misses it"""
    c = CASES[name]
    with _open(capi, c["dest"]) as ctx:
        after = _merge(mesh, ctx, c["dest"], c["sub"], c["pose"], name, c["min_weight"], c["interp"])
        if name == "misses":
            assert np.array_equal(after["S"], c["dest"]["S"]) and np.array_equal(after["W"], c["dest"]["W"])
        # once more on top of itself: a destination that is not empty
        _merge(mesh, ctx, after, c["sub"], c["pose"], name + " again", c["min_weight"], c["interp"])


def test_recentred_destination(capi, mesh):
    """the centres are those of the volume's present origin, after its shifts"""
    c = CASES["skew"]
    with _open(capi, c["dest"]) as ctx:
        first = _merge(mesh, ctx, c["dest"], c["sub"], c["pose"], "before the shift")
        shift = (3, -2, 1)
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, shift)
        p = ctx.tsdf_params()
        moved = ctx.tsdf_fetch()
        dest = dict(first, origin=np.array([float(v) for v in p.origin], np.float32), S=moved["S"], W=moved["W"])
        assert not np.array_equal(dest["origin"], c["dest"]["origin"]) and dest["W"].any()
        _merge(mesh, ctx, dest, c["sub"], c["pose"], "after the shift")


def test_two_submaps_in_both_orders(capi, mesh):
    d, subs = mc.pair()
    out = []
    for order in ((0, 1), (1, 0)):
        with _open(capi, d) as ctx:
            dest = d
            for k in order:
                dest = _merge(mesh, ctx, dest, *subs[k], f"order {order}, submap {k}")
            out.append(ctx.tsdf_fetch())
    assert np.array_equal(out[0]["S"], out[1]["S"]) and np.array_equal(out[0]["W"], out[1]["W"]) and out[0]["W"].max() < d["max_weight"]


def test_mesh_goes_stale_and_the_rays_see_the_merged_surface(capi, mesh):
    c = CASES["skew"]
    d = c["dest"]
    # rays down the z axis through the middle of the volume
    o, r = d["origin"].astype(float), float(d["resolution"])
    xs, ys = np.meshgrid(o[0] + r * np.arange(6, 18, 1.5), o[1] + r * np.arange(5, 15, 1.5))
    frm = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, o[2] + r * 11.5)], 1)
    to = frm - [0, 0, r * 11]
    with _open(capi, d) as ctx:
        assert ctx.tsdf_mesh_build()[0] == 0
        before, _, _ = ctx.tsdf_raycast(frm, to)   # (packs the states of the empty volume)
        assert not (before["status"] == capi.LV_SURF_HIT).any() and ctx.tsdf_mesh_info().stale == 0
        after = _merge(mesh, ctx, d, c["sub"], c["pose"], "under a built mesh")
        info = ctx.tsdf_mesh_info()
        assert info.built == 1 and info.stale == 1
        seen, _, _ = ctx.tsdf_raycast(frm, to)
        assert (seen["status"] == capi.LV_SURF_HIT).any()
        assert ctx.tsdf_mesh_build()[0] > 0 and ctx.tsdf_mesh_info().stale == 0
    with _open(capi, after) as ctx:   # the same volume, loaded: the same rays
        want, _, _ = ctx.tsdf_raycast(frm, to)
    assert np.array_equal(seen, want)


def test_submaps_fuse_equals_the_reference_loop(capi, mesh):
    d, subs = mc.pair()
    keep = mesh.Submaps()
    for s, p in subs:
        keep.add(s, p)
    moved = [(p[0] + [0.05, -0.02, 0.01], p[1]) for _, p in subs]   # what a pose graph hands back
    filled = dict(d, S=np.full_like(d["S"], 17), W=np.full_like(d["W"], 2))   # fuse clears it first
    with _open(capi, filled) as ctx:
        for poses in (None, moved):
            st = keep.fuse(ctx, poses=poses)
            want, wst = mr.fuse(d, [s for s, _ in subs], [p for _, p in subs] if poses is None else moved)
            got = ctx.tsdf_fetch()
            assert np.array_equal(st, wst) and st[1] > 500
            assert np.array_equal(got["S"], want["S"]) and np.array_equal(got["W"], want["W"])
        live = mesh.submap(ctx)   # the live volume as a submap, merged into a second context at the identity
    assert np.array_equal(live["S"], want["S"]) and live["trunc_cells"] == d["trunc_cells"]
    with _open(capi, d) as ctx:
        _merge(mesh, ctx, d, live, mr.IDENTITY, "the fused volume into a copy of its grid")


def test_states_and_the_resolution_ratio(capi, mesh):
    c = CASES["identity"]
    with capi.Context() as ctx:
        with pytest.raises(capi.LvError, match="no TSDF volume: call lv_tsdf_configure first") as e:
            mesh.merge(ctx, c["sub"], c["pose"])
        assert f"error {LV_ESTATE}" in str(e.value)
        with pytest.raises(capi.LvError, match="lv_surf_merge: min_weight = 0: at least 1"):   # (the arguments come first)
            mesh.merge(ctx, c["sub"], c["pose"], min_weight=0)
    with _open(capi, mc.destination(resolution=4.0)) as ctx:
        with pytest.raises(capi.LvError, match="a ratio of 1/8 to 8") as e:
            mesh.merge(ctx, c["sub"], c["pose"])
        assert f"error {LV_EINVAL}" in str(e.value) and not ctx.tsdf_fetch()["W"].any()
