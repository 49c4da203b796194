"""The scan voxel grid on the device where leaves hold many points, on all three routes (lv_scan.hip: window_small_kernel;
deskew_keys_kernel + window_tail_kernel; the vg_* kernels) — the cases of tests/voxel_cases.py, which
tests/test_voxel_cases_ref.py holds to what they claim.  Every case runs through the entry point it names and must
* report the route it was built for (lv_scan_route: a test meant for one route cannot quietly run another),
* equal oracle.voxelgrid(oracle.deskew(oracle.cloud_ingest(...))) bit for bit (a leaf's centroid is the sequential f32 sum of
  its members in input order, divided by the count), and
* with the route's option off, equal the general chain: the same bits, and an update that consumes the scan identical in x, P,
  passes and n_valid per pass (the Morton and tile order behind the points)."""
import numpy as np
import pytest

import voxel_cases as vc

pytestmark = pytest.mark.gpu

CASES = vc.cases()


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    assert (c.SCAN_ROUTE_NONE, c.SCAN_ROUTE_SMALL, c.SCAN_ROUTE_LARGE, c.SCAN_ROUTE_GENERAL) == (vc.NONE, vc.SMALL, vc.LARGE, vc.GENERAL)
    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _load(ctx, capi, oracle, case):
    """Everything in front of the scan call that does not depend on the options: the LiDAR buffer of a window case."""
    times, states, xt2 = (None, None, None) if case.entry == "downsample" else vc.motion(case, oracle)
    if case.entry == "window":
        kept = ctx.cloud_ingest(vc.window_message(case, times), len(case.xyz), capi.CloudFormat(*vc.format_args()), capi.IngestParams(*vc.INGEST))
        assert kept == len(case.xyz) == ctx.cloud_size()
    return times, states, xt2


def _scan(ctx, case, times, states, xt2):
    if case.entry == "downsample":
        ctx.scan_downsample(case.xyz, case.leaf)
    elif case.entry == "deskew":
        ctx.scan_deskew(case.xyz, times, states, xt2, downsample_prec=case.leaf)
    else:
        assert ctx.scan_deskew_window(vc.WINDOW[0], vc.WINDOW[1], states, xt2, downsample_prec=case.leaf) == len(case.xyz)
    return ctx.scan_route(), ctx.scan_fetch()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_route_and_bits(capi, oracle, lv, case):
    want = vc.expected(case)
    with capi.Context() as ctx:
        assert ctx.scan_route() == capi.SCAN_ROUTE_NONE
        for name, value in case.options:
            ctx.set_option(name, value)
        route, got = _scan(ctx, case, *_load(ctx, capi, oracle, case))
    assert route == case.route, (route, case.route)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    print(f"{case.name}: {len(case.xyz)} in, {len(want)} out, route {route}, {len(diff)} centroids differ")
    assert len(diff) == 0, (diff[:8], got[diff[:4]], want[diff[:4]])


def _map_around(points):
    """A map in which every scan point finds a plane: five coplanar points around each (its plane's normal along x, y or z in
    turn).  Points far outside the test volume (the one that makes a route decline) get none."""
    p = points[np.abs(points).max(axis=1) < 1000.0].astype(np.float64)
    off = np.array([[0, 0, 0], [0.1, 0.1, 0], [0.1, -0.1, 0], [-0.1, 0.1, 0], [-0.1, -0.1, 0]], np.float64)
    patches = np.stack([np.roll(off, k, axis=1) for k in range(3)])        # [3,5,3]
    return (p[:, None, :] + patches[np.arange(len(p)) % 3]).reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("case", [c for c in CASES if not c.options and (c.route != vc.GENERAL or c.entry == "window" or "declines" in c.name)],
                         ids=lambda c: c.name)
def test_route_option_off_is_the_general_chain(capi, oracle, lv, case):
    """On and off: the case's route, then the general chain.  Both options go off together: with small_window alone off, a
    small window from the LiDAR buffer takes the large route (the "/large" cases).  A case that declines runs the general
    chain in both arms."""
    from limo_velo_amd import synth

    want = vc.expected(case)
    x0 = synth.make_state((0.05, -0.03, 0.02), synth.quat_from_rotvec((0.001, -0.0008, 0.0012)))
    P0 = synth.default_P0()
    res = {}
    with capi.Context() as ctx:
        if len(want):
            ctx.map_build(_map_around(want))
        loaded = _load(ctx, capi, oracle, case)
        for on in (1, 0):
            ctx.set_option("small_window", on)
            ctx.set_option("large_window", on)
            route, got = _scan(ctx, case, *loaded)
            upd = None
            if len(want):
                x, P, passes, tr, sums = ctx.update(x0, P0)
                upd = (x, P, passes, [s["n_valid"] for s in sums])
            res[on] = (route, got, upd)
    assert res[1][0] == case.route and res[0][0] == vc.GENERAL, (res[1][0], res[0][0])
    assert res[1][1].shape == res[0][1].shape == want.shape
    assert np.array_equal(_bits(res[1][1]), _bits(res[0][1])) and np.array_equal(_bits(res[1][1]), _bits(want))
    if len(want):
        a, b = res[1][2], res[0][2]
        print(f"{case.name}: passes {a[2]}, n_valid per pass {a[3]}")
        assert a[2] == b[2] and a[3] == b[3]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert max(a[3]) >= 1                             # the update really consumed the scan: points found their planes
