"""The growth paths of the map tools' buffers (limo-velo_amd/csrc/lv_buffers.hpp; DESIGN.md "Host-side buffers"): every tool is
called three times in ONE context — small, larger than the first call left room for, small again — and each result must equal,
bit for bit, the same call made in a fresh context.  A capacity gone stale after a regrowth, or a buffer that kept an earlier
call's contents, shows as a difference.  Then the occupancy grid is configured again with a smaller grid and the field, the plan
and the three queries are held to a fresh context in the same way.

Tiny inputs: maps of a few hundred points, a 16 x 16 x 4 grid then 8 x 8 x 4, views of a dozen returns.  The map queries stage
2, 400, 2 points: 1200 floats pass the 1024-float floor their buffers double from."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
SMALL, LARGE = "small", "large"
TABLE = np.array([254, 120, 60, 50], np.uint8)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def data(capi):
    """Everything the calls take, by size, made once."""
    from limo_velo_amd import synth

    rng = np.random.default_rng(11)
    sc = synth.make_scene(400, 64)
    big = np.ascontiguousarray(sc["map_xyz"], F)
    maps = {SMALL: np.ascontiguousarray(big[::3]), LARGE: big}
    lo, hi = big.min(0), big.max(0)
    queries = {SMALL: rng.uniform(lo, hi, (2, 3)).astype(F), LARGE: rng.uniform(lo - 1, hi + 1, (400, 3)).astype(F)}
    centre = (0.5 * (lo + hi)).astype(F)
    eye = np.eye(3, dtype=F)

    def returns(n):   # a sensor at the map's centre looking at n of its points (sensor frame = world frame - centre)
        return np.ascontiguousarray(big[rng.choice(len(big), n, replace=False)] - centre)

    views = {SMALL: [(eye, centre, returns(12))], LARGE: [(eye, centre, returns(60)), (eye, centre + F(0.25), returns(30))]}

    def camera(w, h, seed):
        img = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
        return dict(R=eye, t=centre, fx=0.5 * w, fy=0.5 * w, cx=0.5 * w, cy=0.5 * h, image=img, dist=np.zeros(5, F))

    cams = {SMALL: [camera(8, 6, 1)], LARGE: [camera(24, 18, 2), camera(16, 12, 3)]}
    xs = np.array([sc["x_init"], sc["x_true"], sc["x_init"]])
    xs[2, :2] += 0.2
    states = {SMALL: xs[:1], LARGE: xs}
    # occupancy: a 4 m cube round the origin in 0.25 m voxels (16 x 16 x 4), then 8 x 8 x 4 of 0.5 m
    grids = {LARGE: dict(origin=(-2.0, -2.0, -0.5), resolution=0.25, nx=16, ny=16, nz=4, min_range=0.1, max_range=6.0),
             SMALL: dict(origin=(-2.0, -2.0, -0.5), resolution=0.5, nx=8, ny=8, nz=4, min_range=0.1, max_range=6.0)}
    origin = np.array([0.1, -0.2, 0.3], F)

    def sweep(n, seed):
        r = np.random.default_rng(seed)
        return (r.uniform(-1, 1, (n, 3)) * [2.5, 2.5, 0.6]).astype(F)

    sweeps = {SMALL: [(eye, origin, sweep(12, 5))], LARGE: [(eye, origin, sweep(48, 6)), (eye, -origin, sweep(20, 7))]}
    probes = {SMALL: sweep(2, 8), LARGE: np.concatenate([sweep(50, 9), [[np.nan, 0, 0], [99, 0, 0]]]).astype(F)}
    goals = {SMALL: np.array([[1.1, 1.1, 0.1]], F), LARGE: sweep(20, 10)}
    centres = {SMALL: np.array([centre], np.float64), LARGE: rng.uniform(lo, hi, (40, 3))}
    return dict(sc=sc, maps=maps, queries=queries, views=views, cams=cams, states=states, grids=grids, sweeps=sweeps, probes=probes,
                goals=goals, centres=centres)


def _flat(out):
    """The arrays of a result, whatever its nesting, in order."""
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in _flat(out[k])]
    if isinstance(out, (list, tuple)):
        return [a for v in out for a in _flat(v)]
    return [] if out is None else [np.ascontiguousarray(out)]


def _same_bits(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb) and len(fa) > 0
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and x.dtype == y.dtype, (i, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (i, x, y)


def _occ_ready(capi, ctx, d, size=LARGE):
    """A configured grid with one integrated sweep, its field and its plan."""
    ctx.occ_configure(capi.default_occupancy_params(**d["grids"][size]))
    ctx.occ_integrate(d["sweeps"][LARGE])
    ctx.occ_distance_build()
    ctx.occ_plan_build(d["goals"][SMALL], TABLE, capi.default_plan_params(connectivity=26, min_clear_s2=1))


# per tool: prepare(capi, ctx, data) once per context, call(capi, ctx, data, size) -> result
def _prep_map(capi, ctx, d):
    ctx.map_build(d["maps"][LARGE])


def _prep_scan(capi, ctx, d):
    ctx.map_build(d["maps"][LARGE])
    ctx.scan_set(d["sc"]["scan_xyz"])


def _none(capi, ctx, d):
    pass


def _on_map(fn):
    """A tool whose buffers follow the map: the map itself is built small, large, small."""
    def call(capi, ctx, d, size):
        ctx.map_build(d["maps"][size])
        return fn(capi, ctx, d, size)

    return call


def _place(capi, ctx, d, size):
    first = ctx.place_add_map(d["centres"][size])
    desc, cen = ctx.place_fetch()
    return desc[first:], cen[first:]


def _integrate(capi, ctx, d, size):
    ctx.occ_clear()
    return ctx.occ_integrate(d["sweeps"][size]), ctx.occ_fetch()


def _plan_build(capi, ctx, d, size):
    st = ctx.occ_plan_build(d["goals"][size], TABLE, capi.default_plan_params(connectivity=26, min_clear_s2=1))
    return st, ctx.occ_plan_fetch()


TOOLS = {
    "query_knn": (_prep_map, lambda capi, ctx, d, s: ctx.map_knn(d["queries"][s], 5)),
    "query_radius": (_prep_map, lambda capi, ctx, d, s: ctx.map_radius(d["queries"][s], 1.5)),
    "update_batch": (_prep_scan, lambda capi, ctx, d, s: ctx.update_batch(d["states"][s], d["sc"]["P0"], want_P=True)),
    "iterate_batch": (_prep_scan, lambda capi, ctx, d, s: ctx.iterate_batch(d["states"][s])),
    "visibility": (_none, _on_map(lambda capi, ctx, d, s: ctx.map_remove_dynamic(d["views"][s], dry_run=True))),
    "paint": (_none, _on_map(lambda capi, ctx, d, s: ctx.map_paint(d["cams"][s]))),
    "place": (_prep_map, _place),
    "surface": (_none, _on_map(lambda capi, ctx, d, s: ctx.map_normals())),
    "outliers": (_none, _on_map(lambda capi, ctx, d, s: ctx.map_remove_outliers(dry_run=True))),
    "cluster": (_none, _on_map(lambda capi, ctx, d, s: ctx.map_cluster(capi.default_cluster_params(radius=0.8, min_size=2)))),
    "occ_integrate": (_occ_ready, _integrate),
    "occ_query": (_occ_ready, lambda capi, ctx, d, s: ctx.occ_query(d["probes"][s])),
    "distance_query": (_occ_ready, lambda capi, ctx, d, s: ctx.occ_distance_query(d["probes"][s])),
    "plan_build": (_occ_ready, _plan_build),
    "plan_paths": (_occ_ready, lambda capi, ctx, d, s: ctx.occ_plan_paths(d["probes"][s])),
}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_small_large_small(capi, data, tool):
    prepare, call = TOOLS[tool]
    sizes = (SMALL, LARGE, SMALL)
    with capi.Context() as ctx:
        prepare(capi, ctx, data)
        kept = [call(capi, ctx, data, s) for s in sizes]
    fresh = {}
    for s in (SMALL, LARGE):
        with capi.Context() as ctx:
            prepare(capi, ctx, data)
            fresh[s] = call(capi, ctx, data, s)
    for s, got in zip(sizes, kept):
        _same_bits(got, fresh[s])
    # (the sizes do differ: a test that staged the same thing three times would hold nothing)
    fs, fl = _flat(fresh[SMALL]), _flat(fresh[LARGE])
    assert len(fs) != len(fl) or any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(fs, fl))


def _after_configure(capi, ctx, d):
    _occ_ready(capi, ctx, d, SMALL)
    return (ctx.occ_fetch(), ctx.occ_distance_fetch(), ctx.occ_plan_fetch(), ctx.occ_query(d["probes"][LARGE]),
            ctx.occ_distance_query(d["probes"][LARGE]), ctx.occ_plan_paths(d["probes"][LARGE]))


def test_a_smaller_grid_configured_over_a_larger(capi, data):
    with capi.Context() as ctx:
        _occ_ready(capi, ctx, data, LARGE)
        ctx.occ_query(data["probes"][LARGE])
        ctx.occ_distance_query(data["probes"][LARGE])
        ctx.occ_plan_paths(data["probes"][LARGE])
        kept = _after_configure(capi, ctx, data)
    with capi.Context() as ctx:
        fresh = _after_configure(capi, ctx, data)
    _same_bits(kept, fresh)
    assert kept[0].shape == (4, 8, 8)
