"""GPU tests of lv_map_paint (lv_paint.hip): colours for the map's points from camera images, against the numpy statement of the
rule in tests/paint_ref.py.  Counts must equal the reference on every decided point (see there) and lie inside the admissible
interval on the others, whose share is bounded; colours are held to the reference within 0.01 levels on images whose neighbouring
pixels differ by at most 2 levels (random images serve only the count checks)."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import paint_ref as pr

pytestmark = pytest.mark.gpu

LV_EINVAL = -1
W, H = 640, 480
FX, FY, CX, CY = 420.0, 415.0, 319.3, 240.6
DIST = (-0.28, 0.07, 1.0e-3, -5.0e-4, 0.01)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def look_at(t, target):
    """R camera -> world (x right, y down, z forward) of a camera at t looking at target, the world's z up."""
    z = np.asarray(target, np.float64) - np.asarray(t, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def smooth_image(w, h, seed, channels=3):
    """uint8 [h, w, channels]: sines of periods >= 400 px and amplitude <= 100 levels: neighbouring pixels differ by <= 2 levels."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = []
    for _ in range(channels):
        px, py, ph = rng.uniform(400, 900), rng.uniform(400, 900), rng.uniform(0, 2 * math.pi)
        out.append(128.0 + 60.0 * np.sin(2 * math.pi * ii / px + ph) + 40.0 * np.cos(2 * math.pi * jj / py - ph))
    img = np.clip(np.rint(np.stack(out, axis=2)), 0, 255).astype(np.uint8)
    return img[:, :, 0] if channels == 1 else img


def frame(R, t, image, fmt=None, dist=None, fx=FX, fy=FY, cx=CX, cy=CY):
    f = dict(R=np.asarray(R, np.float32), t=np.asarray(t, np.float32), fx=fx, fy=fy, cx=cx, cy=cy, image=image,
             dist=np.zeros(5, np.float32) if dist is None else np.asarray(dist, np.float32))
    if fmt is not None:
        f["format"] = fmt
    return f


@pytest.fixture(scope="module")
def scene(capi):
    from limo_velo_amd import synth

    M = 200_000
    sc = synth.make_ring_scene(M, 16, 512)
    # three cameras 1.5-2 m apart, looking into overlapping parts of the scene
    p0 = np.array([3.0, -2.0, 1.6])
    eyes = [p0, p0 + [1.5, -1.0, 0.0], p0 + [-1.0, 1.5, 0.3]]
    targets = [p0 + [10.0, 4.0, -1.0], p0 + [12.0, 1.0, -1.5], p0 + [9.0, 7.0, -1.0]]
    poses = [(look_at(e, tg), e.astype(np.float32)) for e, tg in zip(eyes, targets)]
    return dict(sc=sc, map=sc["map_xyz"], rects=synth.scene_surfaces(M), poses=poses)


def _frames(capi, scene, smooth=True):
    """Three views: plain RGB8 with strided rows, BGR8 with distortion, MONO8."""
    (R0, t0), (R1, t1), (R2, t2) = scene["poses"]
    if smooth:
        i0, i1, i2 = smooth_image(W, H, 1), smooth_image(W, H, 2), smooth_image(W, H, 3, channels=1)
    else:
        rng = np.random.default_rng(5)
        i0, i1, i2 = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
                      rng.integers(0, 256, (H, W), dtype=np.uint8))
    wide = np.zeros((H, W + 7, 3), np.uint8)
    wide[:, :W] = i0
    return [frame(R0, t0, wide[:, :W]), frame(R1, t1, i1, fmt=capi.LV_IMAGE_BGR8, dist=DIST), frame(R2, t2, i2, fmt=capi.LV_IMAGE_MONO8)]


# At zbuf_scale 1 every pixel border is a cell edge: ~2 x 2e-3 of a view's points lie within 1e-3 px of one, and their
# neighbours' decisions follow them through the occlusion buffer; 1.5 % of the judged points is the bound.
def _check_counts(n_seen, lo, hi, decided, what, max_share=0.015, min_seen=1000):
    n = np.asarray(n_seen, np.int64)
    bad = np.flatnonzero(decided & (n != lo))
    assert bad.size == 0, f"{what}: {bad.size} counts differ from the reference, first {bad[:8]} got {n[bad[:8]]} want {lo[bad[:8]]}"
    assert np.all((n >= lo) & (n <= hi)), f"{what}: a count outside its admissible interval"
    judged = int((hi > 0).sum())
    share = float((~decided).sum()) / max(judged, 1)
    print(f"{what}: {judged} judged, {int((~decided).sum())} undecided ({100 * share:.3f} %), {int((n > 0).sum())} seen")
    assert share < max_share, share
    assert (n > 0).sum() > min_seen


def _check_colours(rgb, depth, ref_rgb, ref_depth, lo, decided, what):
    ok = decided & (lo > 0)
    err = np.abs(rgb[ok].astype(np.float64) - ref_rgb[ok]).max()
    print(f"{what}: max |rgb - ref| {err:.2e} levels over {int(ok.sum())} points")
    assert err <= 0.01, err
    assert np.all(np.isinf(depth[decided & (lo == 0)])) and np.all(rgb[decided & (lo == 0)] == 0)
    assert np.abs(depth[ok] - ref_depth[ok]).max() <= 1e-5 * ref_depth[ok].max()


@pytest.mark.parametrize("blend,scale,window", [(0, 4, 2), (1, 1, 0), (0, 1, 2), (1, 4, 0)])
def test_rule_parity(capi, scene, blend, scale, window):
    prm = capi.default_paint_params(blend=blend, zbuf_scale=scale, window=window)
    frames = _frames(capi, scene)
    with capi.Context() as ctx:
        ctx.map_build(scene["map"])
        rgb, depth, n_seen = ctx.map_paint(frames, prm)
        noise = ctx.map_paint(_frames(capi, scene, smooth=False), prm)
    ref_rgb, ref_depth, lo, hi, decided = pr.paint(scene["map"], frames, prm)
    _check_counts(n_seen, lo, hi, decided, f"blend {blend} scale {scale} window {window}")
    _check_colours(rgb, depth, ref_rgb, ref_depth, lo, decided, "parity")
    assert np.array_equal(noise[2], n_seen) and np.array_equal(_bits(noise[1]), _bits(depth))   # counts do not depend on the images
    assert n_seen.max() >= 2


def _box_scene(capi, scene):
    """The scene's map plus 30 k points on a 2 m box floating 6 m in front of view 0 (its bottom 0.6 m above the ground); the
    images of the three views rendered from the scene's surfaces with the box in front (synth.render_pinhole, the box magenta)."""
    from limo_velo_amd import synth

    R0, t0 = scene["poses"][0]
    centre = t0.astype(np.float64) + 6.0 * R0[:, 2].astype(np.float64)
    centre[2] = 1.6
    box = synth.box_rects(centre, (2.0, 2.0, 2.0))
    box_pts = synth.sample_rects(box, 30_000, seed=12)
    frames = []
    for R, t in scene["poses"]:
        img, _ = synth.render_pinhole(scene["rects"], R, t, FX, FY, CX, CY, W, H, occluders=[(box, BOX_RGB)])
        frames.append(frame(R, t, img))
    return np.concatenate([scene["map"], box_pts]), box, frames


BOX_RGB = (255, 0, 255)


def test_end_to_end_rendered_world(capi, scene):
    from limo_velo_amd import synth

    mp, box, frames = _box_scene(capi, scene)
    ns = len(scene["map"])
    prm = capi.default_paint_params()
    with capi.Context() as ctx:
        ctx.map_build(mp)
        rgb, depth, n_seen = ctx.map_paint(frames, prm)
        one = ctx.map_paint(frames[:1], prm)
    seen = n_seen[:ns] > 0
    err = np.abs(rgb[:ns][seen].astype(np.float64) - synth.texture_rgb(mp[:ns][seen])).max(axis=1)
    med, p99 = float(np.median(err)), float(np.percentile(err, 99))
    print(f"end to end: {int(seen.sum())} scene points seen, |rgb - texture| median {med:.3f} p99 {p99:.2f} max {err.max():.1f}")
    assert med <= 2.0, med
    # The 99th percentile is set by the points on the scene's own silhouettes: a foreground point within a pixel of an edge is
    # seen, and its bilinear taps reach the background behind the edge (up to ~200 levels away on this texture).  Those are
    # ~0.9 % of the seen points in these views (the reference gives 0.88 % above 20 levels, p99 9.5, p99.5 55), so the 99th
    # percentile sits at the foot of that tail; 40 levels allows it to grow by a fifth and no more.
    assert p99 <= 40.0, p99
    box_seen = n_seen[ns:] > 0
    assert box_seen.mean() > 0.1 and np.median(np.abs(rgb[ns:][box_seen] - BOX_RGB).max(axis=1)) <= 1.0
    # the scene behind the box in view 0: inside its silhouette shrunk by window + 1 cells no point is seen, none carries its colour
    R0, t0 = scene["poses"][0]
    _, rb = synth.render_pinhole(box, R0, t0, FX, FY, CX, CY, W, H)
    sil = np.isfinite(rb)
    k = (prm.window + 1) * prm.zbuf_scale
    core = sil.copy()
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            core &= np.roll(np.roll(sil, dy, axis=0), dx, axis=1)
    core[:k], core[-k:], core[:, :k], core[:, -k:] = False, False, False, False
    z, _, u, v = pr.project(mp[:ns], frames[0])
    with np.errstate(invalid="ignore"):
        inside = (z > 0.3) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    behind = np.zeros(ns, bool)
    behind[inside] = core[np.rint(v[inside]).astype(int), np.rint(u[inside]).astype(int)]
    assert behind.sum() > 200, behind.sum()
    assert np.all(one[2][:ns][behind] == 0)
    magenta = (np.abs(rgb[:ns] - BOX_RGB).max(axis=1) < 40.0) & seen
    assert not magenta.any(), f"{int(magenta.sum())} scene points carry the box's colour"


def test_map_order_after_eviction(capi, scene):
    frames = _frames(capi, scene)
    prm = capi.default_paint_params(blend=1)
    with capi.Context() as ctx:
        ctx.map_build(scene["map"])
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], np.float32), np.array([1e3, -2.0, 1e3], np.float32), keep_inside=False)
        left = ctx.map_fetch()
        assert 0.3 * len(scene["map"]) < len(left) < 0.7 * len(scene["map"])
        a = ctx.map_paint(frames, prm)
    with capi.Context() as fresh:
        fresh.map_build(left)
        b = fresh.map_paint(frames, prm)
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert (a[2] > 0).sum() > 1000


def _np_knn_ok(ctx, q, before):
    idx, d2, found = ctx.map_knn(q, 5)
    return np.array_equal(idx, before[0]) and np.array_equal(_bits(d2), _bits(before[1])) and np.array_equal(found, before[2])


def test_read_only(capi, scene):
    sc = scene["sc"]
    frames = _frames(capi, scene)
    q = scene["map"][np.random.default_rng(1).integers(0, len(scene["map"]), 400)] + np.float32(0.03)
    with capi.Context() as ctx:
        ctx.map_build(scene["map"])
        fetched, stats = ctx.map_fetch(), ctx.map_stats()
        knn = ctx.map_knn(q, 5)
        ctx.map_paint(frames, capi.default_paint_params())
        ctx.map_paint(frames, capi.default_paint_params(blend=1, zbuf_scale=1))
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(fetched)) and ctx.map_stats() == stats
        assert _np_knn_ok(ctx, q, knn)
        ctx.scan_set(sc["scan_xyz"])
        x1, P1, p1, _, _ = ctx.update(sc["x_init"], sc["P0"])
    with capi.Context() as plain:
        plain.map_build(scene["map"])
        plain.scan_set(sc["scan_xyz"])
        x2, P2, p2, _, _ = plain.update(sc["x_init"], sc["P0"])
    assert p1 == p2 and np.array_equal(x1.view(np.uint64), x2.view(np.uint64)) and np.array_equal(P1.view(np.uint64), P2.view(np.uint64))


def test_background_rebuild(capi, scene):
    frames = _frames(capi, scene)
    prm = capi.default_paint_params()
    lo_b, hi_b = np.array([-1e3, -1e3, -1e3], np.float32), np.array([1e3, 0.0, 1e3], np.float32)
    with capi.Context() as q:
        q.map_build(scene["map"])
        q.map_evict_box(lo_b, hi_b, keep_inside=False)
        want = q.map_paint(frames, prm)
        want_xyz = q.map_fetch()
    with capi.Context() as ctx:
        ctx.set_option("async_relinearise", 1)
        ctx.map_build(scene["map"])
        ctx.map_evict_box(lo_b, hi_b, keep_inside=False)
        ctx.set_option("async_relinearise_test_delay_ms", 400)
        ctx.map_relinearise_async()
        t0 = time.monotonic()
        while ctx.map_rebuild_status()["state"] in (4, 5) and time.monotonic() - t0 < 10:   # until the snapshot is taken
            ctx.map_size()
            time.sleep(0.001)
        assert ctx.map_rebuild_status()["state"] == 1
        during = ctx.map_paint(frames, prm)
        st = ctx.map_rebuild_status()
        assert st["journal"] == 0 and st["state"] == 1, st
        st = ctx.map_rebuild_status(wait=True)
        assert st["adopted"] >= 1 and st["state"] == 0, st
        after = ctx.map_paint(frames, prm)
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(want_xyz))
    for got in (during, after):
        for x, y in zip(got, want):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def test_determinism_and_view_order(capi, scene):
    frames = _frames(capi, scene)
    perm = [frames[2], frames[0], frames[1]]
    with capi.Context() as ctx:
        ctx.map_build(scene["map"])
        for blend in (0, 1):
            prm = capi.default_paint_params(blend=blend)
            a = ctx.map_paint(frames, prm)
            b = ctx.map_paint(frames, prm)
            for x, y in zip(a, b):
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
            c = ctx.map_paint(perm, prm)
            assert np.array_equal(c[2], a[2]) and np.array_equal(_bits(c[1]), _bits(a[1]))
            if blend == 0:
                assert np.abs(c[0] - a[0]).max() <= 1e-4
            else:   # bitwise equal but where two seeing views give the same z to the bit
                single = [ctx.map_paint([f], prm)[1] for f in frames]
                d = np.stack([_bits(s) for s in single])
                fin = np.stack([np.isfinite(s) for s in single])
                tie = np.zeros(len(a[1]), bool)
                for i in range(3):
                    for j in range(i + 1, 3):
                        tie |= fin[i] & fin[j] & (d[i] == d[j])
                assert np.array_equal(_bits(c[0][~tie]), _bits(a[0][~tie]))


def test_limits(capi, scene):
    frames = _frames(capi, scene)
    good = capi.default_paint_params()
    bad_params = [dict(min_depth=0.0), dict(min_depth=70.0), dict(max_depth=float("inf")), dict(min_depth=float("nan")),
                  dict(max_norm_radius=0.0), dict(max_norm_radius=float("nan")), dict(zbuf_scale=0), dict(zbuf_scale=17),
                  dict(window=-1), dict(window=9), dict(margin_abs=0.0), dict(margin_rel=-0.01), dict(margin_abs=float("inf")),
                  dict(blend=2), dict(blend=-1)]
    big = np.zeros((1, 1), np.uint8)

    def bad_views():
        out = []
        for k, val in (("fx", float("nan")), ("cy", float("inf")), ("t", [0.0, float("nan"), 0.0]), ("R", np.full((3, 3), np.inf)),
                       ("dist", [0, 0, 0, float("nan"), 0])):
            f = dict(frames[0])
            f[k] = val
            out.append([f])
        out.append([frames[0]] * 33)
        out.append([frame(frames[0]["R"], frames[0]["t"], np.zeros((1, 8193), np.uint8))])
        out.append([frame(frames[0]["R"], frames[0]["t"], np.zeros((4097, 4097), np.uint8))])
        out.append([frame(frames[0]["R"], frames[0]["t"], np.zeros((4096, 4096), np.uint8))] * 5)   # 2^26 + 2^24 pixels
        return out

    with capi.Context() as ctx:
        ctx.map_build(scene["map"])
        m = ctx.map_size()
        fetched = ctx.map_fetch()

        def raw(views, prm, arr=None):
            rgb = np.full((m, 3), 7.0, np.float32)
            depth = np.full(m, 7.0, np.float32)
            seen = np.full(m, 7, np.uint8)
            keep = []
            if arr is None:
                arr = (capi.LvCameraView * max(len(views), 1))()
                for i, f in enumerate(views):
                    arr[i], img = capi.camera_view(f)
                    keep.append(img)
            fp = C.POINTER(C.c_float)
            rc = ctx.lib.lv_map_paint(ctx.h, arr, C.c_size_t(len(views)), C.byref(prm), rgb.ctypes.data_as(fp), depth.ctypes.data_as(fp),
                                      seen.ctypes.data_as(C.POINTER(C.c_uint8)))
            untouched = np.all(rgb == 7.0) and np.all(depth == 7.0) and np.all(seen == 7)
            return rc, untouched

        for kw in bad_params:
            assert raw(frames, capi.default_paint_params(**kw)) == (LV_EINVAL, True), kw
        for views in bad_views():
            assert raw(views, good) == (LV_EINVAL, True)
        assert raw([], good) == (LV_EINVAL, True)
        arr = (capi.LvCameraView * 1)()
        arr[0], keep = capi.camera_view(frames[0])
        arr[0].image = None
        assert raw([frames[0]], good, arr) == (LV_EINVAL, True)
        arr[0], keep = capi.camera_view(frames[0])
        arr[0].row_stride = W * 3 - 1
        assert raw([frames[0]], good, arr) == (LV_EINVAL, True)
        arr[0].row_stride, arr[0].width = W * 3, 0
        assert raw([frames[0]], good, arr) == (LV_EINVAL, True)
        arr[0].width, arr[0].format = W, 3
        assert raw([frames[0]], good, arr) == (LV_EINVAL, True)
        assert ctx.lib.lv_map_paint(ctx.h, None, C.c_size_t(1), C.byref(good), None, None, None) == LV_EINVAL
        assert raw(frames, good)[0] == 0          # the limits themselves pass
        assert raw([frames[0]] * 32, capi.default_paint_params(zbuf_scale=16, window=8))[0] == 0
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(fetched))
    with capi.Context() as unbuilt:                # an unbuilt map: LV_OK, nothing written
        assert unbuilt.map_paint(frames, good)[0].shape == (0, 3)
        assert unbuilt.lib.lv_map_paint(unbuilt.h, (capi.LvCameraView * 1)(*[capi.camera_view(frames[0])[0]]), C.c_size_t(1),
                                        C.byref(good), None, None, None) == 0
    with capi.Context() as empty:                  # every point evicted: LV_OK
        empty.map_build(scene["map"][:1000])
        empty.map_evict_box(np.array([-1e3] * 3, np.float32), np.array([1e3] * 3, np.float32), keep_inside=False)
        assert empty.map_size() == 0
        rgb, depth, seen = empty.map_paint(frames, good)
        assert len(rgb) == len(depth) == len(seen) == 0


def test_vision_buffer_forty_frames(capi, scene):
    from limo_velo_amd import paint

    rng = np.random.default_rng(21)
    buf = paint.VisionBuffer(40)
    frames = []
    for i in range(45):
        p = np.array([3.0, -2.0, 1.6]) + np.r_[rng.uniform(-4, 4, 2), rng.uniform(-0.3, 0.3)]
        a = rng.uniform(-math.pi, math.pi)
        R = look_at(p, p + [math.cos(a), math.sin(a), rng.uniform(-0.3, 0.0)])
        img = smooth_image(320, 240, 100 + i)
        buf.add(0.1 * i, img, R, p, 210.0, 208.0, 159.6, 119.4, dist=DIST if i % 3 == 0 else None)
    frames = buf.frames()
    assert len(frames) == 40
    for blend in (0, 1):
        prm = capi.default_paint_params(blend=blend)
        with capi.Context() as ctx:
            ctx.map_build(scene["map"])
            rgb, depth, n_seen = paint.paint(ctx, buf, prm)
        ref_rgb, ref_depth, lo, hi, decided = pr.paint(scene["map"], frames, prm)
        _check_counts(n_seen, lo, hi, decided, f"40 frames, blend {blend}", max_share=0.02)
        _check_colours(rgb, depth, ref_rgb, ref_depth, lo, decided, "40 frames")
        assert n_seen.max() > 32 or (n_seen > 1).sum() > 1000


def test_scale_one_million_points_full_hd(capi):
    from limo_velo_amd import synth

    M = 1_000_000
    sc = synth.make_ring_scene(M, 16, 512)
    p0 = np.array([3.0, -2.0, 1.6])
    f = frame(look_at(p0, p0 + [8.0, 5.0, -1.2]), p0, smooth_image(1920, 1080, 9), fx=1250.0, fy=1245.0, cx=959.5, cy=539.5, dist=DIST)
    prm = capi.default_paint_params()
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        rgb, depth, n_seen = ctx.map_paint([f], prm)
    ref_rgb, ref_depth, lo, hi, decided = pr.paint(sc["map_xyz"], [f], prm)
    s = np.random.default_rng(3).choice(M, 100_000, replace=False)
    _check_counts(n_seen[s], lo[s], hi[s], decided[s], "1 M points, 1920 x 1080", min_seen=500)   # ~0.9 % of the map is seen
    _check_colours(rgb[s], depth[s], ref_rgb[s], ref_depth[s], lo[s], decided[s], "1 M points")
