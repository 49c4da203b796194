"""Timing of the colour layer (lv_colour_integrate, the vertex colours inside lv_tsdf_mesh_build) on the default 512 x 512 x 64
volume at 0.2 m after the ten 64 x 2048 sweeps of scripts/occupancy_timing.py, with Full-HD views (1920 x 1080, f = 1000 px) that
stand at the sweeps' poses and look round the horizon.
  `integrate_1_ms`, `integrate_32_ms`  host wall time of lv_colour_integrate with 1 and with 32 views (staging and upload of the
                  images, compaction, occlusion buffer, fold, the stats copied back): median / min / max of REPEATS, after one
                  call that allocates the layer and the buffers;
  `stats_1`, `stats_32`  what the calls counted: candidates, pairs projected, pairs seen, voxels coloured;
  `host_1_ms`     the host route for ONE view: lv_tsdf_fetch of S and W plus the numpy rule of tests/colour_ref.py;
  `mesh_build_ms` lv_tsdf_mesh_build(min_weight 1) without the layer and with it (the same volume), and `mesh_colours_ms` the
                  copy of the vertex colours;
  `plain_route`   the one-lane-per-voxel route the list route was to be compared with: not built, so not recorded.
Prints one JSON line; --out writes it too.

    python scripts/colour_timing.py --sweeps /tmp/occ_sweeps.npz [--out profiles/colour_timing.json] [--no-host]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

REPEATS = 5
WIDTH, HEIGHT, FOCAL = 1920, 1080, 1000.0


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def make_frames(sweeps, n):
    """n Full-HD views: view i stands at the pose of sweep i % len(sweeps) and looks along the horizon at yaw i * 360 / n."""
    jj, ii = np.meshgrid(np.arange(HEIGHT), np.arange(WIDTH), indexing="ij")
    base = np.stack([(ii // 8) % 256, (jj // 4) % 256, (ii + jj) // 12 % 256], axis=2).astype(np.uint8)
    frames = []
    for i in range(n):
        yaw = 2 * math.pi * i / n
        z = np.array([math.cos(yaw), math.sin(yaw), 0.0])
        x = np.cross(z, [0.0, 0.0, 1.0])
        R = np.stack([x, np.cross(z, x), z], axis=1).astype(np.float32)
        t = np.asarray(sweeps[i % len(sweeps)][1], np.float32)
        frames.append(dict(R=R, t=t, fx=FOCAL, fy=FOCAL, cx=(WIDTH - 1) / 2, cy=(HEIGHT - 1) / 2, image=np.roll(base, 37 * i, axis=1)))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi

    frames = make_frames(sweeps, 32)
    prm = capi.default_colour_params()
    res = dict(what="lv_colour_integrate / vertex colours in lv_tsdf_mesh_build", grid="512x512x64 @ 0.2 m (defaults), trunc_cells 3",
               sweeps=f"{len(sweeps)} x {occupancy_timing.RINGS}x{occupancy_timing.AZ}", views=f"{WIDTH}x{HEIGHT}, f = {FOCAL:g} px",
               params=dict(zbuf_scale=prm.view.zbuf_scale, window=prm.view.window, band=prm.band, max_weight=prm.max_weight),
               plain_route="not built: not recorded")
    with capi.Context() as ctx:
        ctx.tsdf_configure(capi.default_tsdf_params())
        ctx.tsdf_integrate(sweeps)
        ctx.tsdf_mesh_build()   # warm-up
        grey = [timed(ctx.tsdf_mesh_build)[0] for _ in range(REPEATS)]
        ctx.colour_integrate(frames, prm)   # allocates the layer and the buffers
        for n in (1, 32):
            ts = []
            for _ in range(REPEATS):
                ms, stats = timed(lambda: ctx.colour_integrate(frames[:n], prm))
                ts.append(ms)
            res[f"integrate_{n}_ms"] = spread(ts)
            res[f"stats_{n}"] = [int(v) for v in stats]
        built = [timed(ctx.tsdf_mesh_build) for _ in range(REPEATS)]
        res["mesh_build_ms"] = dict(without_layer=spread(grey), with_layer=spread([b[0] for b in built]))
        res["mesh"] = [int(v) for v in built[-1][1]]
        res["mesh_colours_ms"] = spread([timed(ctx.mesh_colours)[0] for _ in range(REPEATS)])
        if not a.no_host:
            import colour_ref

            p = ctx.tsdf_params()

            def host():
                vol = ctx.tsdf_fetch(S=True, W=True)
                return colour_ref.integrate(vol["S"], vol["W"], None, [float(v) for v in p.origin], p.resolution, frames[:1], prm)

            ms, out = timed(host)
            res["host_1_ms"] = ms
            assert int(out["stats_lo"][0]) == res["stats_1"][0]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
