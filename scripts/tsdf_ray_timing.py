"""Timing of ray casting on the TSDF surface (lv_surf_raycast / lv_surf_raycast_views) on the volume scripts/tsdf_timing.py builds:
its ten 64 x 2048 sweeps fused into the default 512 x 512 x 64 volume at 0.2 m (carve 0), every observed voxel given a colour.
  `raycast`     64 x 2048 rays of 80 m from the first pose (scan_pattern), records only: `first_ms`, the call after the volume
                changed (it packs the cell states first; median of 5, the change being an lv_tsdf_load of the volume's own values
                and the layer loaded again), and `later_ms`, the calls after it (median of 20); host wall time of the whole call,
                the results copied back.  `full_ms`: the later calls with normals and colours.
  `render`      mesh.render of a 640 x 480 pinhole camera at the first pose, looking along its heading: `ms`, median of 10
                (lv_surf_raycast_views with normals and colours, and the images put together in numpy).
  `occ_raycast` lv_occ_raycast of the same rays on the occupancy grid of the same sweeps: the yardstick (median of 20).
  `host`        what a caller without these calls pays: `fetch_ms` (lv_tsdf_fetch, median of 5) plus scripts/tsdf_ray_host.cpp, the
                same rule (lv_tsdf_ray.hpp) built with g++ -O2 on one core, for the same rays; its records and normals must
                equal the library's.
The library timed is the one capi loads (LV_LIB_PATH names another build); --label names it in the output and --merge FILE takes
over the entries of an earlier run of this script, so that two builds can stand side by side in one file: that is how the
packed_* and direct_* entries of profiles/tsdf_ray_timing.json were taken (DESIGN.md "Surface ray casting"; the direct build is not
in the tree), and the three options are kept for the next comparison build.
Prints one JSON line; --out writes it too.

    python scripts/tsdf_ray_timing.py --sweeps /tmp/occ_sweeps.npz [--label packed] [--merge other.json] [--out profiles/tsdf_ray_timing.json]"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

RINGS, AZ, RANGE = 64, 2048, 80.0
WIDTH, HEIGHT, FOCAL = 640, 480, 400.0


def median_ms(fn, n, before=None):
    ts = []
    for _ in range(n):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=n)


def host_baseline(p, vol, frm, to, min_weight=1):
    """(the host's JSON, its records, its normals)"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tsdf_ray_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "tsdf_ray_host.cpp"), "-o", exe])
        with open(os.path.join(d, "params"), "wb") as f:
            f.write(np.array(list(p.origin) + [p.resolution, p.min_range, p.max_range], np.float32).tobytes())
            f.write(np.array([p.nx, p.ny, p.nz, p.trunc_cells, p.max_weight, p.carve, min_weight], np.int32).tobytes())
        vol["S"].tofile(os.path.join(d, "S"))
        vol["W"].tofile(os.path.join(d, "W"))
        np.hstack([frm, to]).astype(np.float32).tofile(os.path.join(d, "rays"))
        out = json.loads(subprocess.check_output([exe] + [os.path.join(d, n) for n in ("params", "S", "W", "rays", "out")]))
        raw = np.fromfile(os.path.join(d, "out"), np.uint8)
    n = len(frm)
    return out, raw[:32 * n].view(np.int32).reshape(n, 8), raw[32 * n:].view(np.float32).reshape(n, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--label", default="library")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the host baseline and the yardstick out (a second build: they are the same)")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, mesh, occupancy

    R0, t0 = np.asarray(sweeps[0][0], np.float32), np.asarray(sweeps[0][1], np.float32)
    to = (occupancy.scan_pattern(AZ, RINGS, math.radians(-25.0), math.radians(3.0), RANGE) @ R0.T + t0).astype(np.float32)
    frm = np.ascontiguousarray(np.broadcast_to(t0, to.shape))
    Rc = (R0 @ np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)).astype(np.float32)   # camera z along the sensor's x
    res = dict(what="lv_surf_raycast / lv_surf_raycast_views", grid="512x512x64 @ 0.2 m (defaults), ten 64x2048 sweeps fused, carve 0",
               rays=f"{RINGS}x{AZ} x {RANGE} m from one pose", render=f"{WIDTH}x{HEIGHT}, f = {FOCAL}", builds={})
    with capi.Context() as ctx:
        ctx.tsdf_configure()
        ctx.tsdf_integrate(sweeps)
        vol = ctx.tsdf_fetch()
        p = ctx.tsdf_params()
        layer = np.zeros(vol["W"].shape + (4,), np.uint32)
        layer[vol["W"] > 0] = (200, 120, 40, 1)
        ctx.colour_load(layer)

        def cast(normals=False, colours=False):
            return ctx.tsdf_raycast(frm, to, None, normals, colours)

        def change():
            ctx.tsdf_load(vol["S"], vol["W"])
            ctx.colour_load(layer)

        out, nrm, col = cast(True, True)   # warm-up: buffers, code objects
        mesh.render(ctx, Rc, t0, FOCAL, FOCAL, (WIDTH - 1) / 2, (HEIGHT - 1) / 2, WIDTH, HEIGHT)
        row = dict(lib=os.path.basename(capi.LIB_PATH))
        row["raycast"] = dict(first_ms=median_ms(cast, 5, before=change), later_ms=median_ms(cast, 20), full_ms=median_ms(lambda: cast(True, True), 20),
                              hit=int((out["status"] == capi.LV_SURF_HIT).sum()), blocked=int((out["status"] == capi.LV_SURF_BLOCKED).sum()),
                              steps=int(out["steps"].sum()), coloured=int(col[:, 3].astype(bool).sum()))
        depth, _, _ = mesh.render(ctx, Rc, t0, FOCAL, FOCAL, (WIDTH - 1) / 2, (HEIGHT - 1) / 2, WIDTH, HEIGHT)
        row["render"] = dict(ms=median_ms(lambda: mesh.render(ctx, Rc, t0, FOCAL, FOCAL, (WIDTH - 1) / 2, (HEIGHT - 1) / 2, WIDTH, HEIGHT), 10),
                             pixels_hit=int(np.isfinite(depth).sum()))
        res["builds"][a.label] = row
        if not a.no_host:
            h, h_res, h_nrm = host_baseline(p, vol, frm, to)
            assert np.array_equal(h_res, out.view(np.int32).reshape(-1, 8)) and np.array_equal(h_nrm.view(np.uint32), nrm.view(np.uint32))
            res["host"] = dict(fetch_ms=median_ms(ctx.tsdf_fetch, 5), equal_outputs=True, **h)
            ctx.occ_configure()
            ctx.occ_integrate(sweeps)
            prm = capi.default_ray_params()
            occ = ctx.occ_raycast(frm, to, prm)
            res["occ_raycast"] = dict(later_ms=median_ms(lambda: ctx.occ_raycast(frm, to, prm), 20), stopped=int((occ["status"] == capi.LV_RAY_STOPPED).sum()),
                                      steps=int(occ["steps"].sum()))
    if a.merge:
        with open(a.merge) as f:
            old = json.load(f)
        for k, v in old["builds"].items():
            res["builds"].setdefault(k, v)
        for k in ("host", "occ_raycast"):
            if k in old:
                res.setdefault(k, old[k])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
