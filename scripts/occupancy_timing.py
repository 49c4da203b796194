"""Timing of the occupancy grid (lv_occ_integrate / lv_occ_project) on the 1 M-point bench scene's surfaces: 64-ring x 2048 sweeps
(synth.ring_sweep, range_sigma 0.01) from 10 poses into the default 512 x 512 x 64 grid at 0.2 m.  Per view:
  `rays`          returns used (stats), `cut` of them cut at max_range;
  `updates`       voxels updated (free + hit: the bits the fold finds set);
  `ms`            host wall time of lv_occ_integrate with that one view: staging, upload, march, fold, the stats copied back;
  `march_ms`, `fold_ms`  the kernels' own times, from a `rocprofv3 --kernel-trace --stats` run of this script (--kernel-stats CSV);
  `rays_per_s`, `visits_per_s`  against march_ms when known, else against ms.
`visits_view0`: the in-grid cells the rays of view 0 stand in, counted by tests/occupancy_ref.py (not unique: what the march walks).
`project_ms`: lv_occ_project over all layers, median of 5.  `all_views_ms`: the 10 views in one call.
Prints one JSON line; --out writes it too.  The sweeps are ray-cast on the CPU: --sweeps FILE keeps them (and visits_view0) in an
.npz, so that a second run (the profiled one) does not cast them again.

    python scripts/occupancy_timing.py --sweeps /tmp/occ_sweeps.npz [--out profiles/occupancy_timing.json] [--kernel-stats CSV]"""
import argparse
import csv
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_VIEWS, RINGS, AZ = 10, 64, 2048
M = 1_000_000


def poses():
    """10 poses on a circle of 12 m round the scene's first pose, heading along the tangent, 1.5 m above the ground."""
    out = []
    for i in range(N_VIEWS):
        a = 2.0 * math.pi * i / N_VIEWS
        yaw = a + math.pi / 2
        R = np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1.0]], np.float32)
        out.append((R, np.array([3.0 + 12.0 * math.cos(a), -2.0 + 12.0 * math.sin(a), 1.5], np.float32)))
    return out


def make_sweeps(path, count_visits=True):
    if path and os.path.exists(path):
        with np.load(path) as z:
            return [(z[f"R{i}"], z[f"t{i}"], z[f"p{i}"]) for i in range(N_VIEWS)], int(z["visits_view0"])
    import lvamd

    lvamd.load()
    from limo_velo_amd import synth

    rects = synth.scene_surfaces(M)
    views = [(R, t, synth.ring_sweep(rects, R, t, RINGS, AZ, range_sigma=0.01, seed=11 + i)) for i, (R, t) in enumerate(poses())]
    visits = -1
    if count_visits:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import occupancy_ref as ocr

        prm = ocr.params()
        R, t, pts = views[0]
        qe, _ = ocr.returns(prm, R, t, pts)
        steps, ve = ocr.walk(ocr.view_origin(prm, t), qe)
        dims = np.array([prm["nx"], prm["ny"], prm["nz"]])
        visits = int(np.sum(np.all((ve >= 0) & (ve < dims), axis=1)))
        for cells, alive in steps:
            visits += int(np.sum(alive & np.all((cells >= 0) & (cells < dims), axis=1)))
    if path:
        d = {"visits_view0": np.int64(visits)}
        for i, (R, t, p) in enumerate(views):
            d[f"R{i}"], d[f"t{i}"], d[f"p{i}"] = R, t, p
        np.savez(path, **d)
    return views, visits


def kernel_ms(path):
    """{kernel name fragment: average ms} from rocprofv3's kernel_stats.csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in ("occ_march_kernel", "occ_fold_kernel", "occ_project_kernel"):
                if key in row["Name"]:
                    out[key] = dict(calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6, min_ms=float(row["MinNs"]) * 1e-6,
                                    max_ms=float(row["MaxNs"]) * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--prepare", action="store_true", help="cast and save the sweeps only (no GPU)")
    a = ap.parse_args()
    views, visits0 = make_sweeps(a.sweeps)
    if a.prepare:
        return
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi

    ks = kernel_ms(a.kernel_stats) if a.kernel_stats else {}
    res = dict(what="lv_occ_integrate", grid="512x512x64 @ 0.2 m (defaults)", sweep=f"{RINGS}x{AZ}", map_points_scene=M, views=[],
               visits_view0=visits0, kernels=ks)
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(views[:1])   # warm-up (staging buffers, code objects)
        ctx.occ_clear()
        for v in views:
            t0 = time.perf_counter()
            st = ctx.occ_integrate([v])
            ms = (time.perf_counter() - t0) * 1e3
            row = dict(rays=int(st[0]), cut=int(st[1]), updates=int(st[2] + st[3]), hit=int(st[3]), ms=ms)
            if "occ_march_kernel" in ks:
                row["march_ms"], row["fold_ms"] = ks["occ_march_kernel"]["avg_ms"], ks["occ_fold_kernel"]["avg_ms"]
            base = row.get("march_ms", ms) * 1e-3
            row["rays_per_s"] = row["rays"] / base
            if len(res["views"]) == 0 and visits0 > 0:
                row["visits"] = visits0
                row["visits_per_s"] = visits0 / base
            res["views"].append(row)
            print(json.dumps(row), file=sys.stderr)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            g = ctx.occ_project(0, 63)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["project_ms"] = float(np.median(ts))
        res["projection"] = dict(occupied=int((g == 100).sum()), free=int((g == 0).sum()), unknown=int((g == -1).sum()))
        ctx.occ_clear()
        t0 = time.perf_counter()
        ctx.occ_integrate(views)
        res["all_views_ms"] = (time.perf_counter() - t0) * 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
