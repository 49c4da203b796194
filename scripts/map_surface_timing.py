"""Times lv_map_normals / lv_map_remove_outliers against what the parent's entry points offer for the same job: lv_map_knn over
the map's own points at the same k.  Best of 3 after a warm-up, whole calls (host clock); the device time per kernel comes from
running one operation at a time under `rocprofv3 --kernel-trace --stats -- python scripts/map_surface_timing.py --only OP`.

    python scripts/map_surface_timing.py [--points 1000000] [--k 10] [--ring] [--only knn|normals|stat|radius] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lvamd  # noqa: E402

lvamd.load()
from limo_velo_amd import capi, synth  # noqa: E402


def best_of(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ring", action="store_true", help="the ring scene of scripts/map_paint_timing.py instead of the bench scene")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    xyz = (synth.make_ring_scene(a.points, 64, 2048) if a.ring else synth.make_scene(a.points, 1000))["map_xyz"]
    res = dict(points=int(len(xyz)), k=a.k, scene="ring" if a.ring else "bench")
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        own = ctx.map_fetch()
        ops = {
            "knn": lambda: ctx.map_knn(own, a.k, 2.0),
            "normals": lambda: ctx.map_normals(capi.default_surface_params(k=a.k)),
            "stat": lambda: ctx.map_remove_outliers(capi.default_outlier_params(mode=0, k=a.k), dry_run=True),
            "radius": lambda: ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.5, min_neighbours=3), dry_run=True),
        }
        for name, fn in ops.items():
            if a.only and a.only != name:
                continue
            res[name + "_call_ms"] = best_of(fn)
    if "knn_call_ms" in res and "normals_call_ms" in res:
        res["normals_over_knn_call"] = res["normals_call_ms"] / res["knn_call_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
