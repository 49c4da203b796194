"""Times lv_map_planes against the route the entry points offered before it: lv_map_fetch, then the same rule on one CPU core
(scripts/map_planes_host.cpp, the library's own lv_planes.hpp compiled with g++ -O2).  Bench scene; K = 512 and 4096 hypotheses,
1 and 8 planes, with and without the refit.  GPU: best of 3 after a warm-up, whole calls (host clock).  CPU: one run of the
extraction alone (its file I/O is not counted; the fetch is timed beside it).  Both routes end with the same thing in host memory,
a plane label per map point, and the script asserts that the two are equal.

    python scripts/map_planes_timing.py [--points 1000000] [--out profiles/map_planes_timing.json] [--gpu-only]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import lvamd  # noqa: E402

lvamd.load()
from limo_velo_amd import capi, synth  # noqa: E402


def best_of(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--iterations", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--distance", type=float, default=0.1)
    ap.add_argument("--gpu-only", action="store_true", help="no CPU route (a profiler run)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    xyz = synth.make_scene(a.points, 1000)["map_xyz"]
    res = dict(points=int(len(xyz)), scene="bench", distance=a.distance, runs=[])
    with tempfile.TemporaryDirectory() as tmp, capi.Context() as ctx:
        exe = os.path.join(tmp, "map_planes_host")
        if not a.gpu_only:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "scripts", "map_planes_host.cpp"), "-o", exe])
        ctx.map_build(xyz)
        t_fetch, own = best_of(ctx.map_fetch)
        res["map_fetch_ms"] = t_fetch
        pts, lab = os.path.join(tmp, "points.f32"), os.path.join(tmp, "labels.i32")
        np.ascontiguousarray(own, np.float32).tofile(pts)
        for K in a.iterations:
            for P in a.planes:
                for refine in (1, 0):
                    prm = capi.default_plane_params(distance=a.distance, iterations=K, max_planes=P, refine=refine)
                    t_gpu, out = best_of(lambda: ctx.map_planes(prm))
                    run = dict(iterations=K, max_planes=P, refine=refine, n_planes=int(out["n_planes"]), map_planes_ms=t_gpu,
                               inliers=[int(v) for v in out["planes"]["inliers"]], tests=int(K * out["planes"]["candidates"].astype(np.int64).sum()))
                    if not a.gpu_only:
                        line = subprocess.check_output([exe, pts, lab, repr(float(np.float32(a.distance))), str(K), str(P), str(prm.min_inliers), str(prm.seed),
                                                        "0", "0", "0", "1", repr(float(prm.max_angle)), str(refine)], text=True).split()
                        host = np.fromfile(lab, np.int32)
                        same = bool(np.array_equal(host, out["labels"])) and int(line[1]) == out["n_planes"]
                        assert same, f"K {K}, {P} planes, refine {refine}: the CPU route and lv_map_planes differ"
                        t_cpu = float(line[0])
                        run.update(host_one_core_ms=t_cpu, fetch_plus_host_ms=t_fetch + t_cpu, speedup=(t_fetch + t_cpu) / t_gpu, same_labels=same)
                    res["runs"].append(run)
                    print(json.dumps(run), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
