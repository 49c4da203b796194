"""Timing of the elevation map (lv_elev_build) from the device map of the 1 M-point bench scene (synth.make_scene).  Two grids: the
default one (512 x 512 at 0.2 m) and the same footprint at 0.1 m (1024 x 1024).  Per grid:
  `ms_median`, `ms_min`  host wall time of lv_elev_build with pts = NULL (the map's points swept twice, the terrain kernel, the fold,
                  the stats copied back, one synchronise), over --reps calls after two warm-up calls;
  `stats`         points used, overhang points, known cells, lethal cells;
  `fetch_class_ms`  lv_elev_fetch(LV_ELEV_CLASS), the int8 grid a planner takes;
  `kernels`       per kernel calls / average / min / max ms from a `rocprofv3 --kernel-trace --stats` run of this script with
                  --case NAME, a run of its own per case (attached afterwards: --merge ... --attach NAME=kernel_stats.csv).
The baseline is what a user did before: `map_fetch_ms` (lv_map_fetch of the living points) plus `numpy_ms`, the rule in numpy on
the host (tests/elevation_ref.py) on the default grid; `numpy_agrees` says that its layers and stats equal the device's.
Prints one JSON line; --out writes it too.

    python scripts/elevation_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_default -- python scripts/elevation_timing.py --case default --no-numpy
    python scripts/elevation_timing.py --merge plain.json --attach default=prof_default/.../kernel_stats.csv \
        --out profiles/elevation_timing.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

KERNELS = ("elev_low_kernel", "elev_band_kernel", "elev_terrain_kernel", "elev_stats_kernel")
CASES = {
    "default": dict(),
    "res_0.1": dict(resolution=0.1, nx=1024, ny=1024, head=3840, max_span=307, max_step=256),   # the same metres at 0.1 m
}


def kernel_ms(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key in row["Name"]:
                    out[row["Name"].split("(")[0]] = dict(calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6,
                                                          min_ms=float(row["MinNs"]) * 1e-6, max_ms=float(row["MaxNs"]) * 1e-6)
    return out


def merge(path, attach, out):
    with open(path) as f:
        res = json.loads(f.readline())
    for item in attach or []:
        name, csv_path = item.split("=", 1)
        ks = kernel_ms(csv_path)
        res["cases"][name]["kernels"] = ks
        res["cases"][name]["kernels_ms_sum"] = sum(v["avg_ms"] for v in ks.values())
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, choices=sorted(CASES), help="this case only (for a profiled run)")
    ap.add_argument("--attach", action="append", default=None, metavar="CASE=CSV", help="with --merge: a case's rocprofv3 kernel_stats.csv")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--merge", default=None, metavar="JSON", help="a result of this script to attach kernel times to (no GPU)")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.attach, a.out)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, synth

    scene = synth.make_scene(a.points, 2_000)
    res = dict(what="lv_elev_build from the device map", map_points=int(len(scene["map_xyz"])), reps=a.reps, cases={})
    with capi.Context() as ctx:
        ctx.map_build(scene["map_xyz"])
        for name, kw in CASES.items():
            if a.case and name != a.case:
                continue
            p = capi.default_elevation_params(**kw)
            for _ in range(2):   # warm-up: allocation, code objects
                st = ctx.elev_build(p)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.elev_build(p)
                ts.append((time.perf_counter() - t0) * 1e3)
            ctx.elev_fetch(capi.LV_ELEV_CLASS)
            tf = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.elev_fetch(capi.LV_ELEV_CLASS)
                tf.append((time.perf_counter() - t0) * 1e3)
            row = dict(params=kw, grid=f"{p.nx}x{p.ny} @ {p.resolution:.3g} m", ms_median=float(np.median(ts)), ms_min=float(np.min(ts)),
                       ms_max=float(np.max(ts)), stats=[int(v) for v in st], fetch_class_ms=float(np.median(tf)))
            res["cases"][name] = row
            print(json.dumps({name: row}), file=sys.stderr)
        if not a.no_numpy and not a.case:
            import elevation_ref as er

            p = capi.default_elevation_params()
            prm = er.params(origin=[float(v) for v in p.origin], resolution=float(p.resolution), nx=p.nx, ny=p.ny, min_points=p.min_points,
                            head=p.head, max_span=p.max_span, max_step=p.max_step, max_slope2=p.max_slope2)
            tm = []
            for _ in range(3):
                t0 = time.perf_counter()
                pts = ctx.map_fetch()
                tm.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            want, wstats = er.build(prm, pts)
            res["map_fetch_ms"] = float(np.median(tm))
            res["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            st = ctx.elev_build(p)
            got = {n: ctx.elev_fetch(layer) for layer, (n, _) in enumerate(capi.ELEV_LAYERS)}
            res["numpy_agrees"] = bool(er.same_layers(got, want) is None and np.array_equal(st, wstats))
            res["speedup_vs_fetch_and_numpy"] = (res["map_fetch_ms"] + res["numpy_ms"]) / res["cases"]["default"]["ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
