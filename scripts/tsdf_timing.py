"""Timing of TSDF fusion and the mesh build (lv_tsdf_integrate / lv_tsdf_mesh_build) on the ten 64 x 2048 sweeps of
scripts/occupancy_timing.py, fused into the default 512 x 512 x 64 volume at 0.2 m (trunc_cells 3), with carve 0 and carve 1.
  `one_sweep_ms`  host wall time of lv_tsdf_integrate with one sweep per call (staging, upload, march, fold, the stats copied back);
                  the ten sweeps after a clear, the whole round repeated REPEATS times: median / min / max over all calls;
  `ten_sweeps_ms` the ten sweeps as ONE call (one fold), after a clear: median / min / max of REPEATS;
  `mesh_build_ms` lv_tsdf_mesh_build(min_weight 1) of the volume the ten sweeps leave, and `mesh_fetch_ms` the copy of its arrays;
  `stats`, `mesh` what the call and the build counted (they must equal the host's);
  `kernels`       the kernels' own times, from a `rocprofv3 --kernel-trace --stats` run of this script with --once (--kernel-stats
                  CSV: both carves together; --kernel-trace CSV: `kernels_by_carve`, split by launch order; `scan_impl` is hipcub's scan);
  `host`          scripts/tsdf_host.cpp, the same rule (lv_tsdf.hpp) built with g++ -O2 on one core: the ten sweeps as one call,
                  then the mesh.
The library timed is the one capi loads (LV_LIB_PATH names another build); --label names it in the output and --merge FILE takes
over the entries of an earlier run of this script, so that two builds can stand side by side in one file.
Prints one JSON line; --out writes it too.

    python scripts/tsdf_timing.py --sweeps /tmp/occ_sweeps.npz [--label library] [--merge other.json] [--out profiles/tsdf_timing.json]"""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

REPEATS = 5
KERNELS = ("tsdf_march_kernel", "tsdf_fold_kernel", "tsdf_classify_kernel", "tsdf_vertex_kernel", "tsdf_face_count_kernel",
           "tsdf_face_emit_kernel")


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(path):
    """{kernel: calls and average / min / max ms} from rocprofv3's kernel_stats.csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key in row["Name"]:
                    out[key] = dict(calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6, min_ms=float(row["MinNs"]) * 1e-6,
                                    max_ms=float(row["MaxNs"]) * 1e-6)
    return out


def kernels_by_carve(path):
    """{carve0: {kernel: calls, avg / min / max ms}, carve1: ...} from rocprofv3's kernel_trace.csv of a run of this script: the
    dispatches in start order; this script runs carve 0 first and launches as many march kernels for either, so the second half
    of the march launches opens carve 1."""
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    seq = [(k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6) for r in rows for k in KERNELS + ("scan_impl",)
           if k in r["Kernel_Name"]]
    marches = [i for i, (k, _) in enumerate(seq) if k == "tsdf_march_kernel"]
    cut = marches[len(marches) // 2]
    out = {}
    for label, part in (("carve0", seq[:cut]), ("carve1", seq[cut:])):
        d = {}
        for k, ms in part:
            d.setdefault(k, []).append(ms)
        out[label] = {k: dict(calls=len(v), avg_ms=float(np.mean(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v))) for k, v in d.items()}
    return out


def host_baseline(p, sweeps, min_weight=1):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tsdf_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "tsdf_host.cpp"), "-o", exe])
        with open(os.path.join(d, "params"), "wb") as f:
            f.write(np.array(list(p.origin) + [p.resolution, p.min_range, p.max_range], np.float32).tobytes())
            f.write(np.array([p.nx, p.ny, p.nz, p.trunc_cells, p.max_weight, p.carve, min_weight], np.int32).tobytes())
        with open(os.path.join(d, "views"), "wb") as f:
            f.write(np.array([len(sweeps)], np.int32).tobytes())
            for R, t, pts in sweeps:
                f.write(np.asarray(R, np.float32).tobytes() + np.asarray(t, np.float32).tobytes() + np.array([len(pts)], np.int32).tobytes())
            for _, _, pts in sweeps:
                f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        return json.loads(subprocess.check_output([exe, os.path.join(d, "params"), os.path.join(d, "views")]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--label", default="library")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-trace", default=None, help="kernel_trace.csv of a profiled run of this script: the kernels' times per carve")
    ap.add_argument("--no-host", action="store_true", help="leave the host baseline out (a second build: it is the same)")
    ap.add_argument("--once", action="store_true", help="one round only (the profiled run: its kernel statistics, not its wall times, are wanted)")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi

    repeats = 1 if a.once else REPEATS
    res = dict(what="lv_tsdf_integrate / lv_tsdf_mesh_build", grid="512x512x64 @ 0.2 m (defaults), trunc_cells 3",
               sweeps=f"{len(sweeps)} x {occupancy_timing.RINGS}x{occupancy_timing.AZ}", builds={}, host={})
    row = dict(lib=os.path.basename(capi.LIB_PATH))
    if a.kernel_stats:
        row["kernels"] = kernel_ms(a.kernel_stats)
    if a.kernel_trace:
        row["kernels_by_carve"] = kernels_by_carve(a.kernel_trace)
    with capi.Context() as ctx:
        for carve in (0, 1):
            p = capi.default_tsdf_params(carve=carve)
            ctx.tsdf_configure(p)
            ctx.tsdf_integrate(sweeps[:1])   # warm-up: staging buffers, code objects
            ctx.tsdf_integrate(sweeps)
            ctx.tsdf_mesh_build()
            ctx.tsdf_mesh_fetch()
            one, ten, build, fetch = [], [], [], []
            for _ in range(repeats):
                ctx.tsdf_clear()
                for v in sweeps:
                    one.append(timed(lambda: ctx.tsdf_integrate([v]))[0])
                ctx.tsdf_clear()
                ms, stats = timed(lambda: ctx.tsdf_integrate(sweeps))
                ten.append(ms)
                ms, counts = timed(ctx.tsdf_mesh_build)
                build.append(ms)
                fetch.append(timed(ctx.tsdf_mesh_fetch)[0])
            c = dict(one_sweep_ms=spread(one), ten_sweeps_ms=spread(ten), mesh_build_ms=spread(build), mesh_fetch_ms=spread(fetch),
                     stats=[int(v) for v in stats], mesh=[int(v) for v in counts])
            row["carve%d" % carve] = c
            print(json.dumps({"carve": carve, **c}), file=sys.stderr)
            if not a.no_host:
                h = host_baseline(p, sweeps)
                assert h["stats"] == c["stats"] and [h["vertices"], h["triangles"], h["vertices"], h["refused"]] == c["mesh"], (h, c)
                res["host"]["carve%d" % carve] = h
    res["builds"][a.label] = row
    if a.merge:
        with open(a.merge) as f:
            old = json.load(f)
        for k, v in old["builds"].items():
            res["builds"].setdefault(k, v)
        if not res["host"]:
            res["host"] = old.get("host", {})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
