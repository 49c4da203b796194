"""Timing of the NDT registration (lv_ndt_build, lv_ndt_align) on the 1 M-point bench scene (synth.make_scene): the target is built
from the device map at 1 m voxels, and the scene's 64k-point scan is aligned from K = 1, 8 and 64 guesses with search 1 and 7.

The baseline is the same rule on one CPU core: scripts/ndt_host.cpp compiles limo-velo_amd/csrc/lv_ndt.hpp with g++ -O2.  Its
moments must equal the device's, and the poses it reaches after --iterations iterations (the first 8 guesses) must lie within the
device test's bound of 1e-8 of the device's: the script asserts both.

Per case:
  `align_ms`        host wall time of lv_ndt_align at --iterations iterations with step_tol = 0 (nothing converges early), median;
  `iter_ms`         device time per iteration: the difference of the wall times at --iterations and at 2 iterations over the
                    difference of the counts (an evaluation launch, a turn launch, and every 8th iteration one look at the count
                    of running hypotheses);
  `host_iter_ms`    one evaluation of ONE hypothesis on the CPU core times K;
  `bytes_min`       what an iteration must read at least: 12 B per source point and hypothesis, and every used voxel's mean and
                    Omega (72 B) once; `gather_bytes` is what the lanes ask for: 72 B per point, hypothesis and voxel searched;
  `min_GBps`        bytes_min / iter_ms;
  `kernels`         per kernel calls / average / min / max ms from a `rocprofv3 --kernel-trace --stats` run of this script with
                    --case NAME, a run of its own per case (attached afterwards: --merge ... --attach NAME=kernel_stats.csv); an
                    iteration is one ndt_eval_kernel and one ndt_turn_kernel.
Prints one JSON line; --out writes it too.

    python scripts/ndt_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python scripts/ndt_timing.py --case search7_K64
    python scripts/ndt_timing.py --merge plain.json --attach search7_K64=prof/.../kernel_stats.csv --out profiles/ndt_timing.json"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


KERNELS = ("ndt_moments_kernel", "ndt_gauss_kernel", "ndt_eval_kernel", "ndt_turn_kernel")


def kernel_ms(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key in row["Name"]:
                    out[key + ("<map>" if "ILb1" in row["Name"] or "<true>" in row["Name"] else "")] = dict(
                        calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6, min_ms=float(row["MinNs"]) * 1e-6,
                        max_ms=float(row["MaxNs"]) * 1e-6)
    return out


def merge(path, attach, out):
    with open(path) as f:
        res = json.loads(f.readline())
    for item in attach or []:
        name, csv_path = item.split("=", 1)
        ks = kernel_ms(csv_path)
        row = res["cases"][name]
        row["kernels"] = ks
        row["kernel_iter_ms"] = ks["ndt_eval_kernel"]["avg_ms"] + ks["ndt_turn_kernel"]["avg_ms"]
        row["kernel_min_GBps"] = row["bytes_min"] / row["kernel_iter_ms"] * 1e-6
        row["kernel_speedup_per_iteration"] = row["host_iter_ms"] / row["kernel_iter_ms"]
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="this case only, without the host rule (for a profiled run): search<1|7>_K<1|8|64>")
    ap.add_argument("--merge", default=None, metavar="JSON", help="a result of this script to attach kernel times to (no GPU)")
    ap.add_argument("--attach", action="append", default=None, metavar="CASE=CSV", help="with --merge: a case's rocprofv3 kernel_stats.csv")
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--scan", type=int, default=65536)
    ap.add_argument("--iterations", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.attach, a.out)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, ndt, synth

    import graph_ref as gr

    scene = synth.make_scene(a.points, a.scan)
    tgt, src = np.ascontiguousarray(scene["map_xyz"], np.float32), np.ascontiguousarray(scene["scan_xyz"], np.float32)
    truth = np.asarray(scene["x_true"][:7], np.float64)
    rng = np.random.default_rng(0)
    guesses = np.array([gr.retract(truth, np.concatenate([rng.normal(0, 0.15, 3), rng.normal(0, 0.02, 3)])) for _ in range(64)])
    p = ndt.grid_for(tgt, 1.0, 1.0)
    d2 = ndt.gauss_d2(1.0)
    tmp = tempfile.mkdtemp(prefix="ndt_timing_")
    exe = os.path.join(tmp, "ndt_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                           "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "ndt_host.cpp"), "-o", exe])
    tgt.tofile(os.path.join(tmp, "target.f32"))
    src.tofile(os.path.join(tmp, "source.f32"))

    def host(search, K):
        cmd = [exe, os.path.join(tmp, "target.f32"), os.path.join(tmp, "source.f32"), os.path.join(tmp, "moments.bin")]
        cmd += [repr(float(v)) for v in p.origin] + [repr(float(p.resolution)), str(p.nx), str(p.ny), str(p.nz), str(p.min_points), repr(p.reg)]
        cmd += [str(search), repr(d2), str(a.iterations), str(K)]
        text = "\n".join(" ".join(repr(float(v)) for v in g) for g in guesses[:K]) + "\n"
        out = subprocess.run(cmd, input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        return float(out[0].split()[1]), float(out[1].split()[1]), np.array([[float(v) for v in line.split()] for line in out[2:2 + K]])

    res = dict(what="lv_ndt_build from the device map, lv_ndt_align of the scene's scan", map_points=int(len(tgt)), scan_points=int(len(src)),
               grid=f"{p.nx}x{p.ny}x{p.nz} @ 1 m", iterations=a.iterations, cases={})
    with capi.Context() as ctx:
        ctx.map_build(tgt)
        ts = []
        for _ in range(2 + a.reps):
            t0 = time.perf_counter()
            stats = ctx.ndt_build(p, None)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["build_ms"] = float(np.median(ts[2:]))
        res["stats"] = [int(v) for v in stats]
        used_voxels = int(stats[2])
        nc = p.nx * p.ny * p.nz
        for search in (1, 7):
            if a.case:   # a profiled run: the device alone
                for K in (1, 8, 64):
                    if a.case == f"search{search}_K{K}":
                        for its in (2, a.iterations):
                            for _ in range(1 + a.reps):
                                ctx.ndt_align(src, guesses[:K], max_iterations=its, search=search, d2=d2, step_tol=0.0)
                continue
            host_build_ms, host_eval_ms, hres = host(search, 8)
            if search == 1:
                m = np.fromfile(os.path.join(tmp, "moments.bin"), np.uint8)
                n = m[:4 * nc].view(np.uint32)
                S1 = m[4 * nc:28 * nc].view(np.int64)
                S2 = m[28 * nc:].view(np.int64)
                assert np.array_equal(n, ctx.ndt_fetch(capi.NDT_COUNT).ravel()) and np.array_equal(S1, ctx.ndt_fetch(capi.NDT_S1).ravel())
                assert np.array_equal(S2, ctx.ndt_fetch(capi.NDT_S2).ravel()), "the host's moments differ from the device's"
                res["host_build_ms"] = host_build_ms
            for K in (1, 8, 64):
                kw = dict(search=search, d2=d2, step_tol=0.0)
                wall = {}
                for its in (2, a.iterations):
                    ctx.ndt_align(src, guesses[:K], max_iterations=its, **kw)
                    tt = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        r, best = ctx.ndt_align(src, guesses[:K], max_iterations=its, **kw)
                        tt.append((time.perf_counter() - t0) * 1e3)
                    wall[its] = float(np.median(tt))
                kk = min(K, 8)
                dist = max(gr.distance(np.concatenate([r["t"][:kk], r["q"][:kk]], axis=1), hres[:kk, :7]), 0.0)
                assert dist <= 1e-8, f"search {search}, K {K}: the device ends {dist} from the host rule"
                assert np.array_equal(r["n_in"][:kk], hres[:kk, 8].astype(np.uint32)) and np.array_equal(r["accepted"][:kk], hres[:kk, 10].astype(np.uint32))
                iter_ms = (wall[a.iterations] - wall[2]) / (a.iterations - 2)
                bytes_min = 12 * len(src) * K + 72 * used_voxels
                row = dict(align_ms=wall[a.iterations], align_2_ms=wall[2], iter_ms=iter_ms, host_iter_ms=host_eval_ms * K,
                           speedup_per_iteration=host_eval_ms * K / iter_ms, bytes_min=bytes_min, gather_bytes=72 * len(src) * K * search,
                           min_GBps=bytes_min / iter_ms * 1e-6, pose_distance_from_host=dist, best=[int(best[0]), int(best[1])],
                           distance_from_truth=float(gr.distance(np.concatenate([r["t"], r["q"]], axis=1)[best[0]:best[0] + 1], truth[None])))
                res["cases"][f"search{search}_K{K}"] = row
                print(json.dumps({f"search{search}_K{K}": row}), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
