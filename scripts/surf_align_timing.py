"""Timing of the registration against the TSDF surface (lv_surf_align) on the volume scripts/tsdf_timing.py builds: its ten
64 x 2048 sweeps fused into the default 512 x 512 x 64 volume at 0.2 m (carve 0; S and W are 64 MB each: the gathers do not stay in
an L2).  Three sources, each from K = 1, 64 and 1024 guesses scattered round the true pose (0.05 m, 0.01 rad):
  `frame_s1`    a 640 x 480 depth frame rendered at the first pose (mesh.render_frame), every pixel (mesh.frame_points, stride 1);
  `frame_s4`    the same frame at stride 4;
  `sweep`       the first 64 x 2048 sweep itself.

The baseline is what a caller without the call pays: lv_tsdf_fetch, then the same rule on one CPU core (scripts/surf_align_host.cpp
compiles limo-velo_amd/csrc/lv_surf_align.hpp with g++ -O2).  The host evaluates the first --host-guesses guesses; their n_in must
equal the device's and their costs lie within 1e-9 relative of the device's at max_iterations = 0: the script asserts both.

Per case:
  `align_ms`        host wall time of lv_surf_align at --iterations turns with step_tol = 0 (nothing converges early), median;
  `iter_ms`         device time per turn: the difference of the wall times at --iterations and at 2 turns over the difference of
                    the counts (an evaluation launch, a turn launch, and every 8th turn one look at the count of running hypotheses);
  `host_iter_ms`    one evaluation of ONE hypothesis on the CPU core times K;
  `gather_bytes`    what the lanes ask for in a turn at least: 12 B per source point and hypothesis, and 8 corners x (S, W) x 4 B
                    for every point that is IN at the first guess (a point whose corners are read and which then fails the gate
                    is not counted: a lower bound);
  `gather_GBps`     gather_bytes / iter_ms;
  `kernels`         per kernel calls / average / min / max ms from a `rocprofv3 --kernel-trace --stats` run of this script with
                    --case NAME, a run of its own per case (attached afterwards: --merge ... --attach NAME=kernel_stats.csv); a
                    turn is one surf_align_eval_kernel and one surf_align_turn_kernel.
Prints one JSON line; --out writes it too.

    python scripts/surf_align_timing.py --sweeps /tmp/occ_sweeps.npz --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python scripts/surf_align_timing.py --sweeps /tmp/occ_sweeps.npz --case sweep_K64
    python scripts/surf_align_timing.py --merge plain.json --attach sweep_K64=prof/.../kernel_stats.csv --out profiles/surf_align_timing.json"""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

KERNELS = ("surf_align_eval_kernel", "surf_align_turn_kernel")
WIDTH, HEIGHT, FOCAL = 640, 480, 400.0
KS = (1, 64, 1024)


def kernel_ms(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key in row["Name"]:
                    out[key] = dict(calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6, min_ms=float(row["MinNs"]) * 1e-6,
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
        row["kernel_iter_ms"] = ks["surf_align_eval_kernel"]["avg_ms"] + ks["surf_align_turn_kernel"]["avg_ms"]
        row["kernel_gather_GBps"] = row["gather_bytes"] / ks["surf_align_eval_kernel"]["avg_ms"] * 1e-6
        row["kernel_speedup_per_iteration"] = row["host_iter_ms"] / row["kernel_iter_ms"]
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def quat_exp(v):
    th = float(np.linalg.norm(v))
    s = 0.5 if th < 1e-12 else np.sin(th / 2) / th
    return np.array([v[0] * s, v[1] * s, v[2] * s, np.cos(th / 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--case", default=None, help="this case only, without the host rule (for a profiled run): <frame_s1|frame_s4|sweep>_K<1|64|1024>")
    ap.add_argument("--merge", default=None, metavar="JSON", help="a result of this script to attach kernel times to (no GPU)")
    ap.add_argument("--attach", action="append", default=None, metavar="CASE=CSV", help="with --merge: a case's rocprofv3 kernel_stats.csv")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-guesses", type=int, default=2)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.attach, a.out)
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, mesh
    from limo_velo_amd.synth import quat_mul

    R0, t0 = np.asarray(sweeps[0][0], np.float32), np.asarray(sweeps[0][1], np.float32)
    Rc = (R0 @ np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)).astype(np.float32)   # camera z along the sensor's x
    rng = np.random.default_rng(0)

    def guesses_round(R, t):
        q = mesh._quat_of(R)
        out = [np.concatenate([np.asarray(t, np.float64), q])]
        for _ in range(max(KS) - 1):
            qq = quat_mul(q, quat_exp(rng.normal(0, 0.01, 3)))
            out.append(np.concatenate([np.asarray(t, np.float64) + rng.normal(0, 0.05, 3), qq / np.linalg.norm(qq)]))
        return np.array(out)

    res = dict(what="lv_surf_align", grid="512x512x64 @ 0.2 m (defaults), ten 64x2048 sweeps fused, carve 0", iterations=a.iterations, cases={})
    with capi.Context() as ctx:
        ctx.tsdf_configure()
        ctx.tsdf_integrate(sweeps)
        p = ctx.tsdf_params()
        prm = mesh.align_params_for(ctx)
        frame = mesh.render_frame(ctx, Rc, t0, FOCAL, FOCAL, (WIDTH - 1) / 2, (HEIGHT - 1) / 2, WIDTH, HEIGHT)
        sources = {"frame_s1": (mesh.frame_points(frame, 1), guesses_round(Rc, t0)), "frame_s4": (mesh.frame_points(frame, 4), guesses_round(Rc, t0)),
                   "sweep": (np.ascontiguousarray(sweeps[0][2], np.float32), guesses_round(R0, t0))}
        res["params"] = dict(max_dist=prm.max_dist, huber=prm.huber, min_weight=prm.min_weight)
        kw = dict(max_dist=prm.max_dist, huber=prm.huber, step_tol=0.0)
        if a.case:   # a profiled run: the device alone
            name, K = a.case.rsplit("_K", 1)
            src, g = sources[name]
            for its in (2, a.iterations):
                for _ in range(1 + a.reps):
                    ctx.surf_align(src, g[:int(K)], max_iterations=its, **kw)
            return
        ts = []
        for _ in range(3):
            t_0 = time.perf_counter()
            vol = ctx.tsdf_fetch()
            ts.append((time.perf_counter() - t_0) * 1e3)
        res["fetch_ms"] = float(np.median(ts))
        tmp = tempfile.mkdtemp(prefix="surf_align_timing_")
        exe = os.path.join(tmp, "surf_align_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "surf_align_host.cpp"), "-o", exe])
        with open(os.path.join(tmp, "params"), "wb") as f:
            f.write(np.array(list(p.origin) + [p.resolution], np.float32).tobytes())
            f.write(np.array([p.nx, p.ny, p.nz], np.int32).tobytes())
        vol["S"].tofile(os.path.join(tmp, "S"))
        vol["W"].tofile(os.path.join(tmp, "W"))
        for name, (src, g) in sources.items():
            src.tofile(os.path.join(tmp, name))
            hk = min(a.host_guesses, len(g))
            text = "\n".join(" ".join(repr(float(v)) for v in x) for x in g[:hk]) + "\n"
            cmd = [exe] + [os.path.join(tmp, n) for n in ("params", "S", "W", name)] + [str(prm.min_weight), repr(prm.max_dist), repr(prm.huber), str(hk)]
            out = subprocess.run(cmd, input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
            host_eval_ms = float(out[0].split()[1])
            host = np.array([[float(v) for v in line.split()] for line in out[1:1 + hk]])
            scored, _ = ctx.surf_align(src, g[:hk], max_iterations=0, **kw)
            live = scored["status"] != capi.SURF_ALIGN_NO_OVERLAP
            assert np.array_equal(host[live, 0].astype(np.uint32), scored["n_in"][live]), f"{name}: the host's n_in differ from the device's"
            rel = float(np.max(np.abs(host[live, 1] - scored["cost"][live]) / host[live, 1])) if live.any() else 0.0
            assert rel <= 1e-9, f"{name}: the device's cost is {rel} (relative) from the host rule's"
            for K in KS:
                wall = {}
                for its in (2, a.iterations):
                    ctx.surf_align(src, g[:K], max_iterations=its, **kw)
                    tt = []
                    for _ in range(a.reps):
                        t_0 = time.perf_counter()
                        r, best = ctx.surf_align(src, g[:K], max_iterations=its, **kw)
                        tt.append((time.perf_counter() - t_0) * 1e3)
                    wall[its] = float(np.median(tt))
                iter_ms = (wall[a.iterations] - wall[2]) / (a.iterations - 2)
                gather = (12.0 * len(src) + 64.0 * float(host[0, 0])) * K   # (guess 0's n_in stands for the points whose corners are read)
                row = dict(points=int(len(src)), K=K, align_ms=wall[a.iterations], align_2_ms=wall[2], iter_ms=iter_ms, host_iter_ms=host_eval_ms * K,
                           speedup_per_iteration=host_eval_ms * K / iter_ms if iter_ms > 0 else None, gather_bytes=gather,
                           gather_GBps=gather / iter_ms * 1e-6 if iter_ms > 0 else None, cost_rel_from_host=rel, n_in_guess0=int(host[0, 0]) if hk else None,
                           best=[int(best[0]), int(best[1])], accepted=int(r["accepted"][best[0]]) if best[0] >= 0 else None)
                res["cases"][f"{name}_K{K}"] = row
                print(json.dumps({f"{name}_K{K}": row}), file=sys.stderr)
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
