"""Timing of the device trajectory (lv_traj_register, lv_traj_register_cloud, lv_traj_smooth): 2^24 points against 2^16 knots,
time-sorted and shuffled, with the tile route on and off ("traj_tile"); 2^20 knots smoothed; against the same rule on one CPU core
(scripts/traj_host.cpp, g++ -O2), whose outputs must agree: two f32 values that each lie within half an ulp of f64 values 1e-9 apart
differ by at most one f32 ulp + 1e-9 * max(1, |x|); f64 knots by 1e-9 * max(1, |x|).

Per register case: `call_ms` (host arrays in, points and status out: the whole call), `count_only_ms` (the same call with out and
status NULL: staging, upload and kernel, no download), `stats`.  With the kernel time of the profiled run attached, the split is
`staging_upload_ms` = count_only - kernel, `kernel_ms`, `download_ms` = call - count_only.  A call on host arrays is bound by its
transfers and the host's staging copy, not by the kernel; `register_cloud` is the route without the upload (2^22 points ingested
into the device LiDAR buffer, registered from there; its `download_ms` is measured the same way).

Kernel times come from a `rocprofv3 --kernel-trace` run of its own (--profile: every case once, nothing else), attached with --merge.
Every step under its own timeout, chained:

    g++ -O2 -std=c++17 -ffp-contract=off -Itests/emu -Ilimo-velo_amd/csrc scripts/traj_host.cpp -o scripts/traj_host &&
    timeout -k 10 400 python scripts/traj_timing.py --out plain.json &&
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python scripts/traj_timing.py --profile &&
    timeout -k 10 60 python scripts/traj_timing.py --merge plain.json --attach prof --out profiles/traj_timing.json"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_POINTS, N_KNOTS, N_SMOOTH, N_CLOUD = 1 << 24, 1 << 16, 1 << 20, 1 << 22
SMOOTH = dict(sigma=0.02, half_window=8, iterations=2, pin_ends=1)
CASES = (("sorted_tile", False, 1), ("sorted_search", False, 0), ("shuffled_tile", True, 1), ("shuffled_search", True, 0))
CHUNK = 1 << 22          # TRAJ_CHUNK of lv_traj.hpp: launches per register call = N_POINTS / CHUNK
HOST = os.path.join(ROOT, "scripts", "traj_host")
KNOT_DTYPE = np.dtype([("time", "f8"), ("t", "f8", 3), ("q", "f8", 4)])
POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("pad_", "f4"), ("time", "f8"), ("intensity", "f4"), ("range", "f4")])


def make_knots(n, dt):
    """a drive along a wavy path, turning; stamps from the Unix epoch"""
    t = np.arange(n) * dt
    k = np.zeros(n, KNOT_DTYPE)
    k["time"] = 1_700_000_000.0 + t
    k["t"] = np.stack([2.0 * t + 3.0 * np.sin(0.7 * t), 2.0 * np.cos(0.5 * t), 0.5 * np.sin(0.9 * t)], axis=1)
    v = np.stack([0.3 * np.sin(0.8 * t), 0.2 * np.cos(0.6 * t), 0.9 * t], axis=1)
    th = np.linalg.norm(v, axis=1)
    k["q"][:, :3] = v * (np.sin(0.5 * th) / np.maximum(th, 1e-300))[:, None]
    k["q"][:, 3] = np.cos(0.5 * th)
    return k


def make_points(knots, m, seed=1):
    rng = np.random.default_rng(seed)
    p = np.zeros(m, POINT_DTYPE)
    xyz = rng.uniform(-50, 50, (m, 3)).astype(np.float32)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["time"] = np.sort(rng.uniform(knots["time"][0], knots["time"][-1], m))
    return p


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, spread(ts)


def host(args, tmp, arrays):
    paths = []
    for name, a in arrays:
        paths.append(os.path.join(tmp, name))
        np.ascontiguousarray(a).tofile(paths[-1])
    return paths


def dispatches(prof_dir):
    """[(kernel name, ms)] of the profiled run in dispatch order"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one kernel_trace.csv under {prof_dir}, found {files}")
    rows = []
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    rows.sort()
    return [(n, ms) for _, n, ms in rows]


def ingest_cloud(ctx, capi, pts):
    """pts (POINT_DTYPE, time-sorted) into the device LiDAR buffer, 2^20 points a message"""
    fmt = capi.CloudFormat(32, 0, 4, 8, 16, 1, 24, 1, 0, 0, 0)   # the records as they are: x y z f32, f64 stamp at 16, f32 intensity at 24
    ctx.cloud_clear(float("inf"))
    ctx.cloud_reserve(1 << 20, 32, len(pts))
    for off in range(0, len(pts), 1 << 20):
        piece = pts[off:off + (1 << 20)]
        kept = ctx.cloud_ingest(piece.tobytes(), len(piece), fmt, capi.IngestParams(0, 0, 0, 0.1, 1, 0.0))
        assert kept == len(piece), (kept, len(piece))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="every case once and nothing else (for the rocprofv3 run)")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--attach", default=None, metavar="PROF_DIR")
    ap.add_argument("--small", action="store_true", help="a sixteenth of every size (a dry run)")
    a = ap.parse_args()
    n_points, n_knots, n_smooth, n_cloud = (N_POINTS, N_KNOTS, N_SMOOTH, N_CLOUD) if not a.small else (N_POINTS >> 4, N_KNOTS >> 4, N_SMOOTH >> 4, N_CLOUD >> 4)
    launches = max(n_points // CHUNK, 1)
    if a.merge:
        with open(a.merge) as f:
            res = json.loads(f.readline())
        d = dispatches(a.attach)
        reg = [ms for n, ms in d if "traj_register_kernel" in n]
        smo = [ms for n, ms in d if "traj_smooth_kernel" in n]
        cl = max(res["sizes"]["cloud_points"] // CHUNK, 1)
        assert len(reg) == launches * len(CASES) + cl and len(smo) == SMOOTH["iterations"], (len(reg), len(smo))
        for k, (name, _, _) in enumerate(CASES):
            row = res["register"][name]
            row["kernel_ms"] = float(sum(reg[k * launches:(k + 1) * launches]))
            row["staging_upload_ms"] = row["count_only_ms"]["median"] - row["kernel_ms"]
            row["download_ms"] = row["call_ms"]["median"] - row["count_only_ms"]["median"]
            row["kernel_points_per_s"] = res["sizes"]["points"] / (row["kernel_ms"] * 1e-3)
            row["kernel_GB_per_s_at_33B"] = 33.0 * res["sizes"]["points"] / (row["kernel_ms"] * 1e-3) * 1e-9
        row = res["register_cloud"]
        row["kernel_ms"] = float(sum(reg[-cl:]))
        row["download_ms"] = row["call_ms"]["median"] - row["kernel_ms"]
        res["smooth"]["kernel_ms"] = float(sum(smo))
        res["smooth"]["kernel_ms_per_iteration"] = float(sum(smo)) / len(smo)
    else:
        import lvamd

        lvamd.load()
        from limo_velo_amd import capi

        knots = make_knots(n_knots, 1.0 / 64)
        pts = make_points(knots, n_points)
        perm = np.random.default_rng(2).permutation(n_points)
        shuffled = pts[perm]
        sknots = make_knots(n_smooth, 1.0 / 256)
        ctx = capi.Context()
        ctx.traj_set(knots)
        res = dict(what="lv_traj_register / lv_traj_register_cloud / lv_traj_smooth", reps=a.reps, smooth_params=SMOOTH,
                   sizes=dict(points=n_points, knots=n_knots, smooth_knots=n_smooth, cloud_points=n_cloud), register={})
        outs = {}
        for name, shuf, tile in CASES:
            src = shuffled if shuf else pts
            ctx.set_option("traj_tile", tile)
            if a.profile:
                ctx.traj_register(src, want_points=False, want_status=False)
                continue
            ctx.traj_register(src)   # warm-up: allocation, code objects
            (out, st, stats), call = timed(lambda: ctx.traj_register(src), a.reps)
            _, count_only = timed(lambda: ctx.traj_register(src, want_points=False, want_status=False), a.reps)
            outs[name] = out
            res["register"][name] = dict(call_ms=call, count_only_ms=count_only, stats=stats, launches=launches)
            print(json.dumps({name: res["register"][name]}), file=sys.stderr)
        ctx.set_option("traj_tile", 1)
        # the route without the upload
        ingest_cloud(ctx, capi, pts[:n_cloud])
        t1, t2 = float("-inf"), float("inf")
        if a.profile:
            ctx.traj_register_cloud(t1, t2)
        else:
            ctx.traj_register_cloud(t1, t2)
            (cout, cst, cstats), call = timed(lambda: ctx.traj_register_cloud(t1, t2), a.reps)
            assert np.array_equal(cout.view(np.uint32), outs["sorted_tile"][:n_cloud].view(np.uint32))   # the same bits as from host arrays
            res["register_cloud"] = dict(call_ms=call, stats=cstats, points=n_cloud, note="two calls inside: the first sizes the output")
        ctx.cloud_clear(float("inf"))
        # smoothing
        ctx.traj_set(sknots)
        if a.profile:
            ctx.traj_smooth(**SMOOTH)
        else:
            ctx.traj_smooth(**SMOOTH)
            ts = []
            for _ in range(a.reps):
                ctx.traj_set(sknots)
                t0 = time.perf_counter()
                ctx.traj_smooth(**SMOOTH)
                ts.append((time.perf_counter() - t0) * 1e3)
            smoothed = ctx.traj_fetch()
            res["smooth"] = dict(call_ms=spread(ts), ms_per_iteration=float(np.median(ts)) / SMOOTH["iterations"])
        ctx.close()
        if not a.profile:
            # the yardstick, and the outputs held against each other
            assert np.array_equal(outs["sorted_tile"].view(np.uint32), outs["sorted_search"].view(np.uint32))
            assert np.array_equal(outs["shuffled_tile"].view(np.uint32), outs["shuffled_search"].view(np.uint32))
            assert np.array_equal(outs["shuffled_tile"].view(np.uint32), outs["sorted_tile"][perm].view(np.uint32))
            with tempfile.TemporaryDirectory() as tmp:
                xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)
                kp, xp, tp = host(a, tmp, (("knots.bin", knots), ("xyz.bin", xyz), ("times.bin", pts["time"])))
                op = os.path.join(tmp, "out.bin")
                cpu = json.loads(subprocess.check_output(["taskset", "-c", "0", HOST, "register", kp, xp, tp, op]))
                want = np.fromfile(op, np.float32).reshape(-1, 3)
                got = outs["sorted_tile"]
                bound = np.spacing(np.abs(want)).astype(np.float64) + 1e-9 * np.maximum(1.0, np.abs(want))
                worst = float((np.abs(got.astype(np.float64) - want) / bound).max())
                assert worst <= 1.0, worst
                res["register_cpu"] = dict(ms=cpu["ms"], method="scripts/traj_host.cpp, g++ -O2, one core", worst_difference_over_bound=worst,
                                           identical_fraction=float(np.mean(got.view(np.uint32) == want.view(np.uint32))))
                sp, = host(a, tmp, (("sknots.bin", sknots),))
                cpu = json.loads(subprocess.check_output(["taskset", "-c", "0", HOST, "smooth", sp, repr(SMOOTH["sigma"]), str(SMOOTH["half_window"]),
                                                          str(SMOOTH["iterations"]), op]))
                want = np.fromfile(op, KNOT_DTYPE)
                worst = 0.0
                sg = np.where(np.sum(want["q"] * smoothed["q"], axis=1) < 0, -1.0, 1.0)[:, None]
                for g, w in ((smoothed["t"], want["t"]), (sg * smoothed["q"], want["q"])):
                    worst = max(worst, float((np.abs(g - w) / (1e-9 * np.maximum(1.0, np.abs(w)))).max()))
                assert worst <= 1.0 and np.array_equal(smoothed["time"], want["time"]), worst
                res["smooth_cpu"] = dict(ms=cpu["ms"], ms_per_iteration=cpu["ms"] / SMOOTH["iterations"], method="scripts/traj_host.cpp, g++ -O2, one core",
                                         worst_difference_over_bound=worst)
            for name in res["register"]:
                res["register"][name]["cpu_over_call"] = res["register_cpu"]["ms"] / res["register"][name]["call_ms"]["median"]
            res["smooth"]["cpu_over_call"] = res["smooth_cpu"]["ms"] / res["smooth"]["call_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
