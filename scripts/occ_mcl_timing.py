"""Timing of the localisation's measurement update (lv_occ_mcl_weigh) on the grid scripts/occupancy_timing.py builds: its ten
64 x 2048 sweeps integrated into the default 512 x 512 x 64 grid at 0.2 m, then a planar distance field over layers 18..24 (0.4 m ..
1.8 m above the ground) and the 3-D field.  K = 4096, 65536 and 2^20 particles drawn uniformly over the field's free cells, under
B = 64, 360 and 2048 end points of the first sweep (K = 2^20 with B = 2048 is 2^31 pairs, past the call's limit of 2^30, and is
left out), with a likelihood table of 1024 entries.
  `ms`       host wall time of the whole call (poses, beams and table staged and uploaded, the kernel, scores, counts and `best`
             copied back, the stream synchronised) after a warm-up call of every shape: median, 10th and 90th percentile;
  `kernel_ms`  with --kernel-trace CSV (the kernel_trace.csv of a `rocprofv3 --kernel-trace` run of this script with --profiled):
             the kernel's own time per shape, and `call_less_kernel_ms` = the call's median less the kernel's: staging, copies,
             launch and synchronisation, the host's share;
  `sum`      the sum of the eligible scores, `eligible`, `best` and `best_score`;
  `host`     what a caller without this call pays: `fetch_ms` (lv_occ_distance_fetch, median of 5) plus
             scripts/occ_mcl_host.cpp, the same rule (lv_mcl.hpp) built with g++ -O2 on one core (median of 3 runs; one run from
             2^26 pairs up).  Its sum, eligible and best must equal the device's.
Prints one JSON line; --out writes it too.

    python scripts/occ_mcl_timing.py --sweeps /tmp/occ_sweeps.npz [--out profiles/occ_mcl_timing.json] [--kernel-trace CSV]"""
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

KS, BS = (4096, 65536, 1 << 20), (64, 360, 2048)
MAX_PAIRS = 1 << 30
FIELDS = (("planar", dict(planar=1, k_lo=18, k_hi=24)), ("3-D", dict()))
Z = 1.0   # the particles' height: layer 21 of the default grid, inside the planar band


def spread(ts):
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)), n=len(ts))


def rounds_of(K, B):
    return int(min(200, max(5, (1 << 28) // (K * B))))


PROFILED_CALLS = 11   # per shape in a --profiled run: the warm-up and ten more


def shapes():
    """(field name, B, K) in the order this script makes its calls."""
    return [(fname, B, K) for fname, _ in FIELDS for B in BS for K in KS if K * B <= MAX_PAIRS]


def kernel_ms(path):
    """Per shape, in shapes()'s order, the kernel's own time from rocprofv3's kernel_trace.csv of a --profiled run: the dispatches
    of mcl_kernel in start order are PROFILED_CALLS per shape; the first (the warm-up) is dropped."""
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if "mcl_kernel" in r["Kernel_Name"]]
    assert len(ms) == PROFILED_CALLS * len(shapes()), (len(ms), len(shapes()))
    return [spread(ms[i * PROFILED_CALLS + 1:(i + 1) * PROFILED_CALLS]) for i in range(len(shapes()))]


def host_baseline(field, table, jobs):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "occ_mcl_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "occ_mcl_host.cpp"), "-o", exe])
        s2 = np.ascontiguousarray(field["s2"], np.int32)
        planar = s2.ndim == 2
        with open(os.path.join(d, "head"), "wb") as f:
            f.write(np.array(list(field["origin"]) + [field["resolution"]], np.float32).tobytes() +
                    np.array([s2.shape[-1], s2.shape[-2], 1 if planar else s2.shape[0], int(planar)], np.int32).tobytes())
        s2.tofile(os.path.join(d, "s2"))
        np.ascontiguousarray(table, np.uint32).tofile(os.path.join(d, "table"))
        names = []
        for i, (prm, beams, poses) in enumerate(jobs):
            names.append(os.path.join(d, f"job{i}"))
            runs = 1 if len(beams) * len(poses) >= (1 << 26) else 3
            with open(names[-1], "wb") as f:
                f.write(np.array([prm.out_cost], np.uint32).tobytes() + np.array([prm.min_inside, len(beams), len(poses), runs], np.int32).tobytes() +
                        beams.tobytes() + poses.tobytes())
        return json.loads(subprocess.check_output([exe] + [os.path.join(d, n) for n in ("head", "s2", "table")] + names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--profiled", action="store_true", help="eleven calls of every shape, nothing written: the run to put under rocprofv3")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, mcl

    res = dict(what="lv_occ_mcl_weigh", grid="512x512x64 @ 0.2 m (defaults), ten 64x2048 sweeps integrated; planar field over layers 18..24, and the 3-D field",
               table="likelihood_table(0.2, sigma_hit 0.2, 0.95, 0.05, 80 m, scale 64, 1024 entries)", left_out="K = 2^20 with B = 2048: past K * B <= 2^30",
               shapes=[])
    rng = np.random.default_rng(5)
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(sweeps)
        table = mcl.likelihood_table(float(ctx.occ_params().resolution), 0.2, 0.95, 0.05, 80.0, 64.0, 1024)
        prm = capi.default_mcl_params(out_cost=int(table[-1]), min_inside=1)
        for fname, dp in FIELDS:
            ctx.occ_distance_build(capi.default_distance_params(**dp))
            field = mcl.field_of(ctx)
            fetch = []
            for _ in range(5):
                t0 = time.perf_counter()
                ctx.occ_distance_fetch(metres=False)
                fetch.append((time.perf_counter() - t0) * 1e3)
            jobs, rows = [], []
            for B in BS:
                beams = mcl.beams_from_scan(sweeps[0][2], B, 80.0)
                assert len(beams) == B
                for K in KS:
                    if K * B > MAX_PAIRS:
                        continue
                    poses = mcl.uniform_particles(ctx, K, rng, z=Z, min_clear_s2=1, field=field)

                    def call(poses=poses, beams=beams):
                        return ctx.occ_mcl_weigh(poses, beams, table, prm)

                    first = call()   # warm-up: buffers, code objects
                    if a.profiled:
                        for _ in range(PROFILED_CALLS - 1):
                            call()
                        continue
                    ts = []
                    for _ in range(rounds_of(K, B)):
                        t0 = time.perf_counter()
                        call()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    ok = first["score"] != np.uint64(capi.MCL_NO_SCORE)
                    rows.append(dict(field=fname, K=K, B=B, group=min(64, 1 << (B - 1).bit_length()), ms=spread(ts), sum=int(first["score"][ok].sum()),
                                     eligible=int(ok.sum()), best=int(first["best"][0]), best_score=int(first["best"][1])))
                    assert rows[-1]["eligible"] > 0 and rows[-1]["best"] >= 0, rows[-1]
                    jobs.append((prm, beams, poses))
            if a.profiled:
                continue
            for row, h in zip(rows, host_baseline(field, table, jobs)):
                assert all(row[k] == h[k] for k in ("sum", "eligible", "best", "best_score")), (row, h)
                row["host_ms"] = h["ms"]
            res["shapes"] += rows
            res.setdefault("host_fetch_ms", {})[fname] = spread(fetch)
    if a.profiled:
        return
    if a.kernel_trace:
        for row, k, shape in zip(res["shapes"], kernel_ms(a.kernel_trace), shapes()):
            assert (row["field"], row["B"], row["K"]) == shape
            row["kernel_ms"] = k
            row["call_less_kernel_ms"] = row["ms"]["median"] - k["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
