"""Timing of one localisation cycle with the particles resident on the device (mcl.DeviceFilter.step: lv_occ_mcl_filter_move, _weigh
and _resample with mode 1, nothing of size K leaving the device) against the same cycle on the host round lv_occ_mcl_weigh (mcl.step:
numpy move, the upload of every pose, the download of every score, numpy resampling), on the planar field of scripts/occ_mcl_timing.py:
ten 64 x 2048 sweeps integrated into the default 512 x 512 x 64 grid at 0.2 m, the field over layers 18..24.  K = 4096, 65536 and 2^20
particles drawn uniformly over the field's free cells, B = 64 and 360 end points of the first sweep.
  `filter_ms`, `step_ms`   host wall time of one cycle that ends in lv_synchronize, the two alternated cycle by cycle in the same run
                           after a warm-up cycle of each: median, 10th and 90th percentile.  Both filters go on from their own
                           particles, so the cycles are those of a running filter (resamplings included: `resampled` counts them);
  `filter_back_to_back_ms` the resident cycle again, the same number of cycles with no host cycle between them;
  `kernels_ms`             with --kernel-trace CSV (the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run of this script
                           with --profiled): per shape the median time of each of the filter's kernels.
Prints one JSON line; --out writes it too.

    python scripts/occ_mcl_filter_timing.py [--sweeps /tmp/occ_sweeps.npz] [--out profiles/occ_mcl_filter_timing.json] [--kernel-trace CSV]"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

KS, BS = (4096, 65536, 1 << 20), (64, 360)
DP = dict(planar=1, k_lo=18, k_hi=24)
Z = 1.0
DELTA, ALPHAS = (0.05, 0.3, 0.02), (0.02, 0.02, 0.02, 0.02)
PROFILED_CYCLES = 11   # per shape in a --profiled run: the warm-up and ten more
KERNELS = ("mclf_move_kernel", "mclf_weigh_kernel", "mclf_weights_kernel", "mclf_scan_kernel", "mclf_gather_kernel")


def spread(ts):
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)), n=len(ts))


def rounds_of(K):
    return 40 if K <= 65536 else 12


def shapes():
    return [(B, K) for B in BS for K in KS]


def kernels_ms(path):
    """Per shape, in shapes()'s order, the median time of each of the filter's kernels from a --profiled run: mclf_move_kernel runs
    once per cycle, so its dispatches in start order delimit the shapes; the warm-up cycle of each shape is dropped."""
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out, cycle = [dict((k, []) for k in KERNELS) for _ in shapes()], -1
    for r in rows:
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name is None:
            continue
        if name == "mclf_move_kernel":
            cycle += 1
        if cycle % PROFILED_CYCLES:
            out[cycle // PROFILED_CYCLES][name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    assert cycle + 1 == PROFILED_CYCLES * len(shapes()), cycle
    return [{k: dict(median=float(np.median(v)), n=len(v)) for k, v in s.items() if v} for s in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--profiled", action="store_true", help="eleven filter cycles of every shape, nothing written: the run to put under rocprofv3")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, mcl

    res = dict(what="one cycle: mcl.DeviceFilter.step (fetch=False) against mcl.step",
               grid="512x512x64 @ 0.2 m (defaults), ten 64x2048 sweeps integrated; planar field over layers 18..24",
               tables="likelihood_table(0.2, sigma_hit 0.2, 0.95, 0.05, 80 m, scale 64, 1024 entries); weight_table(64, 4, 4096)", shapes=[])
    rng = np.random.default_rng(5)
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(sweeps)
        ctx.occ_distance_build(capi.default_distance_params(**DP))
        field = mcl.field_of(ctx)
        table = mcl.likelihood_table(float(ctx.occ_params().resolution), 0.2, 0.95, 0.05, 80.0, 64.0, 1024)
        wtable = mcl.weight_table(64.0, 4.0, 4096)
        for B, K in shapes():
            beams = mcl.beams_from_scan(sweeps[0][2], B, 80.0)
            assert len(beams) == B
            p0 = mcl.uniform_particles(ctx, K, rng, z=Z, min_clear_s2=1, field=field)
            filt = mcl.DeviceFilter(ctx, p0, 1)

            def device_cycle():
                s = filt.step(DELTA, beams, table, wtable, alphas=ALPHAS, fetch=False)
                ctx.synchronize()
                return s

            device_cycle()   # warm-up: buffers, code objects
            if a.profiled:
                for _ in range(PROFILED_CYCLES - 1):
                    device_cycle()
                continue
            host = dict(poses=p0, acc=np.zeros(K, np.uint64))

            def host_cycle():
                s = mcl.step(ctx, host["poses"], host["acc"], DELTA, beams, table, wtable, rng, alphas=ALPHAS)
                ctx.synchronize()
                host.update(poses=s["poses"], acc=s["acc"])
                return s

            host_cycle()
            td, th, nd, nh = [], [], 0, 0
            for _ in range(rounds_of(K)):
                t0 = time.perf_counter()
                s = device_cycle()
                td.append((time.perf_counter() - t0) * 1e3)
                nd += int(s["resampled"])
                t0 = time.perf_counter()
                s = host_cycle()
                th.append((time.perf_counter() - t0) * 1e3)
                nh += int(s["resampled"])
            tb = []
            for _ in range(rounds_of(K)):   # the resident cycle back to back, as a running loop sees it
                t0 = time.perf_counter()
                device_cycle()
                tb.append((time.perf_counter() - t0) * 1e3)
            res["shapes"].append(dict(K=K, B=B, filter_ms=spread(td), step_ms=spread(th), filter_back_to_back_ms=spread(tb), filter_resampled=nd,
                                      step_resampled=nh))
    if a.profiled:
        return
    if a.kernel_trace:
        for row, k in zip(res["shapes"], kernels_ms(a.kernel_trace)):
            row["kernels_ms"] = k
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
