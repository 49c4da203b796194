"""Timing of lv_occ_from_surface on the default 512 x 512 x 64 grid and the default volume of the same footprint (0.2 m), after the ten
64 x 2048 sweeps of scripts/tsdf_timing.py have been fused into the volume:
  `cases`   mode REPLACE over the whole grid with reach 0, 1 and 4, and mode FILL over one exposed strip of 32 voxels across x
            (what a recentre by 32 leaves), each from a cleared grid: `call_ms` the host wall time of the whole call (median of `n`
            after a warm-up), `stats`, and `grid_bytes` = 4 bytes read per voxel of the box + 4 written per voxel changed.
  `host`    the route without this call, per reach: lv_tsdf_fetch of S and W (`fetch_ms`), the rule in numpy
            (tests/surf_occ_ref.py, `rule_ms`), lv_occ_load (`load_ms`); the grid it leaves must equal the call's bit for bit.
  `copy`    the floor: a plain device-to-device copy of the grid's 64 MiB (torch), `copy_ms`.
  `kernel_ms`  with --kernel-trace CSV (the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run of this script with
            --profiled): per case the median over its calls of the summed time of the call's surf_occ_* kernels, and per kernel.
Prints one JSON line; --out writes it too.

    python scripts/surf_occ_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o surf_occ -- python scripts/surf_occ_timing.py --profiled
    python scripts/surf_occ_timing.py --merge plain.json --kernel-trace prof/.../surf_occ_kernel_trace.csv --out profiles/surf_occ_timing.json"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

REPLACE, FILL = 2, 0
STRIP = ((480, 0, 0), (511, 511, 63))
CASES = (dict(name="replace_reach0", mode=REPLACE, reach=0), dict(name="replace_reach1", mode=REPLACE, reach=1),
         dict(name="replace_reach4", mode=REPLACE, reach=4), dict(name="fill_strip32", mode=FILL, reach=1, lo=STRIP[0], hi=STRIP[1]))
PROFILED_CALLS = 6   # per case in a --profiled run: the warm-up and five more
REPS = 20


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def kernels_of(case):
    return 5 if case["reach"] else 2   # classify, (grow x, y, z), write


def kernels_ms(path):
    """Per case, in CASES' order: the summed time of one call's kernels (median over the calls behind the warm-up), and per kernel."""
    with open(path) as f:
        rows = sorted((r for r in csv.DictReader(f) if "surf_occ_" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == PROFILED_CALLS * sum(kernels_of(c) for c in CASES), len(rows)
    out, at = [], 0
    for c in CASES:
        k = kernels_of(c)
        calls = [rows[at + i * k:at + (i + 1) * k] for i in range(PROFILED_CALLS)][1:]
        at += PROFILED_CALLS * k
        ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        per = {}
        for call in calls:
            for r in call:
                per.setdefault(re.search(r"surf_occ_\w+", r["Kernel_Name"]).group(0), []).append(ms(r))
        out.append(dict(call=spread([sum(ms(r) for r in call) for call in calls]),
                        kernels={n: dict(median_ms=float(np.median(v)), per_call=len(v) // len(calls)) for n, v in per.items()}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--profiled", action="store_true", help="six calls of every case, nothing written: the run to put under rocprofv3")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--merge", default=None, help="the JSON of an earlier run of this script: nothing runs, --kernel-trace is added to it")
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            finish(json.load(f), a)
        return
    torch = None
    if not a.profiled:
        try:
            import torch   # (before the library: its runtime has to come first)

            torch.cuda.init()
        except Exception:
            torch = None
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(None, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi
    import surf_occ_ref as sr

    res = dict(what="lv_occ_from_surface", grid="512x512x64 @ 0.2 m (defaults)", volume="the same footprint, trunc_cells 3, ten 64x2048 sweeps fused",
               cases=[], host=[])
    with capi.Context() as ctx:
        ctx.tsdf_configure()
        ctx.tsdf_integrate(sweeps)
        ctx.occ_configure()
        op, tp = ctx.occ_params(), ctx.tsdf_params()
        shape = (op.nz, op.ny, op.nx)
        grids = {}
        for c in CASES:
            kw = {k: v for k, v in c.items() if k != "name"}
            prm = capi.default_occ_surface_params(**kw)
            ctx.occ_clear()
            stats = ctx.occ_from_surface(prm)   # warm-up: the bitmaps, code objects
            if a.profiled:
                for _ in range(PROFILED_CALLS - 1):
                    ctx.occ_clear()
                    ctx.occ_from_surface(prm)
                continue
            grids[c["name"]] = ctx.occ_fetch()
            ts = []
            for _ in range(REPS):
                ctx.occ_clear()
                t0 = time.perf_counter()
                ctx.occ_from_surface(prm)
                ts.append((time.perf_counter() - t0) * 1e3)
            lo, hi = c.get("lo", (0, 0, 0)), c.get("hi", (op.nx - 1, op.ny - 1, op.nz - 1))
            box = int(np.prod([h - l + 1 for l, h in zip(lo, hi)]))
            res["cases"].append(dict(name=c["name"], mode=c["mode"], reach=c["reach"], box_voxels=box, call_ms=spread(ts), stats=[int(x) for x in stats],
                                     grid_bytes=4 * box + 4 * int(stats[2])))
        if a.profiled:
            return
        if not a.no_host:
            grid = sr.geometry(list(op.origin), op.resolution, shape)
            vol = sr.geometry(list(tp.origin), tp.resolution, (tp.nz, tp.ny, tp.nx))
            for c in CASES[:3]:
                t0 = time.perf_counter()
                v = ctx.tsdf_fetch()
                t1 = time.perf_counter()
                L, st = sr.from_surface(np.full(shape, sr.NAN_BITS.view(np.float32), np.float32), grid, vol, v["S"], v["W"], op.l_min, op.l_max, mode=c["mode"],
                                        reach=c["reach"])
                t2 = time.perf_counter()
                ctx.occ_load(L)
                t3 = time.perf_counter()
                equal = bool(np.array_equal(L.view(np.uint32), grids[c["name"]].view(np.uint32)))
                assert equal, c["name"]
                res["host"].append(dict(name=c["name"], fetch_ms=(t1 - t0) * 1e3, rule_ms=(t2 - t1) * 1e3, load_ms=(t3 - t2) * 1e3, equal_grid=equal,
                                        stats=[int(x) for x in st]))
    if torch is not None and torch.cuda.is_available():
        n = shape[0] * shape[1] * shape[2]
        src, dst = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
        dst.copy_(src)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["copy"] = dict(bytes=4 * n, copy_ms=spread(ts))
    finish(res, a)


def finish(res, a):
    if a.kernel_trace:
        for row, k in zip(res["cases"], kernels_ms(a.kernel_trace)):
            row["kernel_ms"] = k
            row["grid_gbps"] = row["grid_bytes"] / (k["call"]["median"] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
