"""Timing of the distance field (lv_occ_distance_build) over the default 512 x 512 x 64 grid at 0.2 m after the ten sweeps of
scripts/occupancy_timing.py (64-ring x 2048 sweeps from 10 poses on the 1 M-point bench scene's surfaces).  Four cases: 3-D
unsigned untruncated, 3-D signed, max_cells = 10, and planar over all layers.  Per case:
  `ms_median`, `ms_min`  host wall time of lv_occ_distance_build (the five kernels, the stats copied back, one synchronise), over
                  --reps calls after two warm-up calls;
  `stats`         obstacles, finite values, largest finite d2_out, largest finite d2_in;
  `kernels`       per kernel calls / average / min / max ms from a `rocprofv3 --kernel-trace --stats` run of this script with
                  --case NAME, a run of its own per case (attached afterwards: --merge ... --attach NAME=kernel_stats.csv);
  `min_bytes`     per kernel the bytes it has to move at least once (each input read once, each output written once; what the
                  outward scans read again comes from the caches), and `hbm_fraction`: min_bytes / average kernel time / 8 TB/s.
`scipy_edt_ms`: scipy.ndimage.distance_transform_edt on the fetched grid's obstacle mask in the same process, where scipy is
importable (the host alternative; it does not include fetching the 64 MiB of log-odds).
Prints one JSON line; --out writes it too.

    python scripts/occ_distance_timing.py --sweeps /tmp/occ_sweeps.npz --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_signed -- python scripts/occ_distance_timing.py \
        --sweeps /tmp/occ_sweeps.npz --case signed
    python scripts/occ_distance_timing.py --merge plain.json --attach signed=prof_signed/.../kernel_stats.csv \
        --out profiles/occ_distance_timing.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12   # B/s (spec)
KERNELS = ("dist_classify_kernel", "dist_x_kernel", "dist_y_kernel", "dist_z_kernel", "dist_stats_kernel")
CASES = {
    "unsigned": dict(),
    "signed": dict(signed_field=1),
    "max_cells_10": dict(max_cells=10),
    "planar": dict(planar=1, k_lo=0, k_hi=63),
}


def kernel_ms(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key in row["Name"]:
                    out[key] = dict(calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6, min_ms=float(row["MinNs"]) * 1e-6,
                                    max_ms=float(row["MaxNs"]) * 1e-6)
    return out


def min_bytes(nx, ny, nz_grid, planar):
    """Per kernel the bytes moved at least once: 4 B per log-odds value and per field value, 4 B per bitmap word."""
    nz = 1 if planar else nz_grid
    nv, nw = nx * ny * nz, ((nx + 31) // 32) * ny * nz
    return {"dist_classify_kernel": 4 * nx * ny * nz_grid + 4 * nw, "dist_x_kernel": 4 * nw + 4 * nv, "dist_y_kernel": 8 * nv,
            "dist_z_kernel": 8 * nv + 32 * ((nv + 255) // 256), "dist_stats_kernel": 32 * ((nv + 255) // 256)}


def merge(path, attach, out):
    with open(path) as f:
        res = json.loads(f.readline())
    for item in attach or []:
        name, csv_path = item.split("=", 1)
        row = res["cases"][name]
        ks = kernel_ms(csv_path)
        row["kernels"] = ks
        row["kernels_ms_sum"] = sum(v["avg_ms"] for v in ks.values())
        row["hbm_fraction"] = {k: row["min_bytes"][k] / (v["avg_ms"] * 1e-3) / HBM_PEAK for k, v in ks.items()}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--case", default=None, choices=sorted(CASES), help="this case only (for a profiled run)")
    ap.add_argument("--attach", action="append", default=None, metavar="CASE=CSV", help="with --merge: a case's rocprofv3 kernel_stats.csv")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--merge", default=None, metavar="JSON", help="a result of this script to attach kernel times to (no GPU)")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.attach, a.out)
    import occupancy_timing

    views, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi

    res = dict(what="lv_occ_distance_build", grid="512x512x64 @ 0.2 m (defaults)", sweeps=len(views), reps=a.reps, cases={})
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(views)
        p = ctx.occ_params()
        for name, kw in CASES.items():
            if a.case and name != a.case:
                continue
            dp = capi.default_distance_params(**kw)
            for _ in range(2):   # warm-up: allocation, code objects
                st = ctx.occ_distance_build(dp)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.occ_distance_build(dp)
                ts.append((time.perf_counter() - t0) * 1e3)
            row = dict(params=kw, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)),
                       stats=[int(v) for v in st], min_bytes=min_bytes(p.nx, p.ny, p.nz, kw.get("planar", 0)))
            res["cases"][name] = row
            print(json.dumps({name: row}), file=sys.stderr)
        if not a.no_scipy and not a.case:
            try:
                import scipy
                from scipy import ndimage
            except ImportError:
                ndimage = None
            if ndimage is not None:
                L = ctx.occ_fetch()
                free = ~(L >= np.float32(p.l_occ))
                t0 = time.perf_counter()
                d = ndimage.distance_transform_edt(free)
                res["scipy_edt_ms"] = (time.perf_counter() - t0) * 1e3
                res["scipy_version"] = scipy.__version__
                ctx.occ_distance_build(capi.default_distance_params())
                s2, _ = ctx.occ_distance_fetch(metres=False)
                res["scipy_agrees"] = bool(np.array_equal(np.round(d * d).astype(np.int64), s2.astype(np.int64)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
