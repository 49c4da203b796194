"""Timing of the rolling volumes (lv_volume_recentre, lv_occ_mark) on the default 512 x 512 x 64 grid at 0.2 m, after the ten
sweeps of scripts/occupancy_timing.py have been integrated into the occupancy grid and into the TSDF volume:
  `recentre`      per volume and per shift (32, 0, 0), (1, 0, 0), (0, 32, 0), (0, 0, 8), (32, 32, 0): host wall time of
                  lv_volume_recentre in ms (the kernels and the stats copied back), the median over `reps` calls that alternate
                  +d and -d, its ratio to the plain copy of that volume's bytes, and the stats of the first call;
  `mark`          lv_occ_mark from the 1 M-point bench map (pts = NULL), whole grid, only_unknown: median ms and the stats;
  `copy_ms`       YARDSTICK, not the code under test: a plain hipMemcpyAsync device to device of the volume's bytes (64 MiB for
                  the grid, 128 MiB for S and W), median of `reps`, and the GB/s it moves (read + write);
  `round_trip_ms` YARDSTICK: the only route before lv_volume_recentre: lv_occ_fetch, the shift in numpy, lv_occ_configure,
                  lv_occ_load (median of 3; `round_trip_ms_all` the three).
Prints one JSON line; --out writes it too.  --sweeps FILE as scripts/occupancy_timing.py (--prepare casts them without a GPU).

    python scripts/occ_recentre_timing.py --sweeps /tmp/occ_sweeps.npz [--out profiles/occ_recentre_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

import occupancy_timing as ot  # noqa: E402

SHIFTS = [(32, 0, 0), (1, 0, 0), (0, 32, 0), (0, 0, 8), (32, 32, 0)]
REPS = 11
M = 1_000_000


def copy_ms(n_bytes, reps=REPS):
    """Median ms of hipMemcpyAsync(device to device) of n_bytes on the null stream, each waited for."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    a, b = C.c_void_p(), C.c_void_p()
    if hip.hipMalloc(C.byref(a), n_bytes) or hip.hipMalloc(C.byref(b), n_bytes):
        raise RuntimeError("hipMalloc failed")
    hip.hipMemset(a, 1, n_bytes)
    hip.hipMemset(b, 0, n_bytes)
    hip.hipDeviceSynchronize()
    ts = []
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        rc = hip.hipMemcpyAsync(b, a, n_bytes, 3, None)   # hipMemcpyDeviceToDevice
        rc = rc or hip.hipDeviceSynchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        if rc:
            raise RuntimeError("hipMemcpyAsync failed: %d" % rc)
    hip.hipFree(a)
    hip.hipFree(b)
    return float(np.median(ts[2:]))   # (the first two warm the path up)


def time_recentre(ctx, volume, d, reps=REPS):
    ts, first = [], None
    for r in range(reps):
        s = d if r % 2 == 0 else tuple(-v for v in d)
        t0 = time.perf_counter()
        st = ctx.volume_recentre(volume, s)
        ts.append((time.perf_counter() - t0) * 1e3)
        if first is None:
            first = [int(v) for v in st]
    ctx.volume_recentre(volume, tuple(-v for v in d))   # (an odd number of calls: back to where it started)
    return float(np.median(ts)), first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--prepare", action="store_true", help="cast and save the sweeps only (no GPU)")
    a = ap.parse_args()
    views, _ = ot.make_sweeps(a.sweeps, count_visits=False)
    if a.prepare:
        return
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, synth

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import recentre_ref as rr

    res = dict(what="lv_volume_recentre / lv_occ_mark", grid="512x512x64 @ 0.2 m (defaults)", reps=REPS, recentre={}, map_points=M)
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.tsdf_configure()
        ctx.occ_integrate(views)
        ctx.tsdf_integrate(views)
        n_vox = 512 * 512 * 64
        res["copy_ms"] = dict(grid=copy_ms(4 * n_vox), surface=copy_ms(8 * n_vox))
        res["copy_GBps"] = {k: 2 * b / (v * 1e-3) / 1e9 for (k, v), b in zip(res["copy_ms"].items(), (4 * n_vox, 8 * n_vox))}
        for name, volume in (("grid", capi.LV_VOLUME_OCC), ("surface", capi.LV_VOLUME_SURFACE)):
            ctx.volume_recentre(volume, (1, 1, 1))    # warm-up (the second buffer, code objects)
            ctx.volume_recentre(volume, (-1, -1, -1))
            rows = {}
            for d in SHIFTS:
                ms, st = time_recentre(ctx, volume, d)
                rows["%d,%d,%d" % d] = dict(ms=ms, ratio_to_copy=ms / res["copy_ms"][name], kept=st[0], exposed=st[1], left=st[2])
                print(name, d, json.dumps(rows["%d,%d,%d" % d]), file=sys.stderr)
            res["recentre"][name] = rows
        # the grid scrolls into ground the point map knows: mark from the 1 M-point bench map
        ctx.map_build(synth.make_scene(M, 2_000)["map_xyz"])
        L = ctx.occ_fetch()
        ts = []
        for _ in range(5):
            ctx.occ_load(L)
            t0 = time.perf_counter()
            st = ctx.occ_mark()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["mark"] = dict(ms=float(np.median(ts)), points_used=int(st[0]), candidates=int(st[1]), marked=int(st[2]), observed=int(st[3]))
        # the route without lv_volume_recentre: over PCIe twice, and every snapshot freed
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            p = ctx.occ_params()
            moved = rr.shift_logodds(ctx.occ_fetch(), (32, 0, 0))
            p.origin[0] = float(np.float32(p.origin[0]) + np.float32(32) * np.float32(p.resolution))
            ctx.occ_configure(p)
            ctx.occ_load(moved)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["round_trip_ms"] = float(np.median(ts))
        res["round_trip_ms_all"] = [float(t) for t in ts]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
