"""Timing of ray casting and view gain (lv_occ_raycast / lv_occ_view_gain) on the grid scripts/occupancy_timing.py builds: its ten
64 x 2048 sweeps integrated into the default 512 x 512 x 64 grid at 0.2 m.
  `raycast`    64 x 2048 rays of 80 m from the first pose (scan_pattern): `first_ms`, the call after the grid changed (it packs
               the cell states first; median of 5, the change being an lv_occ_load of the grid's own values), and `later_ms`, the
               calls after it (median of 20); host wall time of the whole call, the results copied back.
  `view_gain`  32 poses on the sweeps' circle x 16 x 360 rays of 80 m in one call: `ms`, median of 10.
  `host`       what a caller without these calls pays: `fetch_ms` (lv_occ_fetch, median of 5) plus scripts/occ_ray_host.cpp, the
               same rule (lv_ray.hpp) built with g++ -O2 on one core, for the same rays and views.
The library timed is the one capi loads (LV_LIB_PATH names another build); --label names it in the output and --merge FILE takes
over the entries of an earlier run of this script, so that two builds can stand side by side in one file.
Prints one JSON line; --out writes it too.

    python scripts/occ_ray_timing.py --sweeps /tmp/occ_sweeps.npz [--label packed] [--merge other.json] [--out profiles/occ_ray_timing.json]"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

RINGS, AZ, GAIN_VIEWS, GAIN_EL, GAIN_AZ, RANGE = 64, 2048, 32, 16, 360, 80.0


def median_ms(fn, n, before=None):
    ts = []
    for _ in range(n):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=n)


def host_baseline(p, L, frm, to, views, pattern):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "occ_ray_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "occ_ray_host.cpp"), "-o", exe])
        f32 = np.array(list(p.origin) + [p.resolution, p.min_range, p.max_range, p.l_occ, p.l_free], np.float32)
        with open(os.path.join(d, "params"), "wb") as f:
            f.write(f32.tobytes() + np.array([p.nx, p.ny, p.nz], np.int32).tobytes())
        L.tofile(os.path.join(d, "grid"))
        np.hstack([frm, to]).astype(np.float32).tofile(os.path.join(d, "rays"))
        with open(os.path.join(d, "views"), "wb") as f:
            f.write(np.array([len(views), len(pattern)], np.int32).tobytes())
            for R, t, _ in views:
                f.write(np.asarray(R, np.float32).tobytes() + np.asarray(t, np.float32).tobytes())
            f.write(np.asarray(pattern, np.float32).tobytes())
        return json.loads(subprocess.check_output([exe] + [os.path.join(d, n) for n in ("params", "grid", "rays", "views")]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--label", default="library")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the host baseline out (a second build: it is the same)")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, occupancy

    R0, t0 = sweeps[0][0], sweeps[0][1]
    to = (occupancy.scan_pattern(AZ, RINGS, math.radians(-25.0), math.radians(3.0), RANGE) @ np.asarray(R0, np.float32).T + t0).astype(np.float32)
    frm = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, np.float32), to.shape))
    pattern = occupancy.scan_pattern(GAIN_AZ, GAIN_EL, math.radians(-25.0), math.radians(3.0), RANGE)
    views = []
    for i in range(GAIN_VIEWS):
        ang = 2.0 * math.pi * i / GAIN_VIEWS
        yaw = ang + math.pi / 2
        R = np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1.0]], np.float32)
        views.append((R, np.array([3.0 + 12.0 * math.cos(ang), -2.0 + 12.0 * math.sin(ang), 1.5], np.float32), pattern))
    res = dict(what="lv_occ_raycast / lv_occ_view_gain", grid="512x512x64 @ 0.2 m (defaults), ten 64x2048 sweeps integrated",
               rays=f"{RINGS}x{AZ} x {RANGE} m from one pose", gain=f"{GAIN_VIEWS} views x {GAIN_EL}x{GAIN_AZ} x {RANGE} m", builds={})
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(sweeps)
        L = ctx.occ_fetch()
        p = ctx.occ_params()
        prm = capi.default_ray_params()
        out = ctx.occ_raycast(frm, to, prm)   # warm-up: buffers, code objects
        ctx.occ_view_gain(views[:1])
        row = dict(lib=os.path.basename(capi.LIB_PATH))
        row["raycast"] = dict(first_ms=median_ms(lambda: ctx.occ_raycast(frm, to, prm), 5, before=lambda: ctx.occ_load(L)),
                              later_ms=median_ms(lambda: ctx.occ_raycast(frm, to, prm), 20),
                              stopped=int((out["status"] == capi.LV_RAY_STOPPED).sum()), steps=int(out["steps"].sum()))
        gain = ctx.occ_view_gain(views)
        row["view_gain"] = dict(ms=median_ms(lambda: ctx.occ_view_gain(views), 10), rays_used=int(gain[:, 0].sum()), rays_stopped=int(gain[:, 1].sum()),
                                unknown=int(gain[:, 2].sum()), free=int(gain[:, 3].sum()))
        res["builds"][a.label] = row
        if not a.no_host:
            res["host"] = dict(fetch_ms=median_ms(ctx.occ_fetch, 5), **host_baseline(p, L, frm, to, views, pattern))
            assert res["host"]["stopped"] == row["raycast"]["stopped"] and res["host"]["gain_unknown"] == row["view_gain"]["unknown"]
    if a.merge:
        with open(a.merge) as f:
            old = json.load(f)
        for k, v in old["builds"].items():
            res["builds"].setdefault(k, v)
        if "host" in old:
            res.setdefault("host", old["host"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
