"""Timing of depth fusion (lv_depth_integrate) into the default 512 x 512 x 64 volume at 0.2 m: U16 millimetre frames of a room of
12 x 12 x 3.7 m seen from its middle (a pinhole camera 1.2 m above the floor, turned by 360 / 32 degrees from frame to frame), one
frame and 32 frames of 640 x 480 (f = 525) and of 1280 x 720 (f = 910), depth 0.3..10 m, carve 0.
  `depth`   `call_ms`: host wall time of the whole call, staging and upload of the images included, median of `n` after a warm-up;
            `stats`, `box_voxels` (the voxels the launch covers), `sw_bytes` = 16 * voxels touched: S and W read and written once
            each where dW > 0, the bytes of the volume the kernel has to move; `image_bytes`: what is staged and uploaded.
  `sweep`   the route without this call: every valid pixel back-projected on the host into a return of an lv_view (`convert_ms`,
            numpy) and lv_tsdf_integrate of those views, at most 2^24 returns a call (`integrate_ms`).  It fuses another rule (rays
            walked through the band, one 64-bit atomic per cell), so its volume is not compared.
  `host`    the same rule on one CPU core: scripts/depth_host.cpp, g++ -O2, the same shortcuts; its S and W must equal the library's.
  `kernel_ms`  with --kernel-trace CSV (the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run of this script with
            --profiled): per shape the median time of depth_fuse_kernel, and `sw_gbps` = sw_bytes over it.
Prints one JSON line; --out writes it too.

    python scripts/depth_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o depth -- python scripts/depth_timing.py --profiled
    python scripts/depth_timing.py --merge plain.json --kernel-trace prof/.../depth_kernel_trace.csv --out profiles/depth_timing.json"""
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

import numpy as np  # noqa: E402

SHAPES = ((640, 480, 525.0, 1), (1280, 720, 910.0, 1), (640, 480, 525.0, 32), (1280, 720, 910.0, 32))
ROOM_LO, ROOM_HI = np.array([-6.0, -6.0, -1.2]), np.array([6.0, 6.0, 2.5])
EYE = np.array([0.3, -0.2, 0.0])
AXES = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)   # camera x, y, z as world -y, -z, +x
PROFILED_CALLS = 6   # per shape in a --profiled run: the warm-up and five more
MAX_RETURNS = 1 << 24


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def frames_of(width, height, focal, n):
    """n U16 millimetre frames of the room from EYE, frame i turned by 2 pi i / 32 about z."""
    out = []
    vv, uu = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    rays = np.stack([(uu - (width - 1) / 2) / focal, (vv - (height - 1) / 2) / focal, np.ones_like(uu, float)], -1)
    for i in range(n):
        a = 2 * np.pi * i / 32
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ AXES
        d = rays @ R.T
        with np.errstate(divide="ignore"):
            t = np.where(d > 0, (ROOM_HI - EYE) / d, np.where(d < 0, (ROOM_LO - EYE) / d, np.inf)).min(-1)   # z-depth: the rays have z = 1
        img = np.clip(np.rint(t * 1000), 0, 65535).astype(np.uint16)
        out.append(dict(R=R.astype(np.float32), t=EYE.astype(np.float32), fx=focal, fy=focal, cx=(width - 1) / 2, cy=(height - 1) / 2, depth=img,
                        depth_scale=0.001))
    return out


def sweep_views(frames, prm):
    """The frames as lv_view sweeps: every valid pixel a return (x D, y D, D) in the camera frame."""
    views = []
    for f in frames:
        img = f["depth"]
        h, w = img.shape
        D = img.astype(np.float32) * np.float32(f["depth_scale"])
        ok = (img != 0) & (D >= prm.min_depth) & (D <= prm.max_depth)
        vv, uu = np.nonzero(ok)
        Dk = D[vv, uu]
        pts = np.stack([(uu - f["cx"]) / f["fx"] * Dk, (vv - f["cy"]) / f["fy"] * Dk, Dk], axis=1).astype(np.float32)
        views.append((f["R"], f["t"], pts))
    return views


def sweep_calls(views):
    calls, cur, n = [], [], 0
    for v in views:
        if cur and (n + len(v[2]) > MAX_RETURNS or len(cur) == 32):
            calls.append(cur)
            cur, n = [], 0
        cur.append(v)
        n += len(v[2])
    return calls + [cur]


def host_baseline(p, prm, frames, S, W):
    """(the host's JSON, its S, its W) from the volume (S, W)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "depth_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "depth_host.cpp"), "-o", exe])
        with open(os.path.join(d, "params"), "wb") as f:
            f.write(np.array(list(p.origin) + [p.resolution, prm.min_depth, prm.max_depth, prm.max_norm_radius], np.float32).tobytes())
            f.write(np.array([p.nx, p.ny, p.nz, p.trunc_cells, p.max_weight, prm.carve, len(frames)], np.int32).tobytes())
        with open(os.path.join(d, "views"), "wb") as f, open(os.path.join(d, "images"), "wb") as g:
            for fr in frames:
                h, w = fr["depth"].shape
                f.write(np.concatenate([np.asarray(fr["R"], np.float32).ravel(), np.asarray(fr["t"], np.float32).ravel(),
                                        np.array([fr["fx"], fr["fy"], fr["cx"], fr["cy"]], np.float32), np.zeros(5, np.float32),
                                        np.array([fr["depth_scale"]], np.float32)]).tobytes())
                f.write(np.array([w, h, 0], np.int32).tobytes())
                g.write(np.ascontiguousarray(fr["depth"]).tobytes())
        S.tofile(os.path.join(d, "S"))
        W.tofile(os.path.join(d, "W"))
        out = json.loads(subprocess.check_output([exe] + [os.path.join(d, n) for n in ("params", "views", "images", "S", "W")]))
        return out, np.fromfile(os.path.join(d, "S"), np.int32).reshape(S.shape), np.fromfile(os.path.join(d, "W"), np.int32).reshape(W.shape)


def kernels_ms(path):
    """Per shape, in SHAPES' order, the dispatches of depth_fuse_kernel of a --profiled run without each shape's warm-up."""
    with open(path) as f:
        rows = sorted((r for r in csv.DictReader(f) if "depth_fuse_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == PROFILED_CALLS * len(SHAPES), len(rows)
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]
    return [spread(ms[s * PROFILED_CALLS + 1:(s + 1) * PROFILED_CALLS]) for s in range(len(SHAPES))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--profiled", action="store_true", help="six calls of every shape, nothing written: the run to put under rocprofv3")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--merge", default=None, help="the JSON of an earlier run of this script: nothing runs, --kernel-trace is added to it")
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            finish(json.load(f), a)
        return
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, mesh

    prm = capi.default_depth_params()
    res = dict(what="lv_depth_integrate", grid="512x512x64 @ 0.2 m (defaults)", scene="a room of 12 x 12 x 3.7 m from its middle, U16 mm", shapes=[])
    with capi.Context() as ctx:
        ctx.tsdf_configure()
        p = ctx.tsdf_params()
        for width, height, focal, n in SHAPES:
            frames = frames_of(width, height, focal, n)
            ctx.tsdf_clear()
            stats = ctx.tsdf_integrate_depth(frames, prm)   # warm-up: buffers, code objects; and the volume the host must equal
            if a.profiled:
                for _ in range(PROFILED_CALLS - 1):
                    ctx.tsdf_integrate_depth(frames, prm)
                continue
            vol = ctx.tsdf_fetch()
            ts = []
            for _ in range(20 if n == 1 else 8):
                t0 = time.perf_counter()
                ctx.tsdf_integrate_depth(frames, prm)
                ts.append((time.perf_counter() - t0) * 1e3)
            row = dict(width=width, height=height, focal=focal, frames=n, depth=dict(call_ms=spread(ts), stats=[int(x) for x in stats],
                                                                                     sw_bytes=16 * int(stats[3]), image_bytes=2 * width * height * n))
            if not a.no_host:
                h, hS, hW = host_baseline(p, prm, frames, np.zeros_like(vol["S"]), np.zeros_like(vol["W"]))
                assert np.array_equal(hS, vol["S"]) and np.array_equal(hW, vol["W"]) and h["stats"] == [int(x) for x in stats], (h["stats"], stats)
                b = h.pop("box")
                row["depth"]["box_voxels"] = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2])
                row["host"] = dict(equal_volume=True, **h)
            # the route of before: pixels to returns on the host, then the ray walk
            ctx.tsdf_clear()
            tc, ti = [], []
            for _ in range(5 if n == 1 else 2):
                t0 = time.perf_counter()
                calls = sweep_calls(sweep_views(frames, prm))
                tc.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                st = sum(mesh.integrate(ctx, c) for c in calls)
                ti.append((time.perf_counter() - t0) * 1e3)
            row["sweep"] = dict(convert_ms=spread(tc), integrate_ms=spread(ti), calls=len(calls), stats=[int(x) for x in st])
            res["shapes"].append(row)
    if a.profiled:
        return
    finish(res, a)


def finish(res, a):
    if a.kernel_trace:
        for row, k in zip(res["shapes"], kernels_ms(a.kernel_trace)):
            row["depth"]["kernel_ms"] = k
            row["depth"]["sw_gbps"] = row["depth"]["sw_bytes"] / (k["median"] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
