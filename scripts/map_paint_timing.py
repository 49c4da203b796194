"""Timing of lv_map_paint on ring scenes of 1 M and 10 M map points (synth.make_ring_scene) with 1 and 8 RGB8 views of 1920 x 1080
pixels (random images; cameras 1.6 m above the ground, looking around the scene) and the default parameters.  Per case, one
warm-up call and REPS timed calls (medians):
  `ms`         host wall time of lv_map_paint with all three outputs: the images staged (host copy into pinned memory) and
               uploaded, the five kernels, the outputs copied back;
  `seen_ms`    the same with n_seen alone copied back (rgb and depth NULL): the share of the 16 B per point of outputs;
  `upload_ms`  the same bytes copied alone from pinned host memory to the device (torch, synchronised): the upload's share;
  `seen`       points seen by at least one view.
Prints one JSON line; --out writes it too.

    python scripts/map_paint_timing.py [--out profiles/map_paint_timing.json] [--sizes 1000000,10000000]
Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python scripts/map_paint_timing.py` run."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's runtime first: tests/conftest.py)

import lvamd  # noqa: E402

lvamd.load()
from limo_velo_amd import capi, synth  # noqa: E402

REPS = 5
W, H = 1920, 1080


def look_at(t, target):
    z = np.asarray(target, np.float64) - t
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1).astype(np.float32)


def frames(n):
    rng = np.random.default_rng(17)
    out = []
    for i in range(n):
        eye = np.array([3.0, -2.0, 1.6]) + np.r_[rng.uniform(-3, 3, 2), 0.0]
        a = 2.0 * math.pi * i / max(n, 1)
        out.append(dict(R=look_at(eye, eye + [math.cos(a), math.sin(a), -0.1]), t=eye.astype(np.float32), fx=1250.0, fy=1250.0,
                        cx=959.5, cy=539.5, image=rng.integers(0, 256, (H, W, 3), dtype=np.uint8)))
    return out


def seen_only(ctx, fr, out):
    arr = (capi.LvCameraView * len(fr))()
    keep = []
    for i, f in enumerate(fr):
        arr[i], img = capi.camera_view(f)
        keep.append(img)
    ctx._check(ctx.lib.lv_map_paint(ctx.h, arr, C.c_size_t(len(fr)), C.byref(capi.default_paint_params()), None, None,
                                    out.ctypes.data_as(C.POINTER(C.c_uint8))))


def upload_ms(nbytes):
    h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d.copy_(h, non_blocking=True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        d.copy_(h, non_blocking=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1000000,10000000")
    a = ap.parse_args()
    torch.cuda.init()
    res = dict(what="lv_map_paint", image=f"{W}x{H} rgb8", reps=REPS, params="defaults", cases=[])
    for M in [int(s) for s in a.sizes.split(",")]:
        sc = synth.make_ring_scene(M, 16, 512)
        with capi.Context() as ctx:
            ctx.map_build(sc["map_xyz"])
            for nv in (1, 8):
                fr = frames(nv)
                ctx.map_paint(fr)
                ts = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    _, _, seen = ctx.map_paint(fr)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out = np.zeros(ctx.map_size(), np.uint8)
                seen_only(ctx, fr, out)
                ts2 = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    seen_only(ctx, fr, out)
                    ts2.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(out, seen)
                case = dict(map_points=M, views=nv, ms=float(np.median(ts)), ms_min=float(np.min(ts)), seen_ms=float(np.median(ts2)),
                            upload_ms=upload_ms(nv * W * H * 3), seen=int((seen > 0).sum()))
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
