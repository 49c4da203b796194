"""Timing of lv_map_remove_dynamic on ring scenes of 1 M and 10 M map points (synth.make_ring_scene, plus 3 000 "ghost" points the
views do not see), with 1 and 8 views of a 64 x 2048 ring sweep (synth.ring_sweep, ~131 k returns each) and the default
parameters.  Three calls per case, each warmed and then timed REPS times (medians):
  `classify`  dry_run, hits NULL: image build + window-min + classification, nothing copied back but the counters;
  `hits`      dry_run with the hit counts copied back (the rank scan of QueryStore is skipped: no id is dead);
  `remove`    min_hits 1 on a map rebuilt before every rep (untimed): the same plus the dead list and MapStore::kill_dead_list.
`ms` = host wall time of the call (perf_counter); `event_ms` = HIP events on the context's stream around it.  Both include the
staging of the returns (host packing + one copy).  Prints one JSON line.

    python scripts/map_visibility_timing.py [--out profiles/map_visibility_timing.json] [--sizes 1000000,10000000]
Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python scripts/map_visibility_timing.py` run."""
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


def views_of(states, rects):
    out = []
    for i, s in enumerate(states):
        R, t = capi.sensor_pose(s)
        out.append((R, t, synth.ring_sweep(rects, R, t, 64, 2048, (-25.0, 3.0), range_sigma=0.01, seed=300 + i)))
    return out


def raw(ctx, views, prm, hits):
    arr = (capi.View * len(views))()
    keep = []
    for i, (R, t, pts) in enumerate(views):
        a = np.ascontiguousarray(pts, np.float32)
        keep.append(a)
        arr[i].R[:] = [float(v) for v in R.ravel()]
        arr[i].t[:] = [float(v) for v in t.ravel()]
        arr[i].points, arr[i].stride, arr[i].n = a.ctypes.data, 12, len(a)
    nr = C.c_size_t(0)
    hp = hits.ctypes.data_as(C.POINTER(C.c_uint8)) if hits is not None else None
    ctx._check(ctx.lib.lv_map_remove_dynamic(ctx.h, arr, C.c_size_t(len(views)), C.byref(prm), hp, C.byref(nr)))
    return int(nr.value)


def timed(fn, stream, prep=None):
    if prep:
        prep()
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall, ev, out = [], [], None
    for _ in range(REPS):
        if prep:
            prep()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record(stream)
        out = fn()
        e.record(stream)
        e.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(s.elapsed_time(e))
    return float(np.median(wall)), float(np.median(ev)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1000000,10000000")
    a = ap.parse_args()
    torch.cuda.init()
    res = {"reps": REPS, "image": "64 x 2048, -25..+3 deg, window 1", "timing": "medians: ms = host wall time, event_ms = HIP events on the context stream"}
    for M in (int(v) for v in a.sizes.split(",")):
        sc = synth.make_ring_scene(M, 16, 512)
        rects = synth.scene_surfaces(M)
        rng = np.random.default_rng(4)
        x0 = np.array(sc["x_true"], np.float64)
        states = [x0]
        for _ in range(7):
            x = x0.copy()
            x[:2] += rng.uniform(-8, 8, 2)
            x[3:7] = synth.quat_mul(x[3:7], synth.quat_from_rpy(0.0, 0.0, math.radians(rng.uniform(-180, 180))))
            states.append(x)
        all_views = views_of(states, rects)
        ghosts = (rng.uniform(-1, 1, (3000, 3)) * [1.0, 0.6, 0.6] + [-2.5, 7.5, 1.0]).astype(np.float32)
        mp = np.concatenate([sc["map_xyz"], ghosts])
        with capi.Context() as ctx:
            ptr = ctx.get_stream()
            st = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.current_stream()
            for nv in (1, 8):
                views = all_views[:nv]
                key = f"map{M // 1000000}M_views{nv}"
                r = {"map_points": len(mp), "returns": int(sum(len(v[2]) for v in views)),
                     "orig_bytes": len(mp) * 16, "byte_bound_us_at_6TBps": len(mp) * 16 / 6e12 * 1e6}
                ctx.map_build(mp)
                dry = capi.default_visibility_params(dry_run=1)
                ms, ev, _ = timed(lambda: raw(ctx, views, dry, None), st)
                r["classify"] = {"ms": ms, "event_ms": ev}
                hits = np.zeros(len(mp), np.uint8)
                ms, ev, _ = timed(lambda: raw(ctx, views, dry, hits), st)
                r["hits"] = {"ms": ms, "event_ms": ev, "seen_through": int((hits > 0).sum())}
                rem = capi.default_visibility_params(min_hits=1)
                ms, ev, n = timed(lambda: raw(ctx, views, rem, None), st, prep=lambda: ctx.map_build(mp))
                r["remove"] = {"ms": ms, "event_ms": ev, "removed": n}
                res[key] = r
                print(key, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
