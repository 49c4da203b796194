"""Timing of place recognition (include/limovelo_hip.h "Place recognition") with the default parameters (20 rings x 60 sectors):
  `add_scan_ms`  lv_place_add_scan of a 64 k-point scan (synth.make_scene, 10 M-point scene);
  `add_map_ms`   lv_place_add_map of 10 k centres (a grid over the scene at z = 1.5 m) on the 10 M-point map;
  `query_ms`     lv_place_query (k = 64) of that scan against 100 k places loaded with lv_place_load (random descriptors with empty
                 columns and bins); includes the scan's descriptor, the scoring, the top-k and the copy back.
Host wall time of each call (every call synchronises before it returns); one warm-up call, then the median of REPS calls
(add_map: of 3).  Prints one JSON line; --out writes it too.

    python scripts/place_timing.py [--out profiles/place_timing.json] [--map-points 10000000]
Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python scripts/place_timing.py` run."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (torch's runtime first: tests/conftest.py)

import lvamd  # noqa: E402

lvamd.load()
from limo_velo_amd import capi, synth  # noqa: E402

REPS = 20


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--map-points", type=int, default=10_000_000)
    ap.add_argument("--scan-points", type=int, default=65_536)
    ap.add_argument("--centres", type=int, default=10_000)
    ap.add_argument("--places", type=int, default=100_000)
    a = ap.parse_args()
    sc = synth.make_scene(a.map_points, a.scan_points)
    L = float(sc["L"])
    side = int(math.ceil(math.sqrt(a.centres)))
    g = np.linspace(-0.95 * L, 0.95 * L, side)
    centres = np.array([[x, y, 1.5] for x in g for y in g])[: a.centres]
    rng = np.random.default_rng(1)
    desc = rng.uniform(0.0, 9.0, (a.places, 20, 60)).astype(np.float32)
    desc *= rng.uniform(size=(a.places, 1, 60)) > 0.25
    desc *= rng.uniform(size=(a.places, 20, 60)) > 0.4
    res = dict(map_points=a.map_points, scan_points=a.scan_points, centres=len(centres), places=a.places, k=64)
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        x = sc["x_true"]

        def add_scan():
            ctx.place_clear()
            ctx.place_add_scan(x)

        res["add_scan_ms"] = timed(add_scan, REPS)

        def add_map():
            ctx.place_clear()
            ctx.place_add_map(centres)

        res["add_map_ms"] = timed(add_map, 3)
        ctx.place_clear()
        ctx.place_load(desc, np.zeros((a.places, 3)))
        res["query_ms"] = timed(lambda: ctx.place_query(x, 64), REPS)
        res["bins_per_place"] = 20 * 60
        res["query_desc_bytes"] = int(desc.nbytes)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
