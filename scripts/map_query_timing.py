"""Timing of the map queries on the bench scene (1 M-point map, 65 536 queries placed like the headline scan): lv_map_knn at
k = 5, 16, 32, lv_map_radius_search at 1 m, one 40 m lv_map_box_search.  Each call is warmed, then timed REPS times.  Two figures
per call, medians: `event_ms` between two HIP events recorded on the library context's own stream (torch.cuda.ExternalStream over
lv_get_stream) before and after the call, and `ms` = the host wall time of the call (perf_counter).  Both include host staging
and the copies back: a query call returns when its results are on the host.  Prints one JSON line with queries/s and an
ESTIMATE of the algorithmic bytes per query (the map records a query's deciding level streams; not a counter reading).

    python scripts/map_query_timing.py [--out profiles/map_query_timing.json]
Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python scripts/map_query_timing.py` run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch's runtime first: tests/conftest.py)

import lvamd  # noqa: E402

lvamd.load()
from limo_velo_amd import capi, synth  # noqa: E402
import lvoracle  # noqa: E402

REPS = 10


def timed(fn, stream):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall, ev = [], []
    for _ in range(REPS):
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
    a = ap.parse_args()
    torch.cuda.init()
    sc = synth.make_scene(1_000_000, 65_536)
    q = lvoracle.transform_scan(sc["x_init"], sc["scan_xyz"])
    n = len(q)
    res = {"map_points": 1_000_000, "queries": n, "reps": REPS, "timing": "medians of REPS calls: ms = host wall time of the call, event_ms = HIP events on the context stream around it; both include host staging and copies"}
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ptr = ctx.get_stream()
        st = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.current_stream()
        for k in (5, 16, 32):
            ms, ev, (idx, d2, found) = timed(lambda: ctx.map_knn(q, k), st)
            res[f"knn_k{k}"] = {"ms": ms, "event_ms": ev, "queries_per_s": n / (ms * 1e-3),
                                "bytes_per_query_note": "level-0 run: ~62 candidates x (12 B xyz + 4 B id) = ~1 KB per query when it decides",
                                "bytes_per_query": 62 * 16}
        ms, ev, (off, idx, d2) = timed(lambda: ctx.map_radius(q, 1.0), st)
        res["radius_1m"] = {"ms": ms, "event_ms": ev, "queries_per_s": n / (ms * 1e-3), "results": int(off[-1]),
                            "mean_per_query": float(off[-1]) / n, "bytes_per_query": "2 passes over the chosen source (level-0 run or 27+ lists)"}
        c = np.median(np.asarray(sc["map_xyz"]), axis=0).astype(np.float32)
        lo, hi = c - 20, c + 20
        ms, ev, (bidx, bxyz) = timed(lambda: ctx.map_box(lo, hi), st)
        res["box_40m"] = {"ms": ms, "event_ms": ev, "results": int(len(bidx)), "bytes": "16 B per id (one pass over the id array) + 16 B per result"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
