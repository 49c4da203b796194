"""Multi-hypothesis update timing (lv_update_batch, limo-velo_amd/csrc/lv_batch.hip) on the 1 M-point scene: batch wall time (host
clock around the synchronous call), hypotheses/s, point-passes/s, the pass-count histogram and the launches per pass, beside the
same hypotheses run through a loop of lv_update (m <= 512).  Writes profiles/update_batch_timing.json (or --out)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_batch_timing.json"))
    ap.add_argument("--ns", default="2048,16384")
    ap.add_argument("--ms", default="1,64,512,4096")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, synth

    sc = synth.make_scene(1_000_000, max(int(n) for n in a.ns.split(",")))
    rng = np.random.default_rng(11)
    rows = []
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        for n in (int(v) for v in a.ns.split(",")):
            ctx.scan_set(sc["scan_xyz"][:n])
            for m in (int(v) for v in a.ms.split(",")):
                xs = np.repeat(sc["x_init"][None], m, 0)
                for i in range(m):   # yaw up to +-20 deg, xy up to +-1.5 m around the start
                    q = synth.quat_from_rpy(0.0, 0.0, math.radians(rng.uniform(-20, 20)))
                    xs[i, 3:7] = synth.quat_mul(q, xs[i, 3:7])
                    xs[i, :2] += rng.uniform(-1.5, 1.5, 2)
                ctx.update_batch(xs, sc["P0"])   # warm-up (allocations, code objects)
                best = math.inf
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    _, _, passes, _ = ctx.update_batch(xs, sc["P0"])
                    best = min(best, time.perf_counter() - t0)
                hist = np.bincount(passes, minlength=ctx.params.MAX_NUM_ITERS + 2).tolist()
                row = dict(n=n, m=m, batch_ms=best * 1e3, hyp_per_s=m / best, point_passes_per_s=float(passes.sum()) * n / best,
                           passes_hist=hist, launches_per_pass=3, chunk_hypotheses=int(min(m, max(1, (256 << 20) // (128 * n)))))
                if m <= 512:
                    ctx.update(xs[0], sc["P0"], want_trace=False)
                    t0 = time.perf_counter()
                    for x in xs:
                        ctx.update(x, sc["P0"], want_trace=False)
                    loop = time.perf_counter() - t0
                    row.update(loop_ms=loop * 1e3, speedup=loop / best)
                print(json.dumps(row), flush=True)
                rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(scene="make_scene(1_000_000, n)", rows=rows), f)


if __name__ == "__main__":
    main()
