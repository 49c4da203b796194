"""Generates tests/golden/update_routes.npz — x, P and the pass count of every route an iterated update can take through the
library (one launch per pass, three kernels, the split API, the resident filter on both forms, capture, profiling, the trace
download), for scans on either side of every size at which the host picks another path.  The kernels are bit-reproducible, so
tests/test_gpu_update_routes.py holds a later build to these BYTES: a change to the host-side driver (lv_update.hpp) that alters
what a route computes shows here.  The file pins the library as built from the commit BEFORE the driver moved into its header.

Uses limo_velo_amd.capi only, so the same script records any build.  Needs an MI355X:

    python tests/golden/make_golden_routes.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAP_POINTS = 50_000
# 0, 1: the empty and the smallest scan; 33: two 32-point tiles; 67_585: the smallest scan whose 256-point fit blocks (265)
# exceed the 264 records solve_kernel folds directly, so the three-kernel route takes the group reduction
SCAN_SIZES = (0, 1, 33, 2_000, 67_585)
MAX_ITERS = (0, 3)
ROUTES = ("update", "update_three_kernel", "split", "correct", "correct_three_kernel", "update_capture", "update_profiling",
          "update_trace")


def case_names():
    return [f"iters{it}/n{n}/{r}" for it in MAX_ITERS for n in SCAN_SIZES for r in ROUTES]


def run_route(ctx, route, x0, P0):
    """One update of the context's current scan by `route` -> (x [26], P [23, 23], passes).  Leaves the options as it found them."""
    if route == "update":
        x, P, passes, _, _ = ctx.update(x0, P0, want_trace=False)
    elif route == "update_three_kernel":
        ctx.set_fused_pass(False)
        try:
            x, P, passes, _, _ = ctx.update(x0, P0, want_trace=False)
        finally:
            ctx.set_fused_pass(True)
    elif route == "split":
        ctx.update_begin(x0, P0)
        for _ in range(ctx.params.MAX_NUM_ITERS + 1):
            ctx.pass_reduce()
            ctx.pass_solve()
        x, P, passes = ctx.update_end()
    elif route in ("correct", "correct_three_kernel"):
        ctx.set_fused_pass(route == "correct")
        try:
            ctx.filter_set(x0, P0)
            passes = ctx.correct()
            x, P = ctx.filter_get()
        finally:
            ctx.set_fused_pass(True)
    elif route == "update_capture":
        ctx.set_capture(True)
        try:
            x, P, passes, _, _ = ctx.update(x0, P0, want_trace=False)
        finally:
            ctx.set_capture(False)
    elif route == "update_profiling":
        ctx.set_profiling(1)
        try:
            x, P, passes, _, _ = ctx.update(x0, P0, want_trace=False)
        finally:
            ctx.set_profiling(0)
    elif route == "update_trace":
        x, P, passes = ctx.update(x0, P0, want_trace=True)[:3]
    else:
        raise ValueError(route)
    return np.asarray(x, np.float64).reshape(26), np.asarray(P, np.float64).reshape(23, 23), int(passes)


def run_cases():
    """Every case of case_names(), in that order -> x [C, 26], P [C, 23, 23], passes [C]."""
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, synth

    xs, Ps, ps = [], [], []
    for it in MAX_ITERS:
        with capi.Context(capi.default_params(MAX_NUM_ITERS=it)) as ctx:
            built = False
            for n in SCAN_SIZES:
                sc = synth.make_scene(MAP_POINTS, max(n, 1))   # (the generator needs one point; the map does not depend on n)
                if not built:
                    ctx.map_build(sc["map_xyz"])
                    built = True
                ctx.scan_set(sc["scan_xyz"][:n])
                for route in ROUTES:
                    x, P, passes = run_route(ctx, route, sc["x_init"], sc["P0"])
                    xs.append(x), Ps.append(P), ps.append(passes)
    return np.stack(xs), np.stack(Ps), np.asarray(ps, np.int64)


def main():
    x, P, passes = run_cases()
    assert np.isfinite(x).all() and np.isfinite(P).all()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "update_routes.npz")
    np.savez_compressed(out, names=np.array(case_names()), x=x, P=P, passes=passes)
    print("wrote", out, os.path.getsize(out), "bytes,", len(passes), "cases, passes", passes.tolist())


if __name__ == "__main__":
    main()
