"""Every route of the iterated update against the bytes the library gave BEFORE the update driver moved into lv_update.hpp
(tests/golden/update_routes.npz, written by tests/golden/make_golden_routes.py on an MI355X from that commit): lv_update on the
one-launch-per-pass form and on three kernels, the split API, lv_filter_set + lv_correct + lv_filter_get on both forms, lv_update
with capture, with profiling and with the trace download; MAX_NUM_ITERS 0 and 3; scans of 0, 1, 33 (two 32-point tiles), 2 000 and
67 585 points (the smallest scan whose fit blocks exceed what solve_kernel folds directly: the group reduction).

The kernels are bit-reproducible and did not change, so equality is asserted on the bytes, not closeness.  Not every case
tells the routes apart: with 0, 1 or 33 points all eight routes agree byte for byte (so few partials that every order of the
reduction gives the same sums); those cases hold the empty and tiny paths (the begin kernel instead of a ride, two tiles, the
pass count).  The 2 000- and 67 585-point cases are the ones whose bytes differ between the one-launch form and the three-kernel
forms.  The host test of the same driver, with fake launches and injected failures, is tests/test_update_host.py."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_routes as mg  # noqa: E402

CASES = [(it, n, r) for it in mg.MAX_ITERS for n in mg.SCAN_SIZES for r in mg.ROUTES]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "update_routes.npz"))
    assert list(g["names"]) == mg.case_names()   # (the recording covers exactly the cases listed here, in this order)
    return {name: (g["x"][i], g["P"][i], int(g["passes"][i])) for i, name in enumerate(g["names"])}


@functools.lru_cache(maxsize=None)
def _scene(n):
    from limo_velo_amd import synth

    return synth.make_scene(mg.MAP_POINTS, max(n, 1))


@pytest.fixture(scope="module")
def contexts(lv):
    """One context per MAX_NUM_ITERS with the map built, shared by that setting's cases; `scan` remembers the size in place."""
    from limo_velo_amd import capi

    made = {}

    def get(iters):
        if iters not in made:
            ctx = capi.Context(capi.default_params(MAX_NUM_ITERS=iters))
            ctx.map_build(_scene(1)["map_xyz"])
            made[iters] = [ctx, None]
        return made[iters]

    yield get
    for ctx, _ in made.values():
        ctx.close()


@pytest.mark.parametrize("iters,n,route", CASES, ids=[f"iters{it}-n{n}-{r}" for it, n, r in CASES])
def test_route_gives_the_parents_bytes(contexts, golden, iters, n, route):
    slot = contexts(iters)
    ctx = slot[0]
    sc = _scene(n)
    if slot[1] != n:
        ctx.scan_set(sc["scan_xyz"][:n])
        slot[1] = n
    x, P, passes = mg.run_route(ctx, route, sc["x_init"], sc["P0"])
    gx, gP, gp = golden[f"iters{iters}/n{n}/{route}"]
    assert passes == gp
    assert x.tobytes() == gx.tobytes(), np.abs(x - gx).max()
    assert P.tobytes() == gP.tobytes(), np.abs(P - gP).max()
    if route != "split":   # (the split API leaves the flag of the update before it) ... and the route meant is the route taken
        assert ctx.last_update_fused() == (route in ("update", "correct", "update_profiling", "update_trace") and n > 0)
