"""Times lv_map_cluster against the route the entry points offered before it: lv_map_radius_search over all map points (the whole
CSR copied to the host) plus scipy.sparse.csgraph.connected_components.  Bench scene, one radius below and one above the level-0
bound of the 0.5 m cells.  Best of 3 after a warm-up, whole calls (host clock); both routes end with the same thing in host
memory, a component label per map point, and the script checks that the two partitions are the same.

    python scripts/map_cluster_timing.py [--points 1000000] [--radii 0.3 1.0] [--out profiles/map_cluster_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lvamd  # noqa: E402

lvamd.load()
from limo_velo_amd import capi, synth  # noqa: E402


def best_of(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--radii", type=float, nargs="+", default=[0.3, 1.0])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    xyz = synth.make_scene(a.points, 1000)["map_xyz"]
    res = dict(points=int(len(xyz)), scene="bench", radii=[])
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        own = ctx.map_fetch()
        m = len(own)
        for radius in a.radii:
            prm = capi.default_cluster_params(radius=radius)
            t_new, out = best_of(lambda: ctx.map_cluster(prm))
            parts = {}

            def old_route():
                t0 = time.perf_counter()
                off, idx, _ = ctx.map_radius(own, radius)
                t1 = time.perf_counter()
                g = csr_matrix((np.ones(len(idx), np.int8), idx.astype(np.int64), off.astype(np.int64)), shape=(m, m))
                n, comp = connected_components(g, directed=False)
                t2 = time.perf_counter()
                parts["search_ms"], parts["host_ms"], parts["entries"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(len(idx))
                return n, comp

            # (a warm-up and a best-of only where one run is short: above the level-0 bound the CSR has ~10^9 entries)
            t0 = time.perf_counter()
            n_old, comp = old_route()
            t_old = (time.perf_counter() - t0) * 1e3
            if t_old < 5e3:
                t_old, (n_old, comp) = best_of(old_route, reps=2)
            # the same partition: a bijection between the two labellings
            pair = np.unique(np.stack([comp.astype(np.int64), out["labels"].astype(np.int64)], axis=1), axis=0)
            same = n_old == out["n_clusters"] and len(pair) == n_old and len(np.unique(pair[:, 0])) == len(np.unique(pair[:, 1])) == n_old
            res["radii"].append(dict(radius=radius, map_cluster_ms=t_new, radius_search_plus_host_ms=t_old, radius_search_ms=parts["search_ms"],
                                     host_components_ms=parts["host_ms"], edges=(parts["entries"] - m) // 2, n_clusters=int(out["n_clusters"]),
                                     largest=int(out["sizes"][0]), speedup=t_old / t_new, same_partition=bool(same)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
