"""The independent statement of the clustering rule (include/limovelo_hip.h "Map clustering") in numpy / scipy:

1. candidate pairs from cKDTree.query_pairs in f64 at radius * (1 + 1e-5) (a superset of the f32 rule's pairs: the f32 squared
   distance differs from the exact one by a few 1e-7 relative);
2. the pairs filtered by the f32 rule: differences, squares and the left-to-right sum in np.float32, <= np.float32(radius) ** 2;
3. the mask: a pair counts only if both ends are included;
4. scipy.sparse.csgraph.connected_components;
5. the canonical order: size descending, ties to the component whose first member comes first; components outside
   [min_size, max_size] and excluded points get -1.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def calc_dist(a, b):
    """f32 squared distance, left to right, unfused (ikd-Tree calc_dist)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = a - b
    s = d * d
    return (s[..., 0] + s[..., 1]) + s[..., 2]


def edges(xyz, radius):
    """[e, 2] int64, i < j: the adjacent pairs under the f32 rule."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) < 2:
        return np.empty((0, 2), np.int64)
    pairs = cKDTree(xyz.astype(np.float64)).query_pairs(float(np.float32(radius)) * (1 + 1e-5), output_type="ndarray").astype(np.int64)
    if len(pairs) == 0:
        return pairs.reshape(0, 2)
    r2 = np.float32(radius) * np.float32(radius)
    keep = calc_dist(xyz[pairs[:, 0]], xyz[pairs[:, 1]]) <= r2
    return pairs[keep]


def canonical(comp, included, min_size=1, max_size=0):
    """(labels [n] int32, sizes [C] uint32, raw_size [n]): component ids `comp` (any numbering; only `included` entries count) put
    into the canonical order.  raw_size[i]: the size of i's component whatever the limits say (0 for an excluded point)."""
    comp = np.asarray(comp, np.int64)
    included = np.asarray(included, bool)
    n = len(comp)
    labels = np.full(n, -1, np.int32)
    raw = np.zeros(n, np.int64)
    idx = np.flatnonzero(included)
    if len(idx) == 0:
        return labels, np.zeros(0, np.uint32), raw
    uniq, first, inv, cnt = np.unique(comp[idx], return_index=True, return_inverse=True, return_counts=True)
    raw[idx] = cnt[inv]
    first_member = idx[first]
    ok = (cnt >= min_size) & ((max_size == 0) | (cnt <= max_size))
    order = np.lexsort((first_member, -cnt))          # size descending, then the first member ascending
    order = order[ok[order]]
    new = np.full(len(uniq), -1, np.int64)
    new[order] = np.arange(len(order))
    labels[idx] = new[inv]
    return labels, cnt[order].astype(np.uint32), raw


def components_of_edges(n, e, included=None):
    """component id per node of the graph on n nodes with the edges e [k, 2] among the included nodes."""
    included = np.ones(n, bool) if included is None else np.asarray(included, bool)
    e = np.asarray(e, np.int64).reshape(-1, 2)
    e = e[included[e[:, 0]] & included[e[:, 1]]] if len(e) else e
    g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
    return connected_components(g, directed=False)[1]


def cluster(xyz, radius, min_size=1, max_size=0, mask=None):
    """dict(labels, sizes, n_clusters, raw_size, comp, included): lv_map_cluster's result for the cloud xyz in map order."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    included = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    comp = components_of_edges(n, edges(xyz, radius), included) if n else np.zeros(0, np.int64)
    labels, sizes, raw = canonical(comp, included, min_size, max_size)
    return dict(labels=labels, sizes=sizes, n_clusters=len(sizes), raw_size=raw, comp=comp, included=included)


def removed(xyz, radius, min_size=1, max_size=0, mask=None, seeds=None):
    """bool [n]: what lv_map_remove_clusters takes.  seeds None: the included points of components below min_size; seeds: the
    components within [min_size, max_size] that hold a seeded included point."""
    c = cluster(xyz, radius, 1, 0, mask)
    raw, inc, comp = c["raw_size"], c["included"], c["comp"]
    if seeds is None:
        return inc & (raw < min_size)
    seeds = np.asarray(seeds).reshape(-1) != 0
    ok = inc & (raw >= min_size) & ((max_size == 0) | (raw <= max_size))
    seeded_comp = np.zeros(int(comp.max()) + 1 if len(comp) else 0, bool)
    seeded_comp[comp[inc & seeds]] = True
    return ok & seeded_comp[comp]
