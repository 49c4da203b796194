"""The statement of the frontier rule (include/limovelo_hip.h "Frontiers") in numpy, for the tests: cell states, the frontier
predicate, the components by scipy.ndimage.label, the canonical numbering, the cluster attributes and the rank over a given
potential array.  Everything after the states is integer arithmetic, so the tests compare by equality."""
import numpy as np
from scipy import ndimage

import occupancy_ref as ocr

F = np.float32
NONE = -1
UNREACHED = 0xFFFFFFFF
OTHER, FREE, OCCUPIED, UNKNOWN = 0, 1, 2, 3
STRUCTURE = {4: 1, 8: 2, 6: 1, 18: 2, 26: 3}   # connectivity -> generate_binary_structure's second argument
FIELDS = ("planar", "k_lo", "k_hi", "connectivity", "min_size")
CLUSTER_DTYPE = np.dtype([("size", np.int32), ("first", np.int32), ("rep", np.int32), ("centre", np.int32, 3), ("lo", np.int32, 3),
                          ("hi", np.int32, 3), ("sum", np.uint64, 3)])


def fparams(**kw):
    """A plain dict of lv_frontier_params (the defaults, overridden by kw)."""
    p = dict(planar=0, k_lo=0, k_hi=0, connectivity=26, min_size=1)
    p.update(kw)
    return p


def states(prm, L, fp):
    """uint8 [nz, ny, nx], or [1, ny, nx] of a planar result: OTHER, FREE, OCCUPIED or UNKNOWN per cell."""
    L = np.asarray(L, F)
    if fp["planar"]:
        v = ocr.project(prm, L, fp["k_lo"], fp["k_hi"])[None]
        return np.where(v == 100, OCCUPIED, np.where(v == 0, FREE, UNKNOWN)).astype(np.uint8)
    with np.errstate(all="ignore"):
        s = np.where(L >= F(prm["l_occ"]), OCCUPIED, np.where(L <= F(prm["l_free"]), FREE, OTHER))
    return np.where(np.isnan(L), UNKNOWN, s).astype(np.uint8)


def frontier_mask(st):
    """bool, the shape of st: FREE cells with an UNKNOWN face neighbour inside the field (a planar st has nz = 1: no z neighbours)."""
    unknown = st == UNKNOWN
    near = np.zeros(st.shape, bool)
    for axis in range(3):
        n = st.shape[axis]
        if n == 1:
            continue
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        near[tuple(lo)] |= unknown[tuple(hi)]
        near[tuple(hi)] |= unknown[tuple(lo)]
    return (st == FREE) & near


def components(mask, connectivity):
    """(lab int32 the shape of mask: 1..n on the components, 0 elsewhere; n) by scipy.ndimage.label."""
    if mask.shape[0] == 1 and connectivity in (4, 8):
        lab, n = ndimage.label(mask[0], ndimage.generate_binary_structure(2, STRUCTURE[connectivity]))
        return lab[None].astype(np.int32), n
    lab, n = ndimage.label(mask, ndimage.generate_binary_structure(3, STRUCTURE[connectivity]))
    return lab.astype(np.int32), n


def canonical(lab, n, min_size):
    """(labels int32 the shape of lab, clusters CLUSTER_DTYPE [C]) from any labelling 1..n: components below min_size dropped, the
    others numbered by size descending, ties to the smaller first member."""
    nz, ny, nx = lab.shape
    flat = lab.reshape(-1)
    cells = np.flatnonzero(flat)
    of = flat[cells] - 1
    size = np.bincount(of, minlength=n).astype(np.int64)
    first = np.full(n, flat.size, np.int64)
    np.minimum.at(first, of, cells)
    keep = np.flatnonzero(size >= min_size)
    order = keep[np.lexsort((first[keep], -size[keep]))]
    number = np.full(n + 1, NONE, np.int64)
    number[order + 1] = np.arange(len(order))
    labels = number[flat].reshape(lab.shape).astype(np.int32)
    labels[lab == 0] = NONE
    cl = np.zeros(len(order), CLUSTER_DTYPE)
    ijk = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], axis=1).astype(np.int64)
    for c, comp in enumerate(order):
        sel = of == comp
        m, idx = ijk[sel], cells[sel]
        s = m.sum(axis=0)
        centre = (2 * s + len(m)) // (2 * len(m))
        d2 = ((m - centre) ** 2).sum(axis=1)
        cl[c] = (len(m), idx.min(), idx[np.lexsort((idx, d2))[0]], centre, m.min(axis=0), m.max(axis=0), s)
    return labels, cl


def build(prm, L, fp):
    """(labels int32 [nz, ny, nx] or [ny, nx] when planar, clusters, stats [4] uint64) of a grid's log-odds."""
    st = states(prm, L, fp)
    mask = frontier_mask(st)
    lab, n = components(mask, fp["connectivity"])
    labels, cl = canonical(lab, n, fp["min_size"])
    stats = np.array([np.sum(st == FREE), np.sum(st == UNKNOWN), np.sum(mask), len(cl)], np.uint64)
    return (labels[0] if fp["planar"] else labels), cl, stats


def rank(labels, n_clusters, P, reach):
    """(best_p uint32 [C], best_cell int32 [C]) of labels over the potential P (both [nz, ny, nx], or both [ny, nx]): per cluster the
    least P within Chebyshev distance reach of a member, ties to the smaller cell; UNREACHED and -1 without a reached cell."""
    lab3 = labels[None] if labels.ndim == 2 else labels
    P3 = np.asarray(P)[None] if labels.ndim == 2 else np.asarray(P)
    nz, ny, nx = lab3.shape
    best = np.full(n_clusters, (UNREACHED << 32) | 0xFFFFFFFF, np.uint64)
    bid = (P3.astype(np.uint64) << np.uint64(32)) | np.arange(P3.size, dtype=np.uint64).reshape(P3.shape)
    bid[P3 == UNREACHED] = np.uint64((UNREACHED << 32) | 0xFFFFFFFF)
    for k, j, i in zip(*np.nonzero(lab3 >= 0)):
        w = bid[max(k - reach, 0):k + reach + 1, max(j - reach, 0):j + reach + 1, max(i - reach, 0):i + reach + 1]
        c = lab3[k, j, i]
        best[c] = min(best[c], w.min())
    return (best >> np.uint64(32)).astype(np.uint32), (best & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def flood_fill(mask, connectivity):
    """A labelling 1..n of mask by a plain Python flood fill (the check on scipy's)."""
    nz, ny, nx = mask.shape
    max_m = STRUCTURE[connectivity]
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < (dz != 0) + (dy != 0) + (dx != 0) <= max_m and not (connectivity in (4, 8) and dz)]
    lab = np.zeros(mask.shape, np.int32)
    n = 0
    for start in zip(*np.nonzero(mask)):
        if lab[start]:
            continue
        n += 1
        lab[start] = n
        stack = [start]
        while stack:
            k, j, i = stack.pop()
            for dz, dy, dx in offs:
                v = (k + dz, j + dy, i + dx)
                if 0 <= v[0] < nz and 0 <= v[1] < ny and 0 <= v[2] < nx and mask[v] and not lab[v]:
                    lab[v] = n
                    stack.append(v)
    return lab, n


def random_logodds(rng, shape, prm, p_unknown=0.3):
    """Log-odds [nz, ny, nx] drawn from {NaN, l_min, l_free, 0, l_occ, l_max}: NaN with p_unknown, the others equally likely."""
    vals = np.array([prm["l_min"], prm["l_free"], 0.0, prm["l_occ"], prm["l_max"]], F)
    L = vals[rng.integers(0, len(vals), shape)]
    L[rng.uniform(size=shape) < p_unknown] = np.nan
    return L.astype(F)


def serpentine(prm, nx, ny, nz, step=2):
    """Log-odds [nz, ny, nx] (nx, ny >= 3), unknown but for a one-cell-wide free corridor in layer 0, one cell inside the border
    (the border is not unknown: a corridor along it would lose its corner cells): rows 1, 1 + step, ... run from column 1 to
    nx - 2 and are joined at alternating ends.  Its frontier is the corridor itself: one component under every connectivity."""
    L = np.full((nz, ny, nx), np.nan, F)
    rows = list(range(1, ny - 1, step))
    for n, j in enumerate(rows):
        L[0, j, 1:nx - 1] = prm["l_min"]
        if n + 1 < len(rows):
            L[0, j:j + step + 1, nx - 2 if n % 2 == 0 else 1] = prm["l_min"]
    return L
