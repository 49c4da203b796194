"""The cases tests/test_tsdf_ray_ref.py, tests/test_tsdf_ray_host.py and tests/test_gpu_tsdf_ray.py share: volumes, a small synthetic
colour layer for each, and rays that reach every branch of the rule.  A case is dict(name, prm, S, W, layer, min_weights, rays)
with rays a dict name -> (from [n, 3], to [n, 3]) f32; a case with `source` is the volume of that tsdf_cases case (built by its
lv_tsdf_integrate calls), one with `shift` that volume after lv_volume_recentre by the shift; the others are loaded by hand.  The
answers of a case are computed once (answers()) and shared, read-only."""
import functools

import numpy as np

import colour_ref as cr
import tsdf_cases as tc
import tsdf_ray_ref as trr
import tsdf_ref as tr

F = np.float32
SOURCES = ("33x17x9-carve0-3views", "33x17x9-carve1-3views", "70x37x20-carve0-3views", "70x37x20-carve1-3views", "33x17x9-maxweight4",
           "70x37x20-maxweight4", "sphere-6")
SHIFT = (3, -2, 1)


def layer_for(W, seed):
    """A synthetic colour layer [nz, ny, nx, 4] uint32: about half the observed voxels coloured, C <= 255 Wc."""
    rng = np.random.default_rng(seed)
    wc = rng.integers(0, 5, W.shape) * (np.asarray(W) > 0) * (rng.random(W.shape) < 0.6)
    c = rng.integers(0, 256, W.shape + (3,)) * wc[..., None]
    c -= rng.integers(0, 2, c.shape) * (c > 0)   # (sums that are no multiple of Wc: the rounding of the voxel colour)
    return np.concatenate([c, wc[..., None]], axis=-1).astype(np.uint32)


def shifted_origin(origin0, resolution, shift):
    """origin0[a] + (float)shift[a] * resolution, f32 and unfused ("Rolling volumes")."""
    return tuple(float(F(o) + F(s) * F(resolution)) for o, s in zip(origin0, shift))


def _box(prm):
    lo = np.asarray(prm["origin"], np.float64)
    return lo, lo + np.array([prm["nx"], prm["ny"], prm["nz"]]) * float(prm["resolution"])


def _centres(prm, cells):
    return (np.asarray(prm["origin"], np.float64) + (np.asarray(cells, np.float64) + 0.5) * float(prm["resolution"])).astype(F)


def common_rays(prm, S, W, min_weight, seed):
    """Random rays from inside and from every side of the grid, rays that start in an IN cell, from == to, rays through voxel
    corners, non-finite and too-far ends."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(prm)
    span = hi - lo
    res = float(prm["resolution"])
    out = {}
    places = [lo + span * (0.52, 0.47, 0.55)] + [lo + span * (0.5 + 1.1 * np.eye(3)[a] * s + 0.1 * np.roll(np.eye(3)[a], 1)) for a in range(3) for s in (-1, 1)]
    for p, place in enumerate(places):
        n = 140
        frm = (place + rng.normal(size=(n, 3)) * res * 0.7).astype(F)
        to = (lo + rng.uniform(-0.25, 1.25, (n, 3)) * span).astype(F)
        out[f"random{p}"] = (frm, to)
    st = trr.states(S, W, min_weight)
    kk, jj, ii = np.nonzero(st == trr.IN)
    pick = rng.permutation(len(ii))[:40]
    cells = np.stack([ii, jj, kk], axis=1)[pick]
    out["start_in"] = (_centres(prm, cells), (lo + rng.uniform(-0.2, 1.2, (len(cells), 3)) * span).astype(F))
    # from == to: in an IN cell, an OUT cell, an UNKNOWN cell (where the volume has them), outside the grid
    same = [lo - span * 0.3, hi + res]
    for state in (trr.IN, trr.OUT, trr.UNKNOWN):
        kk, jj, ii = np.nonzero(st == state)
        if len(ii):
            same.append(_centres(prm, [(ii[0], jj[0], kk[0])])[0])
    same = np.asarray(same, F)
    out["from_is_to"] = (same, same.copy())
    # through voxel corners: from a corner of the lattice along the diagonals of the voxels and of their faces (every boundary a tie)
    dirs = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c).count(0) <= 1], np.float64)
    corner = lo + res * np.floor(np.array([prm["nx"], prm["ny"], prm["nz"]]) * (0.45, 0.55, 0.5))
    frm = np.tile(corner, (len(dirs), 1))
    out["corners"] = (frm.astype(F), (frm + dirs * res * 40).astype(F))
    centre = (lo + span * 0.5).astype(F)
    far = centre + F(9000.0 * res)
    bad_from = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), far, centre, centre, centre, centre], F)
    bad_to = np.array([centre, centre, centre, centre, (np.nan, 1, 1), (np.inf, np.inf, np.inf), centre + F(70000.0 * res), centre + F(1.0)], F)
    out["ignored"] = (bad_from, bad_to)   # (the last one is a ray like any other)
    return out


def long_case():
    """1024 x 3 x 2, loaded by hand: rays along +-x cross every packed word and the word tail; S_A = 0; a HIT whose A is KNOWN only
    at min_weight 1."""
    prm = tr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=1024, ny=3, nz=2, min_range=0.05, max_range=100.0)
    T = prm["trunc_cells"] * 256
    rng = np.random.default_rng(41)
    shape = (2, 3, 1024)
    W = rng.choice(np.array([0, 1, 3]), size=shape, p=(0.25, 0.35, 0.4))
    S = rng.integers(0, T, shape) * W
    inside = rng.random(shape) < 0.012
    S = np.where(inside, -rng.integers(1, T, shape) * W, S)
    S[1, 0, :] = np.abs(S[1, 0, :])    # two rows without an IN cell: a ray along them sees every word
    S[1, 2, :] = np.abs(S[1, 2, :])
    # row (j = 1, k = 0), the marked spot: ... OUT (W 3) | S = 0, W = 1 | IN (W 3) | OUT (W 1) | OUT (W 3) ...
    W[0, 1, 90:115] = 3
    S[0, 1, 90:115] = 500
    W[0, 1, 100], S[0, 1, 100] = 1, 0
    W[0, 1, 101], S[0, 1, 101] = 3, -200
    W[0, 1, 102], S[0, 1, 102] = 1, 300
    S, W = S.astype(np.int32), W.astype(np.int32)
    assert tr_valid(prm, S, W)
    rays = common_rays(prm, S, W, 1, 7)
    frm, to = [], []
    for k in range(2):
        for j in range(3):
            y, z = (j + 0.5) * 0.5, (k + 0.5) * 0.5
            frm += [(-1.0, y, z), (513.0, y, z)]
            to += [(513.0, y, z), (-1.0, y, z)]
    for x0 in rng.uniform(0.0, 512.0, 60):      # along x from anywhere, both ways, on the rows without an IN cell
        for j in (0, 2):
            y = (j + 0.5) * 0.5
            frm += [(x0, y, 0.75), (x0, y, 0.75)]
            to += [(600.0, y, 0.75), (-20.0, y, 0.75)]
    rays["along_x"] = (np.asarray(frm, F), np.asarray(to, F))
    y, z = 0.75, 0.25
    rays["marked"] = (np.array([(49.25, y, z), (55.25, y, z), (50.25, y, z)], F), np.array([(53.0, y, z), (49.0, y, z), (53.0, y, z)], F))
    return dict(name="long-1024x3x2", prm=prm, S=S, W=W, layer=layer_for(W, 5), min_weights=(1, 2), rays=rays)


def dense_case():
    """21 x 4 x 3, loaded by hand with every state everywhere: nx no multiple of 16, and far more stops, BLOCKED rays and one-sided
    gradients than a fused volume shows."""
    prm = tr.params(origin=(-0.5, 0.25, 1.0), resolution=0.25, nx=21, ny=4, nz=3, min_range=0.05, max_range=50.0)
    T = prm["trunc_cells"] * 256
    rng = np.random.default_rng(43)
    shape = (3, 4, 21)
    W = rng.choice(np.array([0, 1, 2, 7]), size=shape, p=(0.3, 0.2, 0.2, 0.3))
    S = (rng.integers(-T // 4, T, shape) * W).astype(np.int32)
    S[rng.random(shape) < 0.1] = 0
    W = W.astype(np.int32)
    assert tr_valid(prm, S, W)
    return dict(name="dense-21x4x3", prm=prm, S=S, W=W, layer=layer_for(W, 6), min_weights=(1, 2, 3), rays=common_rays(prm, S, W, 1, 8))


def tr_valid(prm, S, W):
    """What lv_tsdf_load asks of a volume."""
    T = prm["trunc_cells"] * 256
    return bool(np.all((W >= 0) & (W <= prm["max_weight"]) & (np.abs(S.astype(np.int64)) <= T * W.astype(np.int64))))


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    fused = {c["name"]: c for c in tc.cases()}
    for i, name in enumerate(SOURCES):
        case = fused[name]
        ref = tc.reference(case)
        mw = case["min_weight"]
        out.append(dict(name=name, source=case, prm=case["prm"], S=ref["S"], W=ref["W"], layer=layer_for(ref["W"], 100 + i),
                        min_weights=(mw,), rays=common_rays(case["prm"], ref["S"], ref["W"], mw, 200 + i)))
    # the first volume again after a recentre, under the first case's own rays: the same world, another box
    case = fused[SOURCES[0]]
    ref = tc.reference(case)
    prm = dict(case["prm"], origin=shifted_origin(case["prm"]["origin"], case["prm"]["resolution"], SHIFT))
    S, W = cr.shift_layer(ref["S"], SHIFT), cr.shift_layer(ref["W"], SHIFT)
    out.append(dict(name=SOURCES[0] + "-recentred", source=case, shift=SHIFT, prm=prm, S=S, W=W, layer=cr.shift_layer(layer_for(ref["W"], 100), SHIFT),
                    min_weights=(1,), rays=out[0]["rays"]))   # (the same rays as before the recentre)
    out += [long_case(), dense_case()]
    for c in out:
        for a in (c["S"], c["W"], c["layer"]):
            a.setflags(write=False)
    return tuple(out)


def cases():
    return list(_cases())


def case(name):
    return {c["name"]: c for c in _cases()}[name]


@functools.lru_cache(maxsize=None)
def _answers(name, min_weight, coloured):
    c = case(name)
    out = {}
    for ray, (frm, to) in c["rays"].items():
        res = trr.raycast(c["prm"], c["S"], c["W"], frm, to, min_weight, c["layer"] if coloured else None)
        for a in res:
            a.setflags(write=False)
        out[ray] = res
    return out


def answers(name, min_weight, coloured=True):
    """dict ray set -> (results, normals, rgba) of the case by the reference: computed once, shared, read-only."""
    return _answers(name, int(min_weight), bool(coloured))


def all_rays(c):
    """Every ray set of a case in one pair of arrays, and the slices of the sets."""
    names = sorted(c["rays"])
    frm = np.concatenate([c["rays"][n][0] for n in names])
    to = np.concatenate([c["rays"][n][1] for n in names])
    at, slices = 0, {}
    for n in names:
        slices[n] = slice(at, at + len(c["rays"][n][0]))
        at += len(c["rays"][n][0])
    return frm, to, slices


def all_answers(c, min_weight, coloured=True):
    """The answers of all_rays(c), concatenated in its order."""
    ans = answers(c["name"], min_weight, coloured)
    names = sorted(c["rays"])
    return tuple(np.concatenate([ans[n][i] for n in names]) for i in range(3))
