"""Generated cases of the submap merge for the CPU, host and GPU tests (the rule: tests/surf_merge_ref.py).

The destination is 24 x 20 x 12 voxels; the submaps are around 16 x 12 x 10 (18 x 14 x 10 where a rotated one has to fill a quarter
of the destination).  A submap holds the distance to a plane, truncated to
its own band, with weights that vary from voxel to voxel, nothing behind the band (W = 0, as a fused volume has it) and a few
holes.  Every case names what it claims to exercise; tests/test_surf_merge_ref.py asserts the claims on the reference alone."""
import numpy as np

import surf_merge_ref as mr

F = np.float32
NX, NY, NZ = 24, 20, 12
SHAPE = (NZ, NY, NX)
SUB_SHAPE = (10, 12, 16)


def destination(resolution=0.25, origin=(-3.0, -2.5, -1.5), trunc_cells=3, max_weight=10000, fill=None):
    d = dict(origin=np.asarray(origin, F), resolution=F(resolution), trunc_cells=trunc_cells, max_weight=max_weight,
             S=np.zeros(SHAPE, np.int32), W=np.zeros(SHAPE, np.int32))
    if fill is not None:   # a known volume of constant distance `fill` sub-units and weight max_weight - 3
        d["W"][:] = max_weight - 3
        d["S"][:] = fill * (max_weight - 3)
    return d


def plane_submap(origin, resolution, trunc_cells=3, shape=SUB_SHAPE, normal=(0.3, 0.2, 1.0), offset=0.1, seed=1, w_hi=40, holes=0.03, keep_behind=False):
    """The distance n . x - offset (metres, in the submap's frame) at every voxel centre, in sub-units of the submap and truncated to
    +-T; W in 1..w_hi, 0 in a share `holes` of the voxels and, unless keep_behind, where the distance lies behind the band."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    n = np.asarray(normal, float)
    n = n / np.linalg.norm(n)
    z, y, x = np.meshgrid(*(float(origin[2 - a]) + (np.arange(s) + 0.5) * float(resolution) for a, s in enumerate(shape)), indexing="ij")
    phi = (n[0] * x + n[1] * y + n[2] * z - offset) / float(resolution) * 256.0
    T = 256 * trunc_cells
    W = rng.integers(1, w_hi + 1, shape)
    W[rng.random(shape) < holes] = 0
    if not keep_behind:
        W[phi < -T] = 0
    S = np.floor(np.clip(phi, -T, T) * W).astype(np.int64)
    S = np.clip(S, -T * W, T * W)
    return dict(origin=np.asarray(origin, F), resolution=F(resolution), trunc_cells=trunc_cells, S=S.astype(np.int32), W=W.astype(np.int32),
                normal=n, offset=offset)


def _case(name, dest, sub, pose, claims, min_weight=1, interp=mr.TRILINEAR):
    return dict(name=name, dest=dest, sub=sub, pose=pose, claims=set(claims), min_weight=min_weight, interp=interp)


SKEW = (mr.quat((0.3, -0.5, 0.8), 0.6))
TILT = (mr.quat((0.2, -0.3, 0.9), 0.4))   # a skew rotation under which an 18 x 14 x 10 submap stays inside the destination


def cases():
    """name -> case.  Claims: quarter (a quarter of the destination box contributes: of the voxels the call is launched over,
    surf_merge_ref.box, which under a rotation is the whole destination), outside, unknown, dropped, clamped,
    folded (at max_weight), last_layer (f = 0 on the submap's last layer of an axis, and inside).  `grazes` and `misses` cannot claim
    quarter by what they are: a submap that lies outside the volume but for a strip, and one whose box is empty."""
    out = []
    # same lattice, equal resolution: powers of two, so that every centre is exact
    on = (-3.0 + 3 * 0.25, -2.5 + 2 * 0.25, -1.5 + 1 * 0.25)
    for interp, tag in ((mr.TRILINEAR, ""), (mr.NEAREST, "_nearest")):
        out.append(_case("identity" + tag, destination(), plane_submap(on, 0.25), mr.IDENTITY, {"quarter", "outside", "unknown", "last_layer"}, interp=interp))
        out.append(_case("shift" + tag, destination(), plane_submap(on, 0.25, seed=2), (np.array([0.5, -0.25, 0.25]), mr.IDENTITY[1]),
                         {"quarter", "outside", "unknown", "last_layer"}, interp=interp))
    # a skew rotation with an off-lattice translation, awkward resolutions
    d2 = dict(resolution=0.2, origin=(-2.4, -2.0, -1.2))
    so = (-1.5, -1.1, -0.9)
    t_off = np.array([0.137, -0.211, 0.093])
    # (a quarter of the 5760 voxels is 1440: the submap is 18 x 14 x 10 about the destination's middle, its surface low in it so that
    # little lies behind the band, and few voxels are holes: an UNKNOWN corner silences up to eight destination voxels)
    mid = (-1.8, -1.4, -1.0)
    t_mid = np.array([0.037, -0.061, 0.023])
    big = dict(shape=(10, 14, 18), offset=-0.5, holes=0.004)
    for interp, tag in ((mr.TRILINEAR, ""), (mr.NEAREST, "_nearest")):
        out.append(_case("skew" + tag, destination(**d2), plane_submap(mid, 0.2, seed=3, **big), (t_mid, TILT), {"quarter", "outside", "unknown"}, interp=interp))
    # resolution ratios 0.5, 1.25 and 2 (the submap keeps about its extent in metres)
    out.append(_case("ratio_0.5", destination(**d2), plane_submap(mid, 0.1, shape=(20, 28, 36), seed=4, offset=-0.5, holes=0.002), (t_mid, TILT),
                     {"quarter", "outside", "unknown"}))
    out.append(_case("ratio_1.25", destination(**d2), plane_submap(so, 0.25, seed=5), (t_off, SKEW), {"quarter", "outside", "unknown", "dropped", "clamped"}))
    out.append(_case("ratio_2", destination(**d2), plane_submap((-2.0, -1.6, -1.1), 0.4, shape=(6, 9, 11), trunc_cells=2, seed=6), (t_off, SKEW),
                     {"quarter", "outside", "unknown", "dropped", "clamped"}))
    # a source band wider than the destination's (clamp and drop), and a narrower one
    out.append(_case("band_wider", destination(trunc_cells=2, **d2), plane_submap(mid, 0.2, trunc_cells=5, seed=7, keep_behind=True, **big), (t_mid, TILT),
                     {"quarter", "outside", "dropped", "clamped"}))
    out.append(_case("band_narrower", destination(trunc_cells=6, **d2), plane_submap(mid, 0.2, trunc_cells=2, seed=8, **big), (t_mid, TILT),
                     {"quarter", "outside", "unknown"}))
    # min_weight above some source weights
    out.append(_case("min_weight", destination(**d2), plane_submap(mid, 0.2, seed=9, w_hi=60, **big), (t_mid, TILT), {"quarter", "outside", "unknown"}, min_weight=3))
    # a pre-filled destination that folds at max_weight
    out.append(_case("folds", destination(max_weight=50, fill=100, **d2), plane_submap(mid, 0.2, seed=10, **big), (t_mid, TILT),
                     {"quarter", "outside", "unknown", "folded"}))
    # a submap that only grazes the volume, and one that misses it
    out.append(_case("grazes", destination(**d2), plane_submap(so, 0.2, seed=11, normal=(0.0, 0.1, 1.0), offset=-0.6), (np.array([3.55, 0.3, 0.2]), mr.quat((0, 0, 1), 0.3)),
                     {"outside"}))
    out.append(_case("misses", destination(**d2), plane_submap(so, 0.2, seed=12), (np.array([40.0, 0.3, 0.2]), SKEW), {"outside"}))
    return {c["name"]: c for c in out}


def pair():
    """Two submaps that overlap in the destination, for the order test and Submaps.fuse: (destination, [(submap, pose), ...])."""
    d = destination(resolution=0.2, origin=(-2.4, -2.0, -1.2))
    a = plane_submap((-1.5, -1.1, -0.9), 0.2, seed=21)
    b = plane_submap((-1.2, -1.4, -0.8), 0.25, seed=22, normal=(0.25, 0.25, 1.0), offset=0.12)
    return d, [(a, (np.array([0.137, -0.211, 0.093]), SKEW)), (b, (np.array([-0.3, 0.25, 0.05]), mr.quat((0.1, 0.2, 1.0), -0.35)))]


def linear_field():
    """A plane's distance, analytic on both sides: a submap of resolution 0.25 turned by 0.6 rad about a skew axis into a destination
    of resolution 0.2, both bands wide enough that the voxels judged lie inside both."""
    d = destination(resolution=0.2, origin=(-2.4, -2.0, -1.2), trunc_cells=8)
    s = plane_submap((-2.0, -1.5, -1.25), 0.25, trunc_cells=8, seed=31, holes=0.0, keep_behind=True)
    # exact source values: S = round-free floor of phi * W is the source's own floor (one unit of S, 1 / W of a sub-unit)
    return d, s, (np.array([0.137, -0.211, 0.093]), SKEW)
