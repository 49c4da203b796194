"""The world, the fields and the batches that tests/test_occ_mcl_host.py runs through the host build of lv_mcl.hpp and
tests/test_gpu_occ_mcl.py through the kernel, with their answers by tests/mcl_ref.py (computed once per process); and the scene of
the closed loop.

The world is a room of 40 x 30 x 3 cells of 0.25 m, all observed: walls two cells thick round it, and inside an L-shaped wall (a
long arm along x, a short one along y at its east end) and a pillar, so that no rotation or reflection maps the room onto itself.
The three layers are alike, so the planar field over them and every layer of the 3-D field show the same plan.  Fields: "planar",
"vol" (3-D), "trunc" (planar, max_cells 3: the middle of the room is LV_OCC_FAR), "signed" (planar, negative inside the walls)."""
import functools

import numpy as np

import distance_ref as dr
import mcl_ref as mr
import occupancy_ref as ocr

F = np.float32
NX, NY, NZ = 40, 30, 3
RES = 0.25
PRM = ocr.params(origin=(-1.0, -2.0, -0.125), resolution=RES, nx=NX, ny=NY, nz=NZ, min_range=0.1, max_range=30.0)
DPS = dict(planar=dr.dparams(planar=1, k_lo=0, k_hi=2), vol=dr.dparams(), trunc=dr.dparams(planar=1, k_lo=0, k_hi=2, max_cells=3),
           signed=dr.dparams(planar=1, k_lo=0, k_hi=2, signed_field=1))
Z_SENSOR = 0.3   # in layer 1
BS = (1, 3, 63, 64, 65, 130)
KS = (1, 2, 63, 64, 65, 257)
MAX_COST = 1 << 24


def grid():
    L = np.full((NZ, NY, NX), -1.0, F)
    L[:, :2, :] = L[:, -2:, :] = 1.0
    L[:, :, :2] = L[:, :, -2:] = 1.0
    L[:, 17:19, 8:26] = 1.0      # the L's long arm ...
    L[:, 9:19, 24:26] = 1.0      # ... and its short one
    L[:, 6:8, 9:11] = 1.0        # the pillar
    return L


@functools.lru_cache(maxsize=None)
def field(name, shift=(0, 0, 0)):
    """dict(origin, resolution, s2) of mcl_ref; shift: of the grid after a recentre by it and a rebuild."""
    import recentre_ref as rcr

    L, origin = grid(), np.asarray(PRM["origin"], F)
    if any(shift):
        L, origin = rcr.shift_logodds(L, shift), rcr.origin_at(PRM["origin"], shift, RES)
    s2, _ = dr.build(dict(PRM, origin=tuple(float(v) for v in origin)), L, DPS[name])
    return dict(origin=tuple(float(v) for v in origin), resolution=RES, s2=s2)


def table_of(n):
    """A likelihood-shaped table of n entries: the cost rises with the distance, steeply at first, and is 0 at an obstacle."""
    return np.rint(4000.0 * (1.0 - np.exp(-np.arange(n) / 6.0))).astype(np.uint32)


def random_batch(seed, K, B, n_table=4096, fname="planar", **mp):
    """Poses over the room and a margin round it (so some end points fall outside), every heading; beams of up to 6 m."""
    rng = np.random.default_rng(seed)
    lo = np.array(PRM["origin"][:2]) - 1.0
    hi = np.array(PRM["origin"][:2]) + RES * np.array([NX, NY]) + 1.0
    poses = np.stack([rng.uniform(lo[0], hi[0], K), rng.uniform(lo[1], hi[1], K), rng.uniform(0.0, 0.5, K), rng.uniform(-4.0, 4.0, K)], axis=1)
    a, r = rng.uniform(-np.pi, np.pi, B), rng.uniform(0.2, 6.0, B)
    beams = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.3, 0.3, B)], axis=1)
    return dict(field=fname, mp=mr.mparams(**mp), poses=poses.astype(F), beams=beams.astype(F), table=table_of(n_table))


def edge_beams():
    """With the pose (0, 0, 0, 0) a beam IS its world end point (sn = 0, cs = 1): the field's faces one ulp and one sub-unit either
    side, per axis, and non-finite coordinates."""
    o = np.asarray(PRM["origin"], F)
    n = np.array([NX, NY, NZ])
    mid = (o + (n // 2 + F(0.5)) * F(RES)).astype(F)
    rows, inside = [], []
    for a in range(3):
        lo, hi = o[a], F(o[a] + F(n[a]) * F(RES))
        sub = F(RES) / F(256)
        vals = [(lo, True), (np.nextafter(lo, F(-np.inf)), False), (F(lo - sub), False), (np.nextafter(hi, F(-np.inf)), True), (hi, False),
                (F(hi + sub), False), (F(hi - sub), True), (F(np.nan), False), (F(np.inf), False), (F(-np.inf), False), (F(o[a] + F(65536) * F(RES)), False)]
        for v, ok in vals:
            p = mid.copy()
            p[a] = v
            rows.append(p)
            inside.append(ok)
    return np.array(rows, F), np.array(inside)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> dict(field, mp, poses [K, 4], beams [B, 3], table)."""
    out = {}
    for n, B in enumerate(BS):
        for m, K in enumerate(KS):
            out[f"random_B{B}_K{K}"] = random_batch(100 + 10 * n + m, K, B, fname=("planar", "vol")[(n + m) & 1], out_cost=(0, 5000)[m & 1],
                                                    min_inside=min(B, m % 3))
    for nt in (1, 2, 4096):
        out[f"table_{nt}"] = random_batch(200 + nt, 65, 33, n_table=nt, out_cost=7)
    # a truncated field: LV_OCC_FAR in the middle of the room takes the last entry of a short table
    out["far_clamped"] = random_batch(301, 130, 64, n_table=5, fname="trunc", out_cost=1)
    # a signed field: the inside of the walls takes entry 0
    out["signed_clamped"] = random_batch(302, 130, 64, n_table=50, fname="signed", out_cost=9)
    # end points on the field's last cells, just outside them, and at NaN / inf; planar (z is not looked at) and 3-D
    e, _ = edge_beams()
    zero = np.zeros((1, 4), F)
    out["edges_planar"] = dict(field="planar", mp=mr.mparams(out_cost=100000, min_inside=0), poses=zero, beams=e, table=table_of(64))
    out["edges_vol"] = dict(out["edges_planar"], field="vol")
    # unusable headings among usable ones
    b = random_batch(303, 9, 33)
    b["poses"][:, :2] = [4.0, 1.0]
    b["poses"][:, 3] = [0.3, 1048576.0, -1048576.0, np.nan, np.inf, -np.inf, 1048575.9375, -1048575.9375, 2.0e6]
    out["headings"] = b
    # min_inside at n_in and at n_in + 1: particle 0 stands by the east wall looking out of the field
    b = random_batch(304, 3, 65, min_inside=0)
    b["poses"][0] = [8.6, 2.0, 0.2, 0.0]
    m = int(mr.weigh(field("planar"), b["mp"], b["poses"], b["beams"], b["table"])["n_in"][0])
    out["min_inside_at"] = dict(b, mp=mr.mparams(min_inside=m))
    out["min_inside_above"] = dict(b, mp=mr.mparams(min_inside=m + 1))
    # a score above 2^32: 300 beams of 2^24 each, inside or outside
    b = random_batch(305, 66, 300, n_table=2, out_cost=MAX_COST)
    b["table"] = np.full(2, MAX_COST, np.uint32)
    out["overflow"] = b
    # ties: particles 1 and 3 are alike and the best (they stand in the L's long arm, where the cost is least; the others in the open)
    b = random_batch(306, 5, 64)
    b["poses"][:] = [[1.0, -1.0, 0.2, 0.5], [4.5, 2.5, 0.2, 0.25], [0.0, 3.0, 0.2, 2.0], [4.5, 2.5, 0.2, 0.25], [8.0, 4.6, 0.2, -1.0]]
    b["beams"][:, :2] *= F(0.05)   # (end points next to the robot: the cost is that of the robot's own place)
    out["ties"] = b
    # nobody eligible: every particle stands far outside the field
    b = random_batch(307, 130, 33)
    b["poses"][:, :2] += F(500.0)
    out["none_eligible"] = b
    out["K0"] = dict(random_batch(308, 1, 3), poses=np.zeros((0, 4), F))
    return out


@functools.lru_cache(maxsize=None)
def answers():
    return {name: mr.weigh(field(b["field"]), b["mp"], b["poses"], b["beams"], b["table"]) for name, b in batches().items()}


def check_the_cases_do_what_they_are_for():
    """The answers show what each batch was made for (asserted on the reference, so on whatever equals it)."""
    a, b = answers(), batches()
    no = np.uint64(mr.NO_SCORE)
    assert (field("trunc")["s2"] == mr.FAR).any() and (field("signed")["s2"] < -1).any() and field("vol")["s2"].shape == (NZ, NY, NX)
    big = a["random_B130_K257"]
    assert np.all((big["n_in"] > 0) & (big["n_in"] < 130)) and len(set(big["n_in"].tolist())) > 30   # (some end points outside, for everyone)
    assert len(set(big["score"].tolist())) > 100
    assert np.all(a["table_1"]["score"][a["table_1"]["score"] != no] == 7 * (33 - a["table_1"]["n_in"][a["table_1"]["score"] != no]))   # (table_of(1) = [0])
    # the clamps: the same batches with the table's last, respectively first, entry changed give other scores
    for name, at in (("far_clamped", -1), ("signed_clamped", 0)):
        c = b[name]
        t = c["table"].copy()
        t[at] += 1000
        assert np.any(mr.weigh(field(c["field"]), c["mp"], c["poses"], c["beams"], t)["score"] != a[name]["score"]), name
    e, inside = edge_beams()
    assert a["edges_planar"]["n_in"][0] == inside[:22].sum() + 11 and a["edges_vol"]["n_in"][0] == inside.sum()   # (planar: z is not looked at)
    assert a["edges_vol"]["score"][0] >= 100000 * (~inside).sum()
    h = a["headings"]
    assert list(h["score"] == no) == [False, True, True, True, True, True, False, False, True] and np.all(h["n_in"][[1, 2, 3, 4, 5, 8]] == 0)
    assert np.all(h["n_in"][[0, 6, 7]] > 0)
    m = b["min_inside_at"]["mp"]["min_inside"]
    assert 0 < m < 65 and a["min_inside_at"]["n_in"][0] == m and a["min_inside_at"]["score"][0] != no
    assert a["min_inside_above"]["n_in"][0] == m and a["min_inside_above"]["score"][0] == no
    o = a["overflow"]
    assert np.all(o["score"] == np.uint64(300 * MAX_COST)) and 300 * MAX_COST > 2 ** 32 and list(o["best"]) == [0, 300 * MAX_COST]
    t = a["ties"]
    assert t["best"][0] == 1 and t["score"][1] == t["score"][3] == t["score"].min() and t["score"][3] < np.delete(t["score"], [1, 3]).min()
    n = a["none_eligible"]
    assert np.all(n["score"] == no) and np.all(n["n_in"] == 0) and list(n["best"]) == [-1, -1]
    assert list(a["K0"]["best"]) == [-1, -1] and len(a["K0"]["score"]) == 0


# ---- the closed loop: a robot drives through the room; its scans come from the grid itself
N_AZ, MAX_RANGE = 120, 8.0
TRUE_START = (1.6, -1.2, Z_SENSOR, 0.35)
ODOMETRY = [(0.10, 0.30, 0.05), (0.05, 0.30, 0.05), (0.0, 0.30, 0.10), (0.10, 0.30, 0.0), (0.05, 0.25, 0.10), (0.10, 0.30, 0.05),
            (0.0, 0.30, 0.0), (-0.05, 0.30, -0.05), (-0.10, 0.30, 0.0), (0.0, 0.25, -0.05)]   # (rot1, trans, rot2) per cycle
ALPHAS = (0.02, 0.02, 0.02, 0.02)
TRACK_K = 2048
SIGMA_HIT, SCALE, TEMPERATURE = 0.2, 16.0, 4.0


def true_poses():
    """[11, 4] f64: the start, then the pose after each noise-free odometry step."""
    x, y, z, th = TRUE_START
    out = [(x, y, z, th)]
    for r1, tr, r2 in ODOMETRY:
        x, y, th = x + tr * np.cos(th + r1), y + tr * np.sin(th + r1), th + r1 + r2
        out.append((x, y, z, th))
    return np.array(out)


def yaw(th):
    return np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]], F)


def pattern():
    from limo_velo_amd import occupancy

    return occupancy.scan_pattern(N_AZ, 1, 0.0, 0.0, MAX_RANGE)


def scan_points(ranges):
    """[N_AZ, 3] f64 end points in the body frame of the ranges of pattern() (non-returns stay inf / NaN)."""
    d = pattern().astype(np.float64) / MAX_RANGE
    with np.errstate(all="ignore"):
        return d * np.asarray(ranges, np.float64)[:, None]


def ref_ranges(pose):
    """simulate_scan by tests/occ_ray_ref.py."""
    import occ_ray_ref as orr

    t = np.array(pose[:3], F)
    to = (pattern() @ yaw(pose[3]).T + t).astype(F)
    frm = np.broadcast_to(t, to.shape)
    return orr.range_m(PRM, frm, to, orr.raycast(PRM, grid(), frm, to))


def tables():
    from limo_velo_amd import mcl

    return (mcl.likelihood_table(RES, SIGMA_HIT, 0.95, 0.05, MAX_RANGE, SCALE, 1024), mcl.weight_table(SCALE, TEMPERATURE, 4096))


def scan_beams(ranges, n_beams=60):
    from limo_velo_amd import mcl

    return mcl.beams_from_scan(scan_points(ranges), n_beams, MAX_RANGE)


RANK_CELLS, RANK_DEG = 4, (-30, -20, -10, 0, 10, 20, 30)


def ranking_poses(at=TRUE_START):
    """([n, 4] f32 poses on a grid of whole cells and steps of 10 degrees round `at`, the index of `at` itself, which of them lie
    more than 2 cells or 10 degrees from it)."""
    d = np.arange(-RANK_CELLS, RANK_CELLS + 1)
    dx, dy, dth = (v.reshape(-1) for v in np.meshgrid(d, d, np.array(RANK_DEG), indexing="ij"))
    poses = np.stack([at[0] + dx * RES, at[1] + dy * RES, np.full(len(dx), at[2]), at[3] + np.radians(dth)], axis=1).astype(F)
    true = int(np.flatnonzero((dx == 0) & (dy == 0) & (dth == 0))[0])
    far = (np.hypot(dx, dy) > 2.0) | (np.abs(dth) > 10)
    return poses, true, far


def run_track(ctx, scans, seed):
    """limo_velo_amd.mcl.track over the ten cycles from gaussian_particles round the start; scans: the ranges at true_poses()[1:]."""
    from limo_velo_amd import mcl

    rng = np.random.default_rng(seed)
    table, wtable = tables()
    p0 = mcl.gaussian_particles(TRUE_START, 0.3, 0.15, TRACK_K, rng)
    return mcl.track(ctx, p0, ODOMETRY, [scan_beams(r) for r in scans], table, wtable, rng, alphas=ALPHAS)


def track_error(history):
    """(position error in metres, heading error in radians) of the last estimate."""
    e, t = history[-1]["estimate"], true_poses()[-1]
    dth = e[3] - t[3]
    return float(np.hypot(e[0] - t[0], e[1] - t[1])), float(abs(np.arctan2(np.sin(dth), np.cos(dth))))
