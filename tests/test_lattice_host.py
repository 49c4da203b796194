"""The rule of lv_lattice.hpp (lattice_check, lat_prim_allowed, lat_edge, lat_relax, lat_next, lat_walk: what the kernels of
lv_lattice.hip run) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to
tests/lattice_ref.py: tests/emu/lattice_emu.cpp builds V over given cost bytes by plain sweeps to the fixpoint and walks the paths.
V, stats, reach, status, path states, primitives taken and path costs are equal, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import lattice_ref as lr
import occupancy_ref as ocr
import plan_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
TABLE6 = np.array([254, 180, 110, 70, 55, 50], np.uint8)


def _poses(recs):
    return " ".join("%s %d" % (" ".join(str(int(v)) for v in r["xyz"].view(np.uint32)), int(r["h"])) for r in recs)


def _records(t):
    out = []
    for r in np.asarray(t).reshape(-1):
        out.append(" ".join(str(int(v)) for v in [r["di"], r["dj"], r["h_to"], r["n_sweep"], r["length"], r["reserved"], r["penalty"], *r["sweep"].reshape(-1)]))
    return "\n".join(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lattice_host") / "lattice_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "lattice_emu.cpp"), "-o", str(exe)])

    def run(text):
        return subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")

    def lattice(prm, c, H, P, t, goals, starts=(), n_prims=None):
        t = np.asarray(t).reshape(-1)
        starts = starts if len(starts) else np.zeros(0, lr.POSE_DTYPE)
        ny, nx = c.shape
        lines = ["0", " ".join(str(int(v)) for v in np.array(list(prm["origin"]) + [prm["resolution"]], F).view(np.uint32)) + f" {nx} {ny}",
                 f"{H} {P} {len(t) if n_prims is None else n_prims}", _records(t if n_prims is None else t[:n_prims]), " ".join(str(int(v)) for v in c.reshape(-1)),
                 f"{len(goals)} {_poses(goals)}", f"{len(starts)} {_poses(starts)}"]
        out = run("\n".join(lines) + "\n")
        if out[0] != "params ok":
            return out[0]
        head = out[1].split()
        assert head[:4] == ["lattice", str(nx), str(ny), str(H)]
        V = np.array(out[2].split(), np.uint32).reshape(H, ny, nx)
        st = out[3].split()
        assert st[0] == "stats"
        rows = [[int(v) for v in ln.split()] for ln in out[4:4 + 2 * len(starts):2]]
        taken = [[int(v) for v in ln.split()] for ln in out[5:5 + 2 * len(starts):2]]
        assert all(r[2] == len(r) - 3 == len(tk) for r, tk in zip(rows, taken))
        return V, np.array(st[1:], np.uint64), int(head[4]), rows, taken

    lattice.run = run
    return lattice


def _pose_set(prm, dims, H, rng, n):
    """Goal and start records: cell centres with every kind of heading, random points in and round the grid, non-finite and far ones."""
    nx, ny = dims
    lo = np.array(prm["origin"], np.float64)
    res = prm["resolution"]
    rows = [[lo[0] + (rng.integers(nx) + 0.5) * res, lo[1] + (rng.integers(ny) + 0.5) * res, rng.uniform(), h]
            for h in list(rng.integers(-1, H, n)) + [-1, 0, H - 1, H, -2]]
    rows += [[rng.uniform(lo[0] - res, lo[0] + (nx + 1) * res), rng.uniform(lo[1] - res, lo[1] + (ny + 1) * res), np.nan, int(rng.integers(-1, H))] for _ in range(n // 2)]
    rows += [[np.nan, lo[1], 0, 0], [lo[0], np.inf, 0, -1], [1e30, 0, 0, 0], [lo[0] - 0.25 * res, lo[1], 0, 0]]
    return lr.poses(rows)


def _hold(emu, prm, c, t, goals, starts):
    H, P = t.shape
    V, st, reach, rows, taken = emu(prm, c, H, P, t, goals, starts)
    rV, rst = lr.build(prm, c, t, goals)
    assert np.array_equal(V, rV), f"{np.sum(V != rV)} states differ"
    assert list(st) == list(rst) and reach == lr.reach_of(t)
    status, cost, off, states, tk = lr.paths(prm, c, rV, t, starts)
    for s, row in enumerate(rows):
        a, b = int(off[s]), int(off[s + 1])
        assert row[0] == status[s] and row[1] == cost[s] and row[3:] == list(states[a:b]) and taken[s] == list(tk[a:b]), s
    return V, status


@pytest.mark.parametrize("dims,H,P,reach", [((12, 9), 4, 3, 2), ((23, 17), 8, 5, 3), ((9, 30), 16, 2, 8), ((1, 14), 3, 16, 5), ((1, 1), 2, 2, 1), ((19, 1), 1, 4, 8)])
def test_random_grids(emu, dims, H, P, reach):
    nx, ny = dims
    rng = np.random.default_rng(nx * 17 + ny + P)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=1)
    seen = set()
    for density in (0.0, 0.15, 0.4):
        c = pr.cell_cost(pr.random_s2(rng, (ny, nx), density), 1, TABLE6 if density else np.array([1], np.uint8))
        t = lr.random_table(rng, H, P, reach)
        ps = _pose_set(prm, dims, H, rng, 12)
        _, status = _hold(emu, prm, c, t, ps[:6], ps)
        seen |= set(status.tolist())
        _hold(emu, prm, c, t, ps[-4:], ps)   # every goal unusable
    assert 2 in seen and (nx * ny == 1 or 0 in seen)


def test_any_heading_goals_and_starts(emu):
    """h = -1: a goal seeds every heading of its cell; a start takes the heading with the least V, ties to the smaller h."""
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=6, ny=1, nz=1)
    c = np.ones((1, 6), np.uint8)
    t = lr.table(3, 2)
    t[0, 0] = lr.prim(1, 0, 0, 10)          # heading 0 drives +x
    t[1, 0] = lr.prim(1, 0, 1, 10, 7)       # heading 1 too, at a penalty
    t[2, 0] = lr.prim(-1, 0, 2, 10)         # heading 2 drives -x: it never gets to a goal at the right end
    t[2, 1] = lr.prim(0, 0, 1, 3)           # ... but may turn on the spot into heading 1
    goals = lr.poses([[5.5, 0.5, 0, -1]])
    starts = lr.poses([[2.5, 0.5, 0, -1], [2.5, 0.5, 0, 1], [2.5, 0.5, 0, 2], [5.5, 0.5, 0, -1], [2.5, 0.5, 0, 3]])
    V, st, reach, rows, taken = emu(prm, c, 3, 2, t, goals, starts)
    assert list(V[:, 0, 5]) == [0, 0, 0] and st[0] == 1
    assert list(V[:, 0, 2]) == [60, 81, 87] and reach == 1
    assert [r[:2] for r in rows] == [[0, 60], [0, 81], [0, 87], [0, 0], [2, lr.UNREACHED]]
    assert rows[0][3:] == [2, 3, 4, 5] and taken[0] == [0, 0, 0, 255]
    assert rows[2][3:] == [12 + 2, 6 + 2, 6 + 3, 6 + 4, 6 + 5] and taken[2] == [1, 0, 0, 0, 255]
    assert rows[3][3:] == [5] and taken[3] == [255]   # ties at the goal cell: the smaller h
    _hold(emu, prm, c, t, goals, starts)


def _good():
    t = lr.table(2, 2)
    t[0, 0] = lr.prim(1, 0, 0, 10, 0, [(1, 0)])
    return t


def test_every_refusal_of_the_table_check(emu):
    prm = ocr.params(nx=3, ny=2, nz=1)
    c = np.ones((2, 3), np.uint8)
    g = lr.poses([[0, 0, 0, 0]])

    def bad(t, H=2, P=2, goals=g, n_prims=None):
        out = emu(prm, c, H, P, t, goals, n_prims=n_prims)
        assert isinstance(out, str) and out.startswith("params bad: "), out
        return int(out.split(":")[1])

    assert not isinstance(emu(prm, c, 2, 2, _good(), g), str)
    assert bad(_good(), H=0) == -1 and bad(_good(), H=17) == -1 and bad(_good(), P=0) == -1 and bad(_good(), P=17) == -1
    assert bad(_good(), n_prims=3) == -1
    assert bad(lr.table(2, 2)) == -1                                        # no non-empty record
    assert bad(_good(), goals=np.zeros(0, lr.POSE_DTYPE)) == -1 and bad(_good(), goals=np.zeros(65537, lr.POSE_DTYPE)) == -1
    for field, value in (("di", 9), ("di", -9), ("dj", 9), ("dj", -9), ("h_to", 2), ("n_sweep", 11), ("reserved", 1), ("penalty", (1 << 24) + 1)):
        t = _good()
        t[1, 0][field] = value
        assert bad(t) == 2 and lr.check_table(2, 2, t)[0] == 2, field
    for s, off in ((0, (9, 0)), (0, (0, -9)), (9, (0, 1)), (1, (1, 0))):   # out of range, or a used-looking entry beyond n_sweep
        t = _good()
        t[0, 0]["sweep"][s] = off
        assert bad(t) == 0 and lr.check_table(2, 2, t)[0] == 0
    t = _good()
    t[1, 1] = lr.prim(0, 0, 1, 10)   # a self loop
    assert bad(t) == 3
    # what is allowed: a turn on the spot, an empty slot that would be a loop, the limits themselves
    t = _good()
    t[1, 1] = lr.prim(0, 0, 0, 10)
    t[1, 0] = lr.prim(0, 0, 1, 0)
    t[0, 1] = lr.prim(8, -8, 1, 65535, 1 << 24, [(8, -8)] * 10)
    assert not isinstance(emu(prm, c, 2, 2, t, g), str) and lr.check_table(2, 2, t) is None


def test_relax_at_the_overflow_edge(emu):
    U = lr.UNREACHED
    big = 65535 * 510 + (1 << 24)
    cases = [(0, 1, 1, 1, 0), (0, 1, 1, 10, 5), (U - 1 - 20, 1, 1, 10, 0), (U - 20, 1, 1, 10, 0), (U - 19, 1, 1, 10, 0), (U - 21, 1, 1, 10, 1),
             (U - 1 - big, 255, 255, 65535, 1 << 24), (U - big, 255, 255, 65535, 1 << 24), (U - big + 1, 255, 255, 65535, 1 << 24), (U - 1, 255, 255, 65535, 1 << 24),
             (U, 1, 1, 1, 0), (U, 255, 255, 65535, 1 << 24), (12345, 7, 9, 14, 3), (U - 3, 1, 1, 1, 0)]
    want = []
    for pv, cu, cv, ln, pen in cases:
        s = pv + ln * (cu + cv) + pen   # (Python integers: the 64-bit sum)
        want.append(U if pv == U or s >= U else s)
    assert U - 1 in want and want.count(U) >= 7   # sums of 0xFFFFFFFE, 0xFFFFFFFF and above are all there
    out = emu.run("1\n%d\n%s\n" % (len(cases), "\n".join(" ".join(str(v) for v in c) for c in cases)))
    assert [int(v) for v in out[:len(cases)]] == want


def test_sums_that_reach_the_limit_on_a_corridor(emu):
    """length 65535 and penalty 2^24 over cost-255 cells: V grows by 50 200 066 a step and stops short of 0xFFFFFFFF."""
    nx = 100
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=nx, ny=1, nz=1)
    c = np.full((1, nx), 255, np.uint8)
    t = lr.table(1, 1)
    t[0, 0] = lr.prim(-1, 0, 0, 65535, 1 << 24)
    step = 65535 * 510 + (1 << 24)
    V, st, _, rows, _ = emu(prm, c, 1, 1, t, lr.poses([[0.5, 0.5, 0, 0]]), lr.poses([[85.5, 0.5, 0, 0], [86.5, 0.5, 0, 0]]))
    n = (lr.UNREACHED - 1) // step
    assert n == 85 and list(V[0, 0, :n + 1]) == [k * step for k in range(n + 1)] and np.all(V[0, 0, n + 1:] == lr.UNREACHED)
    assert rows[0][:3] == [0, n * step, n + 1] and rows[1][:3] == [1, lr.UNREACHED, 0] and st[2] == n + 1 and st[3] == n * step
    _hold(emu, prm, c, t, lr.poses([[0.5, 0.5, 0, 0]]), lr.poses([[85.5, 0.5, 0, 0]]))
