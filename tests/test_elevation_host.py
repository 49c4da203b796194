"""The rule of lv_elevation.hpp (the cell and height of a point, the body band, the terrain of a known cell from the tile in LDS, the
class and the height in metres: what the kernels of lv_elevation.hip run) compiled with g++ and -fsanitize=address,undefined
through tests/emu/hip/hip_runtime.h and held to tests/elevation_ref.py: tests/emu/elevation_emu.cpp builds from the given points
and answers the given queries.  Equality on every layer, the stats and the queries, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import elevation_cases as cases
import elevation_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
DTYPES = dict(lo=np.int32, top=np.int32, span=np.int32, step=np.int32, slope2=np.int32, count=np.uint32, band_count=np.uint32, cls=np.int8)


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("elevation_host") / "elevation_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "elevation_emu.cpp"), "-o",
                           str(exe)])

    def run(prm, jobs):
        """jobs: ("B", points) or ("Q", points); returns (layers, stats) per build and (height, cls) per query."""
        head = " ".join([_bits(prm["origin"]), _bits([prm["resolution"]])] +
                        [str(prm[k]) for k in ("nx", "ny", "min_points", "head", "max_span", "max_step", "max_slope2")])
        lines = [head]
        for kind, pts in jobs:
            pts = np.asarray(pts, F).reshape(-1, 3)
            lines.append(f"{kind} {len(pts)} " + _bits(pts))
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        if out[0] != "params ok":
            return out[0]
        nx, ny = prm["nx"], prm["ny"]
        got, at = [], 1
        for kind, pts in jobs:
            if kind == "B":
                rows = np.array([r.split() for r in out[at:at + nx * ny]], np.int64).reshape(nx * ny, 9)
                at += nx * ny
                layers = {name: rows[:, c].astype(DTYPES[name]).reshape(ny, nx) for c, name in enumerate(er.LAYERS[:8])}
                layers["height"] = rows[:, 8].astype(np.uint32).view(F).reshape(ny, nx)
                tag, *stats = out[at].split()
                assert tag == "stats"
                at += 1
                got.append((layers, np.array(stats, np.uint64)))
            else:
                n = len(np.asarray(pts).reshape(-1, 3))
                rows = np.array([r.split() for r in out[at:at + n]], np.int64).reshape(n, 2)
                at += n
                got.append((rows[:, 0].astype(np.uint32).view(F), rows[:, 1].astype(np.int8)))
        assert out[at:] == [""]
        return got

    return run


def _held(got, want, what):
    assert er.same_layers(got[0], want[0]) is None, (what, er.same_layers(got[0], want[0]))
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])


def test_every_case(emu):
    want = cases.answers()
    for name, (prm, pts) in cases.cases().items():
        (got,) = emu(prm, [("B", pts)])
        _held(got, want[name], name)


def test_the_cases_decide_what_they_are_there_for():
    """On the reference alone: each case makes its clause of the rule decide."""
    A = cases.answers()
    L, stats = A["borders"]
    assert stats[0] == cases.NX * cases.NY + 2 and np.all(L["count"][:-1, :-1] >= 1) and L["count"][2, 2] == 1   # a border belongs to the higher cell
    L, stats = A["negative_z"]
    assert L["lo"][3, 3] == -900 and L["lo"][4, 4] == -256 * 40 and L["top"][4, 4] == -256 * 40 and L["height"][3, 3] < -3.0 and stats[1] == 1
    L, stats = A["nonfinite"]
    assert list(stats) == [5, 1, 2, 0] and L["count"][6, 6] == 3 and L["band_count"][6, 6] == 2 and L["top"][6, 6] == 10
    L, _ = A["min_points"]
    assert list(L["cls"][2, 2:5]) == [-1, 0, -1] and list(L["count"][2, 2:5]) == [2, 3, 3] and list(L["band_count"][2, 2:5]) == [2, 3, 2]
    assert np.isnan(L["height"][2, 2]) and not np.isnan(L["height"][2, 3]) and L["span"][2, 4] == 0 and L["lo"][2, 4] == 5
    L, stats = A["head"]
    assert list(L["band_count"][8, 8:11]) == [2, 1, 3] and list(L["top"][8, 8:11]) == [868, 100, 101] and stats[1] == 1
    L, stats = A["head0"]
    assert list(L["band_count"][8, 8:11]) == [1, 1, 2] and list(L["top"][8, 8:11]) == [100, 100, 100] and stats[1] == 3
    L, _ = A["neighbours"]
    assert (L["cls"][9, 3], L["step"][9, 3], L["slope2"][9, 3]) == (0, 0, 0) and L["count"][8:11, 2:5].sum() == 8   # alone among unknown cells
    assert L["slope2"][3, 8] == (2 * 21) ** 2 and L["slope2"][3, 14] == (2 * 30) ** 2 and L["slope2"][3, 13] == 60 ** 2   # only +x, only -x
    assert L["slope2"][10, 8] == 42 ** 2 and L["slope2"][11, 12] == 90 ** 2                                             # only +y, only -y
    L, stats = A["corners"]
    assert np.all(L["cls"][[0, 0, -1, -1], [0, -1, 0, -1]] == 0) and stats[2] == 10
    assert L["step"][0, 0] == 25 and L["slope2"][0, 0] == 50 ** 2 and L["step"][0, -1] == 50 and L["slope2"][0, -1] == 0
    L, _ = A["saturate"]
    assert L["lo"][5, 6] - L["lo"][5, 4] == 2 ** 24 - 10000 and np.all(L["slope2"][5, 4:7] == 2 ** 31 - 1) and L["slope2"][11, 11] == 0
    L, _ = A["span_step"]
    assert (L["span"][1, 1], L["cls"][1, 1], L["span"][4, 2], L["cls"][4, 2]) == (50, 0, 51, 100)
    assert list(L["step"][1, 5:7]) == [60, 60] and list(L["cls"][1, 5:7]) == [0, 0] and list(L["step"][4, 8:10]) == [61, 61] and list(L["cls"][4, 8:10]) == [100, 100]
    L, _ = A["slope"]
    assert list(L["slope2"][5, 11:14]) == [10000] * 3 and list(L["cls"][5, 11:14]) == [0, 0, 0]
    assert L["slope2"][9, 12] == 10001 and list(L["cls"][9, 11:14]) == [0, 100, 0]
    assert list(L["slope2"][5, 3:5]) == [10000] * 2 and list(L["cls"][5, 3:5]) == [0, 0] and list(L["cls"][9, 3:5]) == [100, 100]
    L, stats = A["random"]
    assert stats[1] > 100 and 100 < stats[2] < cases.NX * cases.NY and 0 < stats[3] < stats[2] and (L["count"] == 0).any()


def test_the_scene_reads_as_the_terrain_it_is():
    """The 70 x 37 scene on the reference: wall, table and kerb line lethal, the ramp free at its slope, the canopy ignored, the hole
    unknown, no flat cell lethal."""
    L, stats = cases.scene_answer()
    cls = L["cls"]
    assert cls.shape == (37, 70) and stats[0] == len(cases.scene()) > 60000
    assert np.all(cls[:, cases.WALL_I] == 100)
    ramp = cls[:, 52:69]   # x in [3.4, 6.8): clear of the ramp's foot and of the grid's edge
    assert np.all(ramp == 0)
    tan = np.median(np.sqrt(L["slope2"][:, 52:69].astype(np.float64)) / 512.0)
    assert abs(tan - np.tan(np.radians(12.0))) < 0.005, tan
    (ti0, tj0), (ti1, tj1) = cases.scene_cell(0.7, -2.5), cases.scene_cell(1.3, -1.9)
    assert np.all(cls[tj0:tj1 + 1, ti0:ti1 + 1] == 100) and np.all(L["span"][tj0:tj1 + 1, ti0:ti1 + 1] > 800)
    (ci0, cj0), (ci1, cj1) = cases.scene_cell(1.1, 0.7), cases.scene_cell(2.5, 2.1)
    canopy = (slice(cj0, cj1 + 1), slice(ci0, ci1 + 1))
    assert np.all(cls[canopy] == 0) and np.all(L["count"][canopy] > L["band_count"][canopy]) and 4900 < stats[1] - 1500 < 5400   # (the wall above 1.5 m is overhang too)
    (hi0, hj0), (hi1, hj1) = cases.scene_cell(-1.55, -2.65), cases.scene_cell(-1.05, -2.35)
    assert np.all(cls[hj0:hj1 + 1, hi0:hi1 + 1] == -1) and np.all(L["count"][hj0:hj1 + 1, hi0:hi1 + 1] == 0)
    kj = cases.scene_cell(0.0, 2.4)[1]
    (ki0, _), (ki1, _) = cases.scene_cell(-1.9, 0), cases.scene_cell(2.5, 0)
    # (the kerb's edge runs through the middle of row kj: that row spans it, the next one steps up from it)
    assert np.all(cls[kj:kj + 2, ki0:ki1 + 1] == 100) and np.all(L["span"][kj, ki0:ki1 + 1] > 153) and np.all(L["step"][kj + 1, ki0:ki1 + 1] > 150)
    flat = np.ones(cls.shape, bool)   # everything two cells away from a feature, the ramp aside
    for (i0, j0), (i1, j1) in ((cases.scene_cell(-3.0, -3.7), cases.scene_cell(-2.81, 3.69)), ((ti0, tj0), (ti1, tj1)), ((hi0, hj0), (hi1, hj1)),
                               (cases.scene_cell(-2.0, 2.4), cases.scene_cell(2.59, 3.69))):
        flat[max(j0 - 2, 0):j1 + 3, max(i0 - 2, 0):i1 + 3] = False
    flat[:, 50:] = False
    assert flat.sum() > 1000 and np.all(cls[flat] == 0)


def test_the_scene_and_queries(emu):
    prm, pts = cases.scene_params(), cases.scene()
    rng = np.random.default_rng(3)
    q = np.column_stack([rng.uniform(-7.5, 7.5, 400), rng.uniform(-4.2, 4.2, 400), rng.normal(size=400)]).astype(F)
    q[:6] = [[-7.0, -3.7, np.nan], [np.nan, 0, 0], [0, np.inf, 0], [6.9999, 3.6999, -np.inf], [-7.0001, 0, 0], [1e30, 0, 0]]
    build, (h, k) = emu(prm, [("B", pts), ("Q", q)])
    want = cases.scene_answer()
    _held(build, want, "scene")
    wh, wk = er.query(prm, want[0], q)
    assert er.same_bits(h, wh) and np.array_equal(k, wk)
    assert not np.isnan(h[0]) and np.isnan(h[1]) and np.isnan(h[2]) and k[1] == -1 and not np.isnan(h[3]) and np.isnan(h[4]) and np.isnan(h[5])
    assert (k == 100).any() and (k == 0).any() and (k == -1).sum() > 10


def test_odd_grids_and_rebuilds(emu):
    """Grids that end inside a tile, one cell wide and of one cell; a second build on the same buffers starts from nothing."""
    rng = np.random.default_rng(11)
    for nx, ny in ((33, 3), (1, 5), (70, 3), (1, 1), (32, 8), (65, 17)):
        prm = er.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=nx, ny=ny, min_points=2, head=512, max_span=120, max_step=80, max_slope2=9000)
        n = 12 * nx * ny
        pts = np.column_stack([rng.uniform(-0.3, nx * 0.5 + 0.3, n), rng.uniform(-0.3, ny * 0.5 + 0.3, n),
                               rng.choice([0.0, 0.1, 0.4, 3.0], n) + rng.normal(0, 0.05, n)]).astype(F)
        first, second, empty = emu(prm, [("B", pts), ("B", pts[: n // 3]), ("B", pts[:0])])
        _held(first, er.build(prm, pts), (nx, ny))
        _held(second, er.build(prm, pts[: n // 3]), (nx, ny, "again"))
        _held(empty, er.build(prm, pts[:0]), (nx, ny, "empty"))
        assert np.all(empty[0]["cls"] == -1) and np.all(empty[0]["lo"] == er.NONE) and np.all(empty[0]["top"] == -er.NONE) and not empty[1].any()


def test_parameter_limits(emu):
    ok = cases.prm()
    assert isinstance(emu(ok, []), list)
    for bad in (dict(nx=0), dict(nx=4097), dict(ny=0), dict(nx=4096, ny=4097), dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=np.inf),
                dict(origin=(0.0, np.nan, 0.0)), dict(min_points=0), dict(min_points=2 ** 20 + 1), dict(head=-1), dict(head=2 ** 25 + 1),
                dict(max_span=-1), dict(max_step=2 ** 25 + 1), dict(max_slope2=-1)):
        why = emu({**ok, **bad}, [])
        assert isinstance(why, str) and why.startswith("params bad"), (bad, why)
    for good in (dict(min_points=2 ** 20), dict(head=2 ** 25, max_span=0, max_step=0, max_slope2=0), dict(max_slope2=2 ** 31 - 1)):
        assert isinstance(emu({**ok, **good}, []), list), good
