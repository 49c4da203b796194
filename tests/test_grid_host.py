"""The host-and-device part of limo-velo_amd/csrc/lv_grid.hpp (cell index and inverse, inside test, the cell of a world point, the
projection of a column, the LDS tile with its halo: what the kernels of the four occupancy tools run) compiled with g++ and
-fsanitize=address,undefined through tests/emu/hip/hip_runtime.h: tests/emu/grid_emu.cpp runs one case per call.  Held to numpy
(tests/grid_ref.py, tests/occupancy_ref.py) by equality, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import grid_ref as gr
import occupancy_ref as ocr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
SHAPES = [(32, 32, 1), (8, 8, 8), (32, 8, 4)]   # the planner's and the frontier's planar tile, the planner's 3-D, the frontier's 3-D


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("grid_host") / "grid_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "grid_emu.cpp"), "-o", str(exe)])

    def run(case, text):
        out = subprocess.run([str(exe), case], input=(text + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
        return [ln.split() for ln in out.strip().split("\n")]

    return run


@pytest.mark.parametrize("dims", [(1, 1, 1), (33, 5, 3), (1024, 2, 2), (2, 1024, 2)])
def test_cell_index_round_trip(emu, dims):
    nx, ny, nz = dims
    out = emu("cells", _ints(dims))
    assert out[0] == ["cells", str(nx * ny * nz)]
    got = np.array(out[1:], np.int64)
    k, j, i = np.unravel_index(np.arange(nx * ny * nz), (nz, ny, nx))   # x fastest
    assert np.array_equal(got[:, :3], np.stack([i, j, k], axis=1))
    assert np.array_equal(got[:, 3], np.arange(nx * ny * nz))             # grid_at(grid_ijk(c)) == c, for every cell


def test_inside_at_the_borders(emu):
    dims = (33, 5, 3)
    probes = [(0, 0, 0), (32, 4, 2), (16, 2, 1)]
    for a in range(3):
        for v in (-1, dims[a], -2 ** 31, 2 ** 31 - 1):
            p = [16, 2, 1]
            p[a] = v
            probes.append(tuple(p))
    got = [int(ln[0]) for ln in emu("inside", _ints(dims) + " %d " % len(probes) + _ints(probes))]
    assert got == [int(all(0 <= p[a] < dims[a] for a in range(3))) for p in probes]
    assert got[:3] == [1, 1, 1] and not any(got[3:])


@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("origin,resolution", [((-1.0, 2.0, 0.5), 0.5), ((-51.2, -51.2, -3.2), 0.2)])
def test_cell_of_a_point(emu, origin, resolution, planar):
    dims = (33, 5, 3)
    pts = gr.probe_points(origin, resolution, dims)
    if planar:   # a z that would be refused in 3-D must be accepted: NaN, inf, far off
        extra = np.repeat(pts[:1], 3, axis=0)
        extra[:, 2] = [np.nan, np.inf, 1e30]
        pts = np.concatenate([pts, extra])
    out = emu("cell_of", " ".join([_bits(origin), _bits([resolution]), _ints(dims), str(planar), str(len(pts)), _bits(pts)]))
    got = np.array(out, np.int64)
    ok, cell = gr.cell_of(origin, resolution, dims, bool(planar), pts)
    assert np.array_equal(got[:, 0].astype(bool), ok)
    assert np.array_equal(got[:, 1:], cell)
    # the probes do what they are there for: every cell is met, and each kind of refusal occurs
    n_cells = dims[0] * dims[1] * (1 if planar else dims[2])
    assert len(np.unique(gr.at(dims, cell[ok]))) == n_cells
    qf = ocr.quant_f(pts, origin, resolution)
    axes = 2 if planar else 3
    with np.errstate(all="ignore"):
        assert np.any(np.isnan(qf[:, :axes])) and np.any(np.isinf(qf[:, :axes])) and np.any(np.abs(qf[:, :axes]) == ocr.Q_LIMIT)
        assert np.any((qf[:, :axes] < 0) & (qf[:, :axes] >= -256)) and np.any(qf[:, 0] == dims[0] * 256)   # just below the origin; on the far face
    if planar:
        assert ok[-3:].all() and np.array_equal(cell[-3:], np.repeat(cell[:1], 3, axis=0)) and not np.any(cell[:, 2])
    else:
        assert np.all(ok[:n_cells]) and np.array_equal(gr.at(dims, cell[:n_cells]), np.arange(n_cells))   # the centres, in order


def _project(L, k_lo, k_hi, l_occ, l_free):
    prm = dict(nx=L.shape[2], ny=L.shape[1], nz=L.shape[0], l_occ=l_occ, l_free=l_free)
    return ocr.project(prm, L, k_lo, k_hi).reshape(-1)


@pytest.mark.parametrize("k_lo,k_hi,band", [(1, 3, (1, 3)), (-4, 99, (0, 4)), (0, 0, (0, 0)), (5, 9, (5, 4)), (-7, -1, (0, -1))])
def test_band_and_column(emu, k_lo, k_hi, band):
    nz, ny, nx = 5, 3, 7
    l_occ, l_free = F(0.4), F(-0.4)
    rng = np.random.default_rng(11)
    # every mixture of NaN, free, occupied and in-between within a column, the thresholds themselves included
    L = rng.choice(np.array([np.nan, -2.0, -0.4, -0.39999998, 0.0, 0.39999998, 0.4, 3.5], F), size=(nz, ny, nx)).astype(F)
    L[:, 0, 0] = np.nan
    L[:, 0, 1] = [np.nan, -2.0, np.nan, 3.5, np.nan]
    L[:, 0, 2] = [3.5, np.nan, np.nan, np.nan, -2.0]
    out = emu("project", " ".join([str(nz), str(ny * nx), str(k_lo), str(k_hi), _bits([l_occ]), _bits([l_free]), _bits(L)]))
    assert out[0] == ["band", str(band[0]), str(band[1])]
    got = np.array([int(ln[0]) for ln in out[1:]])
    want = _project(L, k_lo, k_hi, l_occ, l_free)
    assert np.array_equal(got, want)
    if band[0] > band[1]:
        assert np.all(got == -1)
    elif band == (0, 4):
        assert set(got) == {-1, 0, 100} and got[0] == -1 and got[1] == 100 and got[2] == 100


@pytest.mark.parametrize("shape", SHAPES)
def test_halo_tile(emu, shape):
    tx, ty, tz = shape
    out = emu("tile", _ints(shape))
    hz = 1 if tz > 1 else 0
    lx, ly, lz = tx + 2, ty + 2, tz + 2 * hz
    assert out[0] == ["dims"] + [str(v) for v in (hz, lx, ly, lz, tx * ty * tz, lx * ly * lz)]
    box = np.array([ln[1:] for ln in out if ln[0] == "box"], np.int64)
    lanes = np.array([ln[1:] for ln in out if ln[0] == "lane"], np.int64)
    # at: the haloed local box onto [0, LCELLS), one to one, x fastest; halo_of inverts it
    k, j, i = np.unravel_index(np.arange(lx * ly * lz), (lz, ly, lx))
    assert np.array_equal(box[:, :3], np.stack([i - 1, j - 1, k - hz], axis=1))
    assert np.array_equal(box[:, 3], np.arange(lx * ly * lz))
    assert np.array_equal(box[:, 4:], box[:, :3])
    # local_of: 256 lanes x NPT meet every interior cell exactly once; consecutive lanes are consecutive in x
    npt = tx * ty * tz // 256
    assert tx * ty * tz % 256 == 0 and len(lanes) == 256 * npt
    c = lanes[:, 0] + 256 * lanes[:, 1]
    assert np.array_equal(np.sort(c), np.arange(tx * ty * tz))
    assert np.array_equal((lanes[:, 4] * ty + lanes[:, 3]) * tx + lanes[:, 2], c)
    assert np.all((lanes[:, 2:] >= 0) & (lanes[:, 2:] < np.array(shape)))


@pytest.mark.parametrize("dims", [(33, 5, 3), (70, 70, 1)])
@pytest.mark.parametrize("shape", SHAPES)
def test_tiles_cover_the_grid(emu, shape, dims):
    out = emu("tiles", _ints(shape) + " " + _ints(dims))
    per_axis = [-(-dims[a] // shape[a]) for a in range(3)]
    assert out[0] == ["tiles", str(per_axis[0] * per_axis[1] * per_axis[2])]
    t = np.array(out[1:], np.int64)
    assert len(t) == int(out[0][1])
    # every cell of the grid lies in exactly one tile's interior, and no tile is empty
    owner = np.zeros(dims[::-1], np.int64)
    for tx, ty, tz in t:
        x0, y0, z0 = tx * shape[0], ty * shape[1], tz * shape[2]
        assert x0 < dims[0] and y0 < dims[1] and z0 < dims[2]
        owner[z0:z0 + shape[2], y0:y0 + shape[1], x0:x0 + shape[0]] += 1
    assert np.all(owner == 1)
    assert np.array_equal((t[:, 2] * per_axis[1] + t[:, 1]) * per_axis[0] + t[:, 0], np.arange(len(t)))   # tile t, x fastest
