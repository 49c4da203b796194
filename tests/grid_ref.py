"""The grid arithmetic of limo-velo_amd/csrc/lv_grid.hpp restated in numpy: what tests/test_grid_host.py holds the host build of
the header to and tests/test_gpu_occ_grid.py the three tools that share its point-to-cell rule.  The quantisation is
tests/occupancy_ref.py's."""
import numpy as np

import occupancy_ref as ocr

F = np.float32


def cell_of(origin, resolution, dims, planar, pts):
    """(ok [n] bool, cell [n, 3] int64 (i, j, k), zeros where not ok) of the world points pts [n, 3]: per axis quant_f, rejected when
    |q| >= 2^24 or NaN, then q >> 8 and the inside test.  planar: z is neither quantised nor tested, k = 0."""
    qf = ocr.quant_f(np.asarray(pts, F).reshape(-1, 3), origin, resolution)
    if planar:
        qf[:, 2] = F(0)
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < ocr.Q_LIMIT, axis=1)   # (NaN fails too)
    v = np.where(ok[:, None], qf, 0).astype(np.int64) >> 8
    n = np.array(dims, np.int64)
    if planar:
        n[2] = 1
    ok &= np.all((v >= 0) & (v < n), axis=1)
    return ok, np.where(ok[:, None], v, 0)


def at(dims, cell):
    """The linear index of cells [n, 3] = (i, j, k): x fastest."""
    cell = np.asarray(cell, np.int64)
    return (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0]


def probe_points(origin, resolution, dims):
    """[n, 3] f32 world points round a grid: every cell centre; per axis every cell face (the far face included), one ulp either
    side of both border faces, a little below the origin, NaN and +-inf, the first coordinate whose quantisation reaches 2^24 and
    the last one below it; and one point far off on every axis."""
    o, r, n = np.asarray(origin, F), F(resolution), np.asarray(dims)
    k, j, i = np.meshgrid(*(np.arange(m) for m in n[::-1]), indexing="ij")
    centres = (o + (np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(F) + F(0.5)) * r).astype(F)
    mid = (o + (n // 2 + F(0.5)) * r).astype(F)   # a centre: the axes not probed stay inside
    rows = []
    for a in range(3):
        lo, hi = o[a], F(o[a] + F(n[a]) * r)
        vals = [F(o[a] + F(m) * r) for m in range(n[a] + 1)]
        vals += [np.nextafter(lo, F(-np.inf)), np.nextafter(lo, F(np.inf)), np.nextafter(hi, F(-np.inf)), np.nextafter(hi, F(np.inf))]
        vals += [F(lo - r / F(512)), F(lo - F(1e-3)), F(np.nan), F(np.inf), F(-np.inf)]
        vals += [F(o[a] + F(65536) * r), np.nextafter(F(o[a] + F(65536) * r), F(-np.inf)), F(o[a] - F(65536) * r)]
        for v in vals:
            p = mid.copy()
            p[a] = v
            rows.append(p)
    rows.append(np.array([1e9, -1e9, 1e9], F))
    return np.concatenate([centres, np.array(rows, F)]).astype(F)
