"""The rule of ray casting and view gain (include/limovelo_hip.h "Ray casting") in numpy, on top of tests/occupancy_ref.py: what
tests/test_occ_ray_host.py holds the host build of lv_ray.hpp to and tests/test_gpu_occ_ray.py the kernels, field for field.  The
quantisations are occupancy_ref's (quant_f, view_origin, returns); the walk here is stated again, vectorised over the rays in
int64, because it must also say across which axis and at which fraction every cell is entered (check_walk holds its cells to
occupancy_ref.walk's)."""
import numpy as np

import occupancy_ref as ocr

F = np.float32
IGNORED, CLEAR, STOPPED = 0, 1, 2
OTHER, FREE, OCCUPIED, UNKNOWN = 0, 1, 2, 3
RESULT_FIELDS = ("status", "cell", "steps", "axis", "n_free", "n_unknown", "num", "den")
RESULT_DTYPE = np.dtype([(f, np.int32) for f in RESULT_FIELDS])


def states(prm, L):
    """[nz, ny, nx] uint8: FREE iff L <= l_free, OCCUPIED iff L >= l_occ, UNKNOWN iff NaN, else OTHER."""
    L = np.asarray(L, F)
    with np.errstate(all="ignore"):
        s = np.where(L <= F(prm["l_free"]), FREE, OTHER)
        s = np.where(L >= F(prm["l_occ"]), OCCUPIED, s)
    return np.where(np.isnan(L), UNKNOWN, s).astype(np.uint8)


def walk(qs, qe):
    """Yields, for s = 0, 1, ...: (has [m] bool, cells [m, 3], axis [m], num [m], den [m]) — whether ray i has a cell c_s (s <= S_i),
    that cell, and how it was entered (s = 0: axis -1, num 0, den 1).  qs [3] or [m, 3], qe [m, 3], int64 sub-units."""
    qe = np.asarray(qe, np.int64).reshape(-1, 3)
    qs = np.broadcast_to(np.asarray(qs, np.int64), qe.shape)
    m = len(qe)
    d = qe - qs
    ad = np.abs(d)
    sg = np.sign(d)
    v = (qs >> 8).copy()
    r = np.abs((qe >> 8) - v)
    n = np.where(sg > 0, ((v + 1) << 8) - qs, np.where(sg < 0, qs - (v << 8), 0))
    total = r.sum(axis=1)
    axis = np.full(m, -1, np.int64)
    num = np.zeros(m, np.int64)
    den = np.ones(m, np.int64)
    s = 0
    rows = np.arange(m)
    while True:
        has = total >= s
        if not has.any():
            return
        yield has, v.copy(), axis.copy(), num.copy(), den.copy()
        # the axis of the next step: among those with steps left the least n_a / ad_a, ties to x, then y, then z
        a = np.full(m, -1, np.int64)
        for b in range(3):
            can = r[:, b] > 0
            ia = np.maximum(a, 0)
            keep = n[rows, ia] * ad[:, b] <= n[:, b] * ad[rows, ia]   # a stays: it comes first, or ties
            a = np.where(can & ((a < 0) | ~keep), b, a)
        go = np.nonzero(a >= 0)[0]
        ax = a[go]
        axis[go], num[go], den[go] = ax, n[go, ax], ad[go, ax]
        v[go, ax] += sg[go, ax]
        n[go, ax] += ocr.Q
        r[go, ax] -= 1
        s += 1


def check_walk(qs, qe):
    """The cells of walk() are those of occupancy_ref.walk, ray for ray; and 0 <= num <= den on every step."""
    qe = np.asarray(qe, np.int64).reshape(-1, 3)
    steps, ve = ocr.walk(qs, qe)
    mine = list(walk(qs, qe))
    total = np.abs((qe >> 8) - (np.broadcast_to(np.asarray(qs, np.int64), qe.shape) >> 8)).sum(axis=1)
    assert len(mine) == len(steps) + 1
    for s, (has, cells, axis, num, den) in enumerate(mine):
        assert np.array_equal(has, total >= s)
        if s < len(steps):
            alive = steps[s][1]
            assert np.array_equal(alive, total > s) and np.array_equal(cells[alive], steps[s][0][alive])
        last = total == s
        assert np.array_equal(cells[last], ve[last])
        if s:
            assert np.all((axis[has] >= 0) & (num[has] >= 0) & (num[has] <= den[has]))


def _inside(prm, c):
    return (c[:, 0] >= 0) & (c[:, 0] < prm["nx"]) & (c[:, 1] >= 0) & (c[:, 1] < prm["ny"]) & (c[:, 2] >= 0) & (c[:, 2] < prm["nz"])


def _linear(prm, c):
    return (c[:, 2] * prm["ny"] + c[:, 1]) * prm["nx"] + c[:, 0]


def cast_q(prm, st, qs, qe, stop_unknown=False, seen=None):
    """The results [m] (RESULT_DTYPE) of the rays qs -> qe in sub-units over the states st.  seen ([nz, ny, nx] bool, optional) gets
    every in-grid cell that lies before a ray's stop."""
    qe = np.asarray(qe, np.int64).reshape(-1, 3)
    m = len(qe)
    out = np.zeros(m, RESULT_DTYPE)
    done = np.zeros(m, bool)
    nf = np.zeros(m, np.int64)
    nu = np.zeros(m, np.int64)
    total = np.zeros(m, np.int64)
    for s, (has, cells, axis, num, den) in enumerate(walk(qs, qe)):
        total[has] = s
        idx = np.nonzero(has & ~done & _inside(prm, cells))[0]
        c = cells[idx]
        sc = st[c[:, 2], c[:, 1], c[:, 0]]
        stop = (sc == OCCUPIED) | ((sc == UNKNOWN) & bool(stop_unknown))
        h = idx[stop]
        out["status"][h], out["cell"][h], out["steps"][h], out["axis"][h] = STOPPED, _linear(prm, c[stop]), s, axis[h]
        out["num"][h], out["den"][h], out["n_free"][h], out["n_unknown"][h] = num[h], den[h], nf[h], nu[h]
        done[h] = True
        p = idx[~stop]
        nf[p] += sc[~stop] == FREE
        nu[p] += sc[~stop] == UNKNOWN
        if seen is not None:
            cp = c[~stop]
            seen[cp[:, 2], cp[:, 1], cp[:, 0]] = True
    clear = np.nonzero(~done)[0]
    ve = qe[clear] >> 8
    out["status"][clear] = CLEAR
    out["cell"][clear] = np.where(_inside(prm, ve), _linear(prm, ve), -1)
    out["steps"][clear], out["axis"][clear], out["num"][clear], out["den"][clear] = total[clear], -1, 1, 1
    out["n_free"][clear], out["n_unknown"][clear] = nf[clear], nu[clear]
    return out


def ends(prm, frm, to):
    """(ok [n] bool, qs [n, 3], qe [n, 3] int64; zeros where not ok): `from` by the origin rule, `to` by the returns' quantisation."""
    frm = np.asarray(frm, F).reshape(-1, 3)
    to = np.asarray(to, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = (frm - np.asarray(prm["origin"], F)) / F(prm["resolution"])
        ok = np.all(np.abs(c) < ocr.T_LIMIT, axis=1)
        fs = np.floor(c * F(ocr.Q))
        fe = ocr.quant_f(to, prm["origin"], prm["resolution"])
        ok &= np.all(np.abs(fe) < ocr.Q_LIMIT, axis=1)
    qs = np.where(ok[:, None], fs, 0).astype(np.int64)
    qe = np.where(ok[:, None], fe, 0).astype(np.int64)
    return ok, qs, qe


def raycast(prm, L, frm, to, stop_unknown=False):
    """lv_occ_raycast: [n] RESULT_DTYPE."""
    ok, qs, qe = ends(prm, frm, to)
    out = np.zeros(len(ok), RESULT_DTYPE)
    out["cell"] = -1
    if ok.any():
        out[ok] = cast_q(prm, states(prm, L), qs[ok], qe[ok], stop_unknown)
    return out


def range_m(prm, frm, to, res):
    """[n] f64: resolution / 256 * |qe - qs| * num / den for STOPPED rays, inf for CLEAR ones, NaN for IGNORED ones."""
    ok, qs, qe = ends(prm, frm, to)
    length = np.sqrt(((qe - qs).astype(np.float64) ** 2).sum(axis=1))
    out = np.full(len(ok), np.nan)
    out[res["status"] == CLEAR] = np.inf
    h = res["status"] == STOPPED
    out[h] = np.float64(F(prm["resolution"])) / 256.0 * length[h] * res["num"][h] / res["den"][h]
    return out


def view_gain(prm, L, views):
    """lv_occ_view_gain: [n_views, 4] uint64 over views = [(R, t, pattern end points)]."""
    st = states(prm, L)
    out = np.zeros((len(views), 4), np.uint64)
    for v, (R, t, pts) in enumerate(views):
        qs = ocr.view_origin(prm, t)
        pts = np.asarray(pts, F).reshape(-1, 3)
        if qs is None or len(pts) == 0:
            continue
        qe, _ = ocr.returns(prm, R, t, pts)
        if len(qe) == 0:
            continue
        seen = np.zeros(st.shape, bool)
        res = cast_q(prm, st, qs, qe, False, seen)
        out[v] = [len(qe), np.sum(res["status"] == STOPPED), np.sum(seen & (st == UNKNOWN)), np.sum(seen & (st == FREE))]
    return out
