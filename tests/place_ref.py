"""numpy statement of the place-recognition rule (include/limovelo_hip.h "Place recognition"): a Scan Context descriptor (Kim & Kim,
IROS 2018) per place and the yaw-searching distance between two of them.

Frame: world axes, origin at the place's centre.  A scan at state x: q = M p, M = R_x R_off composed in f64 (R from each quaternion
as given, every sum left to right) and rounded to f32; each coordinate M0*px + M1*py + M2*pz in f32, left to right.  Its centre is
R_x t_off + pos in f64.  A map place of centre c: q = p - (float)c in f32.
Binning, all in f32: rho = sqrt(qx*qx + qy*qy); a point counts iff rmin <= rho < rmax and v = qz + z_offset > 0;
ring = floor((rho - rmin) / ((rmax - rmin) / n_rings)), sector = floor((atan2(qy, qx) + pi) / (2 pi / n_sectors)), each clamped to
the last index.  A bin holds the largest v of its points (0 when empty); layout ring-major, desc[ring, sector].
Distance for shift s: query column j against place column (j + s) mod n_sectors; a pair is valid when both norms are non-zero;
d(s) = 1 - mean over valid pairs of the cosine (1 when none is valid); a place's distance is min_s d(s), its shift the smallest s
reaching it.  Here in f64.

atan2 is the one operation whose f32 result the device does not share bit for bit, so describe() also reports the bins whose value
a point lying within `tol` of a ring edge, rmin / rmax or a sector edge could change: such a point could land in either of the two
bins, and a bin is undecided when that point's v would exceed what the bin holds without the undecided points."""
from __future__ import annotations

import math

import numpy as np

PI_F = np.float32(math.pi)
DEFAULTS = dict(n_rings=20, n_sectors=60, rmin=0.0, rmax=80.0, z_offset=2.0)


def rot(q) -> np.ndarray:
    x, y, z, w = (float(v) for v in q)
    return np.array([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                     2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                     2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)])


def frame(state):
    """(M [3, 3] f32, centre [3] f64) of a state (26 f64), with the device's order of operations."""
    x = np.asarray(state, np.float64).ravel()
    A, B, t = rot(x[3:7]), rot(x[7:11]), x[11:14]
    M = np.empty(9, np.float32)
    c = np.empty(3)
    for i in range(3):
        for j in range(3):
            M[i * 3 + j] = np.float32(A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j])
        c[i] = A[i * 3] * t[0] + A[i * 3 + 1] * t[1] + A[i * 3 + 2] * t[2] + x[i]
    return M.reshape(3, 3), c


def scan_q(scan_xyz, state) -> np.ndarray:
    """[n, 3] f32: the scan's points in the descriptor frame of state."""
    M, _ = frame(state)
    p = np.asarray(scan_xyz, np.float32)
    q = np.empty_like(p)
    for i in range(3):
        q[:, i] = (M[i, 0] * p[:, 0] + M[i, 1] * p[:, 1]) + M[i, 2] * p[:, 2]
    return q


def map_q(map_xyz, centre) -> np.ndarray:
    return np.asarray(map_xyz, np.float32) - np.asarray(centre, np.float64).astype(np.float32)


def describe(q, prm=None, tol_m: float = 1e-4, tol_rad: float = 1e-4):
    """(desc [n_rings, n_sectors] f32, undecided [n_rings, n_sectors] bool) of the points q ([n, 3] f32, descriptor frame)."""
    p = dict(DEFAULTS, **(prm or {}))
    R, S = int(p["n_rings"]), int(p["n_sectors"])
    rmin, rmax, zo = np.float32(p["rmin"]), np.float32(p["rmax"]), np.float32(p["z_offset"])
    ring_w = np.float32(np.float32(rmax - rmin) / np.float32(R))
    sector_w = np.float32(np.float32(2.0) * PI_F / np.float32(S))
    q = np.asarray(q, np.float32)
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        rho = np.sqrt(qx * qx + qy * qy)
        v = qz + zo
        ok = (rho >= rmin) & (rho < rmax) & (v > 0)
    rho, v, qx, qy = rho[ok], v[ok], qx[ok], qy[ok]
    ring = np.clip(np.floor((rho - rmin) / ring_w), 0, R - 1).astype(np.int64)
    ang64 = np.arctan2(qy.astype(np.float64), qx.astype(np.float64))
    sec = np.clip(np.floor((ang64.astype(np.float32) + PI_F) / sector_w), 0, S - 1).astype(np.int64)
    desc = np.zeros(R * S, np.float32)
    b = ring * S + sec
    np.maximum.at(desc, b, v)

    # points near an edge: the bins they could land in instead
    fr = (rho.astype(np.float64) - float(rmin)) / float(ring_w)
    near_r = np.abs(fr - np.round(fr)) * float(ring_w) < tol_m
    near_bound = (np.abs(rho.astype(np.float64) - float(rmin)) < tol_m) | (np.abs(rho.astype(np.float64) - float(rmax)) < tol_m)
    fs = (ang64 + math.pi) / float(sector_w)
    near_s = np.abs(fs - np.round(fs)) * float(sector_w) < tol_rad
    amb = near_r | near_s | near_bound
    base = np.zeros(R * S, np.float32)
    np.maximum.at(base, b[~amb], v[~amb])
    und = np.zeros(R * S, bool)
    for i in np.nonzero(amb)[0]:
        rings = {ring[i]}
        if near_r[i] or near_bound[i]:
            rr = int(np.round(fr[i]))
            rings |= {min(max(rr - 1, 0), R - 1), min(max(rr, 0), R - 1)}
        secs = {sec[i]}
        if near_s[i]:
            ss = int(np.round(fs[i]))
            secs |= {(ss - 1) % S, ss % S}
        for r_ in rings:
            for s_ in secs:
                if v[i] >= base[r_ * S + s_]:
                    und[r_ * S + s_] = True
    return desc.reshape(R, S), und.reshape(R, S)


def distances(qdesc, pdesc):
    """(dist [n] f64, shift [n] int, d [n, S] f64 for every shift) of the query descriptor [R, S] against places [n, R, S]."""
    Q = np.asarray(qdesc, np.float64)
    P = np.asarray(pdesc, np.float64).reshape(-1, *Q.shape)
    S = Q.shape[1]
    qn = np.sqrt((Q * Q).sum(0))
    pn = np.sqrt((P * P).sum(1))                      # [n, S]
    d = np.empty((len(P), S))
    for s in range(S):
        Ps = np.roll(P, -s, axis=2)                   # Ps[:, :, j] = P[:, :, (j + s) % S]
        pns = np.roll(pn, -s, axis=1)
        dots = np.einsum("rj,nrj->nj", Q, Ps)
        valid = (qn[None, :] > 0) & (pns > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = np.where(valid, dots / (qn[None, :] * pns), 0.0)
        cnt = valid.sum(1)
        d[:, s] = np.where(cnt > 0, 1.0 - cos.sum(1) / np.maximum(cnt, 1), 1.0)
    d = np.maximum(d, 0.0)
    shift = np.argmin(d, axis=1)
    return d[np.arange(len(P)), shift], shift, d


def shift_yaw(shift: int, n_sectors: int) -> float:
    """The yaw of a shift, wrapped to (-pi, pi]."""
    a = shift * 2.0 * math.pi / n_sectors
    a = math.atan2(math.sin(a), math.cos(a))
    return math.pi if a <= -math.pi else a
