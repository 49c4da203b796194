"""The rule of lv_observe (include/limovelo_hip.h "Aiding observations") in plain f64, product by product in the stated summation
order: what tests/test_gpu_observe.py compares the device with, and what tests/test_aiding_ref.py anchors to 50 digits.

An observation is a dict {kind, mask, z (3 or 4), R (3 x 3), lever (3), gate}; the state is the 26 doubles of lv_state, P is
23 x 23.  Every sum starts at 0.0 and adds its terms left to right (Python floats are IEEE doubles; nothing here is handed to a
BLAS that could reorder).  The state's boxplus is the oracle's (oracle.boxplus)."""
import math

import numpy as np

POSITION, VELOCITY_WORLD, VELOCITY_BODY, ATTITUDE = 1, 2, 3, 4
NS = 23
MTK_TOL = 1e-11


def quat_to_rot(q):
    x, y, z, w = (float(t) for t in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def hat(v):
    return [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def so3_log(q):
    nv = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    if nv < MTK_TOL:
        nv = MTK_TOL
    s = 2.0 / nv * math.atan(nv / q[3])
    return [s * q[0], s * q[1], s * q[2]]


def components(mask):
    return [k for k in range(3) if mask >> k & 1]


def model(x, o):
    """y (3), and the blocks of H: [(first column, 3 x 3), ...]."""
    kind = o["kind"]
    x = [float(t) for t in x]
    z = [float(t) for t in np.ravel(o["z"])]
    R = quat_to_rot(x[3:7])
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if kind == POSITION:
        lv = [float(t) for t in o["lever"]]
        Rl = [R[i][0] * lv[0] + R[i][1] * lv[1] + R[i][2] * lv[2] for i in range(3)]
        y = [z[i] - (x[i] + Rl[i]) for i in range(3)]
        hl = hat(lv)
        Hb = [[-(R[i][0] * hl[0][j] + R[i][1] * hl[1][j] + R[i][2] * hl[2][j]) for j in range(3)] for i in range(3)]
        return y, [(0, eye), (3, Hb)]
    if kind == VELOCITY_WORLD:
        return [z[i] - x[14 + i] for i in range(3)], [(12, eye)]
    if kind == VELOCITY_BODY:
        Rt = [[R[j][i] for j in range(3)] for i in range(3)]
        vb = [Rt[i][0] * x[14] + Rt[i][1] * x[15] + Rt[i][2] * x[16] for i in range(3)]
        return [z[i] - vb[i] for i in range(3)], [(12, Rt), (3, hat(vb))]
    if kind == ATTITUDE:
        qc = [-x[3], -x[4], -x[5], x[6]]
        return so3_log(quat_mul(qc, z[:4])), [(3, eye)]
    raise ValueError(kind)


def observe_one(oracle, x, P, o):
    """-> x, P, result {status, rows, nis, y, dx}.  Status 1 and 2 return x and P themselves."""
    comp = components(o["mask"])
    m = len(comp)
    y3, blocks = model(x, o)
    Rfull = np.asarray(o["R"], np.float64).reshape(3, 3)
    Rm = [[float(Rfull[a][b]) for b in comp] for a in comp]
    y = [y3[k] for k in comp]
    Pl = [[float(t) for t in row] for row in np.asarray(P, np.float64)]
    cols = [(c0 + j, b, j) for b, (c0, _) in enumerate(blocks) for j in range(3)]   # the columns of H in summation order
    H = lambda k, b, j: blocks[b][1][comp[k]][j]
    res = dict(status=0, rows=m, nis=0.0, y=np.array(y3), dx=np.zeros(NS))
    PHt = [[0.0] * m for _ in range(NS)]
    for i in range(NS):
        for k in range(m):
            s = 0.0
            for c, b, j in cols:
                s += Pl[i][c] * H(k, b, j)
            PHt[i][k] = s
    S = [[0.0] * m for _ in range(m)]
    for k in range(m):
        for l in range(k + 1):
            s = 0.0
            for c, b, j in cols:
                s += H(k, b, j) * PHt[c][l]
            S[k][l] = s + Rm[k][l]
    L = [[0.0] * m for _ in range(m)]
    for j in range(m):
        d = S[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        if not d > 0.0 or not math.isfinite(d):
            res["status"] = 2
            return x, P, res
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, m):
            t = S[i][j]
            for k in range(j):
                t -= L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    w = [0.0] * m
    for i in range(m):
        t = y[i]
        for k in range(i):
            t -= L[i][k] * w[k]
        w[i] = t / L[i][i]
    nis = 0.0
    for i in range(m):
        nis += w[i] * w[i]
    res["nis"] = nis
    res["S"] = np.array([[S[max(a, b)][min(a, b)] for b in range(m)] for a in range(m)])
    if o["gate"] > 0.0 and nis > o["gate"]:
        res["status"] = 1
        return x, P, res
    K = [[0.0] * m for _ in range(NS)]
    dx = [0.0] * NS
    KR = [[0.0] * m for _ in range(NS)]
    for i in range(NS):
        t = [0.0] * m
        for k in range(m):
            v = PHt[i][k]
            for l in range(k):
                v -= L[k][l] * t[l]
            t[k] = v / L[k][k]
        for k in range(m - 1, -1, -1):
            v = t[k]
            for l in range(k + 1, m):
                v -= L[l][k] * K[i][l]
            K[i][k] = v / L[k][k]
        d = 0.0
        for k in range(m):
            d += K[i][k] * y[k]
        dx[i] = d
        for l in range(m):
            s = 0.0
            for k in range(m):
                s += K[i][k] * Rm[k][l]
            KR[i][l] = s
    A = [[1.0 if i == c else 0.0 for c in range(NS)] for i in range(NS)]
    for i in range(NS):
        for c, b, j in cols:
            s = 0.0
            for k in range(m):
                s += K[i][k] * H(k, b, j)
            A[i][c] = (1.0 if i == c else 0.0) - s
    AP = [[0.0] * NS for _ in range(NS)]
    for i in range(NS):
        for j in range(NS):
            s = 0.0
            for c in range(NS):
                s += A[i][c] * Pl[c][j]
            AP[i][j] = s
    Pn = np.zeros((NS, NS))
    for i in range(NS):
        for j in range(i, NS):
            s = 0.0
            for c in range(NS):
                s += AP[i][c] * A[j][c]
            q = 0.0
            for l in range(m):
                q += KR[i][l] * K[j][l]
            Pn[i, j] = Pn[j, i] = s + q
    res["dx"] = np.array(dx)
    return oracle.boxplus(np.asarray(x, np.float64), np.array(dx)), Pn, res


def observe(oracle, x, P, obs_list):
    """The observations one after the other -> x, P, [result, ...]."""
    x, P = np.array(x, np.float64), np.array(P, np.float64)
    out = []
    for o in obs_list:
        x, P, r = observe_one(oracle, x, P, o)
        out.append(r)
    return x, P, out
