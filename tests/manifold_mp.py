"""The filter's manifold rules (SO3 x2, S2, vect x5) stated once more in 50-digit mpmath arithmetic.

Not the smooth functions: the RULES the oracle (oracle/lv_oracle.cpp) and the device (lv_manifold.hpp) both restate, branch
for branch — the three-term Taylor pair of cos_sinc_sqrt below 2^-13, the clamp of the log's vector norm, atan (not atan2) of
nv / w, the pole branch of the S2 basis, the 3.1415926 exit of the S2 difference.  Inputs are doubles (exact in mpmath), every
branch is decided on the 50-digit values, results are rounded to double only by the caller.  So `oracle - this` is the oracle's
own rounding error, and `device - this` the device's, as long as no input sits within rounding of a branch bound (the case
table keeps its cases a per cent away from them)."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50

# the constants are the DOUBLES the two restatements hold, not the decimals they were written as
TOL = mp.mpf(1e-11)                    # MTK::tolerance<double>()
S2_LEN = mp.mpf(98090.0 / 10000.0)     # MTK::S2<double, 98090, 10000, 1>
TAYLOR_N_BOUND = mp.mpf(2) ** -13      # sqrt(sqrt(DBL_EPSILON))
PI_EXIT = mp.mpf(3.1415926)            # the literal of the S2 difference's exit


def _v(a):
    return [mp.mpf(float(t)) for t in np.asarray(a, np.float64).ravel()]


def _f(a):
    return np.array([float(t) for t in a])


def cos_sinc_sqrt(x2):
    if x2 >= TAYLOR_N_BOUND:
        x = mp.sqrt(x2)
        return mp.cos(x), mp.sin(x) / x
    return 1 - x2 / 2 + x2 ** 2 / 24 - x2 ** 3 / 720, 1 - x2 / 6 + x2 ** 2 / 120 - x2 ** 3 / 5040


def so3_exp(v, scale=1):
    half = mp.mpf(scale) / 2
    c, s = cos_sinc_sqrt(half * half * (v[0] ** 2 + v[1] ** 2 + v[2] ** 2))
    return [s * half * v[0], s * half * v[1], s * half * v[2], c]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_to_rot(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def mat_vec(A, v):
    return [sum(A[i][j] * v[j] for j in range(len(v))) for i in range(len(A))]


def so3_log(q):
    nv = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    if nv < TOL:
        nv = TOL
    s = 2 / nv * mp.atan(nv / q[3])
    return [s * q[0], s * q[1], s * q[2]]


def hat(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def A_matrix(v):
    n2 = v[0] ** 2 + v[1] ** 2 + v[2] ** 2
    n = mp.sqrt(n2)
    eye = [[mp.mpf(i == j) for j in range(3)] for i in range(3)]
    if n < TOL:
        return eye
    H = hat(v)
    HH = [[sum(H[i][k] * H[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    c1, c2 = (1 - mp.cos(n)) / n2, (1 - mp.sin(n) / n) / n2
    return [[eye[i][j] + c1 * H[i][j] + c2 * HH[i][j] for j in range(3)] for i in range(3)]


def s2_Bx(vec):
    """3 x 2."""
    if vec[0] + S2_LEN > TOL:
        d = S2_LEN + vec[0]
        B = [[-vec[1], -vec[2]], [S2_LEN - vec[1] * vec[1] / d, -vec[2] * vec[1] / d], [-vec[2] * vec[1] / d, S2_LEN - vec[2] * vec[2] / d]]
        return [[e / S2_LEN for e in r] for r in B]
    return [[mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(-1)], [mp.mpf(1), mp.mpf(0)]]


def s2_boxplus(vec, d):
    Bu = mat_vec(s2_Bx(vec), d)
    return mat_vec(quat_to_rot(so3_exp(Bu, 1)), vec)


def s2_boxminus(vec, other):
    hv = mat_vec(hat(vec), other)
    v_sin = mp.sqrt(hv[0] ** 2 + hv[1] ** 2 + hv[2] ** 2)
    v_cos = vec[0] * other[0] + vec[1] * other[1] + vec[2] * other[2]
    theta = mp.atan2(v_sin, v_cos)
    if v_sin < TOL:
        return [PI_EXIT, mp.mpf(0)] if abs(theta) > TOL else [mp.mpf(0), mp.mpf(0)]
    Bx = s2_Bx(other)
    t = mat_vec(hat(other), vec)
    f = theta / v_sin
    return [f * (Bx[0][j] * t[0] + Bx[1][j] * t[1] + Bx[2][j] * t[2]) for j in range(2)]


def boxplus(x, d):
    """State (26 doubles) boxplus tangent (23 doubles) -> 26 mpf."""
    x, d = _v(x), _v(d)
    o = list(x)
    for i in range(3):
        o[i] = x[i] + d[i]
    o[3:7] = quat_mul(x[3:7], so3_exp(d[3:6]))
    o[7:11] = quat_mul(x[7:11], so3_exp(d[6:9]))
    for s, t in ((11, 9), (14, 12), (17, 15), (20, 18)):
        for i in range(3):
            o[s + i] = x[s + i] + d[t + i]
    o[23:26] = s2_boxplus(x[23:26], d[21:23])
    return o


def boxminus(x, other):
    """x boxminus other -> 23 mpf."""
    x, o = _v(x), _v(other)
    d = [mp.mpf(0)] * 23
    for i in range(3):
        d[i] = x[i] - o[i]
    conj = lambda q: [-q[0], -q[1], -q[2], q[3]]
    d[3:6] = so3_log(quat_mul(conj(o[3:7]), x[3:7]))
    d[6:9] = so3_log(quat_mul(conj(o[7:11]), x[7:11]))
    for s, t in ((11, 9), (14, 12), (17, 15), (20, 18)):
        for i in range(3):
            d[t + i] = x[s + i] - o[s + i]
    d[21:23] = s2_boxminus(x[23:26], o[23:26])
    return d


def predict_state(x, dt, acc, gyro):
    """The state half of esekf::predict with the LIMO-Velo process model: x.oplus(f, dt).  Only pos, rot, vel change; the flow
    of offset_R_L_I and of gravity is zero, and exp(0) is the identity exactly, in every arithmetic."""
    x, acc, gyro, dt = _v(x), _v(acc), _v(gyro), mp.mpf(float(dt))
    o = list(x)
    omega = [gyro[i] - x[17 + i] for i in range(3)]
    a_in = mat_vec(quat_to_rot(x[3:7]), [acc[i] - x[20 + i] for i in range(3)])
    for i in range(3):
        o[i] = x[i] + x[14 + i] * dt
        o[14 + i] = x[14 + i] + (a_in[i] + x[23 + i]) * dt
    o[3:7] = quat_mul(x[3:7], so3_exp(omega, dt))
    return o


def err(a, b_mp):
    """max |a - b| of a double array against mpf values, as a float."""
    a = np.asarray(a, np.float64).ravel()
    return float(max(abs(mp.mpf(float(s)) - t) for s, t in zip(a, b_mp)))


to_float = _f
