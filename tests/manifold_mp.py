"""The filter's manifold rules (SO3 x2, S2, vect x5) stated once more in 50-digit mpmath arithmetic.

Not the smooth functions: the RULES the oracle (oracle/lv_oracle.cpp) and the device (lv_manifold.hpp) both restate, branch
for branch — the three-term Taylor pair of cos_sinc_sqrt below 2^-13, the clamp of the log's vector norm, atan (not atan2) of
nv / w, the pole branch of the S2 basis, the 3.1415926 exit of the S2 difference.  Inputs are doubles (exact in mpmath), every
branch is decided on the 50-digit values, results are rounded to double only by the caller.  So `oracle - this` is the oracle's
own rounding error, and `device - this` the device's, as long as no input sits within rounding of a branch bound (the case
table keeps its cases a per cent away from them).

kf_step is one whole pass of the iterated update built from those rules, with upstream's gain in its textbook form and mpmath's
own 23 x 23 inverse: what tests/solve_regimes.py adjudicates the oracle, the device's block form and the device with."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50

# the constants are the DOUBLES the two restatements hold, not the decimals they were written as
TOL = mp.mpf(1e-11)                    # MTK::tolerance<double>()
S2_LEN = mp.mpf(98090.0 / 10000.0)     # MTK::S2<double, 98090, 10000, 1>
TAYLOR_N_BOUND = mp.mpf(2) ** -13      # sqrt(sqrt(DBL_EPSILON))
PI_EXIT = mp.mpf(3.1415926)            # the literal of the S2 difference's exit


def _v(a):
    if isinstance(a, (list, tuple)) and len(a) and isinstance(a[0], mp.mpf):
        return list(a)   # already 50-digit values (kf_step hands its own increment to boxplus unrounded)
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


def s2_Nx_yy(vec):
    """2 x 3:  Bx^T hat(vec) / len^2."""
    Bx, H = s2_Bx(vec), hat(vec)
    return [[sum(Bx[k][i] * H[k][j] for k in range(3)) / S2_LEN / S2_LEN for j in range(3)] for i in range(2)]


def s2_Mx(vec, delta):
    """3 x 2:  -hat(vec) A(Bx delta)^T Bx, and -hat(vec) Bx below the tolerance (the rule's exp_delta is the identity: the
    oracle's note on the integer 1 / 2)."""
    Bx, H = s2_Bx(vec), hat(vec)
    if mp.sqrt(delta[0] ** 2 + delta[1] ** 2) < TOL:
        T = [[-H[i][j] for j in range(3)] for i in range(3)]
    else:
        A = A_matrix(mat_vec(Bx, delta))
        T = [[-sum(H[i][k] * A[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
    return [[sum(T[i][k] * Bx[k][j] for k in range(3)) for j in range(2)] for i in range(3)]


def s2_projection(grav, grav_prop, delta):
    """2 x 2:  Nx(grav) Mx(grav_prop, delta), the S2 block of the update's projections."""
    Nx, Mx = s2_Nx_yy(grav), s2_Mx(grav_prop, delta)
    return [[sum(Nx[i][k] * Mx[k][j] for k in range(3)) for j in range(2)] for i in range(2)]


def projection(seg, grav, grav_prop):
    """The 23 x 23 projection J of one pass: A(seg_rot)^T and A(seg_ext)^T on the two SO3 blocks, the S2 block, identity
    elsewhere.  seg is the tangent the blocks are evaluated at (x [-] x_prop before the solve, dx_ on the terminal pass)."""
    J = mp.eye(23)
    for idx in (3, 6):
        A = A_matrix(seg[idx:idx + 3])
        for i in range(3):
            for j in range(3):
                J[idx + i, idx + j] = A[j][i]
    T = s2_projection(grav, grav_prop, seg[21:23])
    for i in range(2):
        for j in range(2):
            J[21 + i, 21 + j] = T[i][j]
    return J


def _kf_step(x, x_prop, P_prop, rec, R, limits, finalize, keep):
    xd, xp = _v(x), _v(x_prop)
    R = mp.mpf(float(R))
    P = mp.matrix([[mp.mpf(float(t)) for t in row] for row in np.asarray(P_prop, np.float64).reshape(23, 23)])
    HTH = mp.zeros(23, 23)
    HTh = mp.zeros(23, 1)
    for i in range(12):
        HTh[i] = mp.mpf(float(rec["HTh"][i]))
        for j in range(12):
            HTH[i, j] = mp.mpf(float(rec["HTH"][i][j]))
    dx = boxminus(xd, xp)
    J = projection(dx, xd[23:26], xp[23:26])
    dx_new = J * mp.matrix(dx)
    P_ = J * P * J.T
    # P_inv = ((P_ / R)^-1 + E H^T H E^T)^-1, on the kept dofs; rows and columns of the others are zero (their variance is)
    keep = list(range(23)) if keep is None else list(keep)
    n = len(keep)
    sub = lambda M: mp.matrix([[M[a, b] for b in keep] for a in keep])
    if n < 23:
        out = [i for i in range(23) if i not in keep]
        assert all(P[i, j] == 0 for i in out for j in range(23)) and all(HTH[i, j] == 0 for i in out for j in range(23))
    inner = mp.inverse(sub(P_) / R) + sub(HTH)
    small = mp.inverse(inner)
    P_inv = mp.zeros(23, 23)
    for a in range(n):
        for b in range(n):
            P_inv[keep[a], keep[b]] = small[a, b]
    K_h = P_inv * HTh
    K_x = P_inv * HTH          # columns >= 12 are zero
    dxo = K_h + (K_x - mp.eye(23)) * dx_new
    dxo = [dxo[i] for i in range(23)]
    x_new = boxplus(xd, dxo)
    lim = _v(limits)
    conv = all(abs(dxo[i]) <= lim[i] for i in range(23))
    P_out = None
    if finalize:
        J2 = projection(dxo, x_new[23:26], xp[23:26])
        L = J2 * P_ * J2.T
        P_out = L - (J2 * K_x) * (P_ * J2.T)
    return x_new, dxo, conv, P_out


def _result(x_new, dxo, conv, P_out):
    P = None if P_out is None else np.array([[float(P_out[i, j]) for j in range(23)] for i in range(23)])
    return dict(x=_f(x_new), dx=_f(dxo), conv=conv, P=P, x_mp=x_new, dx_mp=dxo, P_mp=P_out)


def kf_step(x, x_prop, P_prop, rec, R, limits, finalize):
    """One pass of the iterated update, the textbook statement of oracle/lv_oracle.cpp::kf_step in 50 digits:
        dx = x [-] x_prop,  dx_new = J dx,  P_ = J P J^T,  P_inv = ((P_ / R)^-1 + E H^T H E^T)^-1  (mpmath's own inverse),
        dx_ = P_inv[:, :12] H^T h + (P_inv[:, :12] H^T H - I) dx_new,  x [+] dx_,  converge = all(|dx_i| <= limits_i),
    and on `finalize` the posterior  J2 P_ J2^T - (J2 K_x) (P_ J2^T)  with J2 the projections at dx_ and the new gravity.
    x, x_prop, P_prop, rec (dict HTH [12, 12], HTh [12]), R and limits are doubles; returns dict(x, dx, conv, P) as doubles
    / bool and x_mp, dx_mp, P_mp, the unrounded values."""
    return _result(*_kf_step(x, x_prop, P_prop, rec, R, limits, finalize, None))


def kf_step_reduced(x, x_prop, P_prop, rec, R, limits, finalize, keep):
    """kf_step solved on the dofs `keep` alone: for a P whose other rows and columns are exactly zero (a dof without variance
    is not estimated), where (P / R)^-1 does not exist.  The limit of kf_step as those variances go to zero: P_inv is zero
    outside keep x keep, so those dofs return -dx_new (zero while they sit at their prediction) and P keeps its zeros."""
    return _result(*_kf_step(x, x_prop, P_prop, rec, R, limits, finalize, keep))


def err_mat(a, b_mp):
    """max |a - b| of a double [23, 23] against an mp matrix, as a float."""
    a = np.asarray(a, np.float64)
    return float(max(abs(mp.mpf(float(a[i, j])) - b_mp[i, j]) for i in range(23) for j in range(23)))


def err(a, b_mp):
    """max |a - b| of a double array against mpf values, as a float."""
    a = np.asarray(a, np.float64).ravel()
    return float(max(abs(mp.mpf(float(s)) - t) for s, t in zip(a, b_mp)))


to_float = _f
