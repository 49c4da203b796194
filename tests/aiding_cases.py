"""The case table of the aiding observations: tests/test_aiding_ref.py anchors tests/aiding_ref.py on it, tests/test_gpu_observe.py
runs the device on it.  A case is {name, x (26), P (23 x 23), obs: [observation dict, ...]}; pure numpy, built once.

Every kind; every mask for POSITION; lever arms of zero and non-zero; rotations of 0.01, 0.3 and 3 rad; gravity beside and at the
pole of its chart; an attitude innovation that moves the rotation past the small-angle branch of the exponential (0.0222 rad); a
gated-out observation; S = 0 (P = 0, R = 0); a batch of eight whose third is gated.  P is dense (every block moves, the
extrinsic rotation and gravity included) and R is of the size of H P H^T, so that S is well conditioned (asserted <= 1e3 by
test_aiding_ref.py)."""
import numpy as np

POSITION, VELOCITY_WORLD, VELOCITY_BODY, ATTITUDE = 1, 2, 3, 4
S2_LEN = 98090.0 / 10000.0
CHI2_3_99 = 11.344866730144373


def quat_exp(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.r_[np.sin(a / 2) * v / a, np.cos(a / 2)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def state(angle, grav=(0.0, 0.0, -S2_LEN)):
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    x = np.zeros(26)
    x[0:3] = [1.25, -2.5, 0.5]
    x[3:7] = quat_exp(axis * angle)
    x[7:11] = quat_exp([0.02, -0.03, 0.05])
    x[11:14] = [0.05, -0.02, 0.1]
    x[14:17] = [1.5, -0.3, 0.05]
    x[17:20] = [0.01, -0.02, 0.005]
    x[20:23] = [0.05, 0.02, -0.03]
    g = np.asarray(grav, np.float64)
    x[23:26] = g * (S2_LEN / np.linalg.norm(g))
    return x


def dense_P(seed, scale=1e-2):
    """SPD with cross terms between every pair of blocks: eigenvalues within scale * [0.5, ~1.6]."""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(23, 23))
    P = scale * (0.5 * np.eye(23) + 0.5 * (B @ B.T) / 23)
    return (P + P.T) / 2


def cov(seed, scale=1e-2):
    rng = np.random.default_rng(1000 + seed)
    B = rng.normal(size=(3, 3))
    R = scale * (np.eye(3) + 0.3 * (B @ B.T) / 3)
    return (R + R.T) / 2


def obs(kind, x, seed, mask=7, lever=(0.0, 0.0, 0.0), gate=0.0, innov=None, scale=0.05):
    """An observation whose innovation at x is `innov` (default: a seeded vector of size ~scale)."""
    rng = np.random.default_rng(2000 + seed)
    d = np.asarray(innov, np.float64) if innov is not None else scale * rng.uniform(-1, 1, 3)
    R = quat_rot(x[3:7])
    lever = np.asarray(lever, np.float64)
    if kind == POSITION:
        z = x[0:3] + R @ lever + d
    elif kind == VELOCITY_WORLD:
        z = x[14:17] + d
    elif kind == VELOCITY_BODY:
        z = R.T @ x[14:17] + d
    else:
        z = quat_mul(x[3:7], quat_exp(d))
        z = z / np.linalg.norm(z)
    return dict(kind=kind, mask=mask, z=np.r_[z, np.zeros(4 - len(z))], R=cov(seed), lever=lever, gate=float(gate))


LEVER = (0.3, -0.1, 0.45)
KIND_NAMES = {POSITION: "position", VELOCITY_WORLD: "velworld", VELOCITY_BODY: "velbody", ATTITUDE: "attitude"}


def _build():
    out = []
    seed = 0

    def add(name, x, P, observations):
        out.append(dict(name=name, x=x, P=P, obs=observations))

    for angle in (0.01, 0.3, 3.0):
        for kind in (POSITION, VELOCITY_WORLD, VELOCITY_BODY, ATTITUDE):
            seed += 1
            x = state(angle)
            add(f"{KIND_NAMES[kind]}-rot{angle}", x, dense_P(seed), [obs(kind, x, seed, lever=LEVER if kind == POSITION else (0, 0, 0))])
    for mask in range(1, 7):
        seed += 1
        x = state(0.3)
        add(f"position-mask{mask}", x, dense_P(seed), [obs(POSITION, x, seed, mask=mask, lever=LEVER)])
    for name, kind, mask in (("position-nolever", POSITION, 7), ("barometer", POSITION, 4), ("wheel", VELOCITY_BODY, 1),
                             ("velbody-mask6", VELOCITY_BODY, 6), ("attitude-mask3", ATTITUDE, 3), ("velworld-mask5", VELOCITY_WORLD, 5)):
        seed += 1
        x = state(0.3)
        add(name, x, dense_P(seed), [obs(kind, x, seed, mask=mask)])
    seed += 1
    x = state(0.3, grav=(-1.0, 1e-4, -2e-4))
    add("grav-beside-pole", x, dense_P(seed), [obs(VELOCITY_WORLD, x, seed)])
    seed += 1
    x = state(0.3)
    x[23:26] = (-S2_LEN, 0.0, 0.0)
    add("grav-at-pole", x, dense_P(seed), [obs(POSITION, x, seed, lever=LEVER)])
    seed += 1
    x = state(0.3)   # the innovation moves the rotation by ~0.15 rad: d_so3_exp leaves its small-angle branch
    add("attitude-large", x, dense_P(seed, scale=0.05), [obs(ATTITUDE, x, seed, innov=(0.25, -0.2, 0.15))])
    seed += 1
    x = state(0.3)
    add("gated", x, dense_P(seed), [obs(POSITION, x, seed, lever=LEVER, gate=CHI2_3_99, innov=(2.0, -1.5, 1.0))])
    seed += 1
    x = state(0.3)
    o = obs(VELOCITY_WORLD, x, seed)
    o["R"] = np.zeros((3, 3))
    add("singular", x, np.zeros((23, 23)), [o])
    seed += 1
    x = state(0.3)
    # the observations of the batch are made for the state the batch starts from: the later ones see innovations that the
    # earlier ones have already partly used.  The third is far off and gated.
    kinds = [POSITION, VELOCITY_BODY, VELOCITY_WORLD, ATTITUDE, POSITION, VELOCITY_BODY, ATTITUDE, VELOCITY_WORLD]
    batch = []
    for i, kind in enumerate(kinds):
        far = i == 2
        batch.append(obs(kind, x, seed + i, mask=(7, 1, 7, 7, 4, 7, 3, 5)[i], lever=LEVER if i == 0 else (0, 0, 0),
                         gate=CHI2_3_99 if far else 0.0, innov=(3.0, 2.0, -2.5) if far else None))
    add("batch8", x, dense_P(seed), batch)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def applied(case):
    """Names of the cases whose every observation is expected to be applied are all but these."""
    return case["name"] not in ("gated", "singular", "batch8")
