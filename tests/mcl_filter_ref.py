"""The resident localisation filter's rule (include/limovelo_hip.h "Resident localisation filter") in numpy: what
tests/test_mcl_filter_host.py holds the host build of lv_mcl_filter.hpp to and tests/test_gpu_occ_mcl_filter.py the kernels of
lv_mcl_filter.hip, bit for bit.

  draws      np.uint64 arithmetic (it wraps): mix is splitmix64's finaliser with its additive constant; word(seed, epoch, i, j) =
             mix(mix(mix(seed) ^ epoch) ^ ((i << 8) | j)); a normal is the sum of twelve 16-bit fields as an integer G, z = G * 2^-17.
  move       np.float32 operations in the stated order; the sine and cosine are rollout_ref.sincos.
  weigh      mcl_ref.weigh on the resident poses.
  sums       exact int64 numpy sums (w <= 2^20, |q| <= 2^22, K <= 2^20: every sum stays below 2^62), handed on as python integers;
             the decision in python integers.
RefFilterContext offers the seven calls of capi.Context (occ_mcl_filter_*) on a field dict(origin, resolution, s2) of mcl_ref."""
import types

import numpy as np

import mcl_ref as mr
import occupancy_ref as ocr
import rollout_ref as rr

F = np.float32
U = np.uint64
NO_SCORE = mr.NO_SCORE
MASK = 2 ** 64 - 1
PI_F, TWO_PI_F = F(3.14159274), F(6.28318548)
Q_CLAMP = 1 << 22
MAX_K, MAX_SINCE, MAX_EPOCH, MAX_WEIGHT, BLOCK = 1 << 20, 1 << 20, 2 ** 32 - 1, 1 << 20, 256


def mix(x):
    """splitmix64's finaliser with its additive constant, on python integers."""
    z = (int(x) + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix_np(x):
    """mix on an np.uint64 array."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, U) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def base(seed, epoch):
    return mix(mix(seed) ^ int(epoch))


def word(seed, epoch, i, j):
    return mix(base(seed, epoch) ^ ((int(i) << 8) | int(j)))


def resample_draw(seed, epoch):
    return mix(base(seed, epoch) ^ MASK)


def normals_g(seed, epoch, K, first=0):
    """[K, 3] int64: G of the three normals of the particles first .. first + K - 1."""
    b = U(base(seed, epoch))
    i = np.arange(first, first + int(K), dtype=U) << U(8)
    out = np.zeros((int(K), 3), np.int64)
    for n in range(3):
        s = np.zeros(int(K), np.int64)
        for k in range(3):
            w = mix_np(b ^ (i | U(3 * n + k)))
            for f in range(4):
                s += ((w >> U(16 * f)) & U(0xFFFF)).astype(np.int64)
        out[:, n] = 2 * s - 12 * 65535
    return out


def move(poses, seed, epoch, delta, sigma):
    """[K, 4] f32: the poses after the motion update of `epoch`."""
    x = np.array(poses, F).reshape(-1, 4)
    d, s = np.asarray(delta, F), np.asarray(sigma, F)
    z = normals_g(seed, epoch, len(x)).astype(F) * F(2.0 ** -17)
    with np.errstate(all="ignore"):
        r1 = d[0] - z[:, 0] * s[0]
        tr = d[1] - z[:, 1] * s[1]
        r2 = d[2] - z[:, 2] * s[2]
        ok = mr.usable(x[:, 3])
        a = x[:, 3] + r1
        ok_a = ok & mr.usable(a)
        sn, cs = rr.sincos(np.where(ok_a, a, F(0)))
        nx = x[:, 0] + tr * cs
        ny = x[:, 1] + tr * sn
        th = a + r2
        th = np.where(th >= PI_F, th - TWO_PI_F, th)
        th = np.where(th < -PI_F, th + TWO_PI_F, th)
    out = x.copy()
    out[:, 0] = np.where(ok_a, nx, x[:, 0])
    out[:, 1] = np.where(ok_a, ny, x[:, 1])
    # (through the bits: an untouched NaN heading keeps its payload)
    bits = np.where(ok_a, th.astype(F).view(np.uint32), np.where(ok, a.astype(F).view(np.uint32), x[:, 3].view(np.uint32)))
    out[:, 3] = bits.astype(np.uint32).view(F)
    return out


def accumulate(acc, score):
    acc, score = np.asarray(acc, U), np.asarray(score, U)
    gone = (acc == U(NO_SCORE)) | (score == U(NO_SCORE))
    return np.where(gone, U(NO_SCORE), np.where(gone, U(0), acc) + np.where(gone, U(0), score))


def weights(acc, wtable, shift):
    """(w [K] int64, s_min; -1 when no particle is eligible)."""
    acc = np.asarray(acc, U)
    wt = np.asarray(wtable, np.uint32).astype(np.int64)
    ok = acc != U(NO_SCORE)
    if not ok.any():
        return np.zeros(len(acc), np.int64), -1
    s_min = int(acc[ok].min())
    d = (np.where(ok, acc, U(s_min)) - U(s_min)) >> U(int(shift))
    return np.where(ok, wt[np.minimum(d, U(len(wt) - 1)).astype(np.int64)], 0), s_min


def terms(field, poses):
    """(q [K, 5] int64: the quantised x, y, z and the heading's sine and cosine; clamped [K] bool)."""
    x = np.asarray(poses, F).reshape(-1, 4)
    qf = ocr.quant_f(x[:, :3], field["origin"], field["resolution"])
    with np.errstate(all="ignore"):
        fin = np.isfinite(qf)
        big = fin & (np.abs(qf) > F(Q_CLAMP))
        q3 = np.where(fin, np.clip(qf, -F(Q_CLAMP), F(Q_CLAMP)), F(0)).astype(np.int64)
        ok = mr.usable(x[:, 3])
        sn, cs = rr.sincos(np.where(ok, x[:, 3], F(0)))
        qs = np.where(ok, np.rint(sn * F(1048576.0)), F(0)).astype(np.int64)
        qc = np.where(ok, np.rint(cs * F(1048576.0)), F(0)).astype(np.int64)
    return np.concatenate([q3, qs[:, None], qc[:, None]], axis=1), (~fin | big).any(axis=1)


def decide(mode, W, sum_w2, K, num, den):
    if mode == 0 or W <= 0:
        return False
    if mode == 2:
        return True
    return int(W) * int(W) * int(den) < int(num) * int(K) * int(sum_w2)


def ancestors(w, draw):
    """[K] int64 of the systematic resampling with M = K (W > 0)."""
    C = np.cumsum(np.asarray(w, np.int64))
    K, W = len(C), int(C[-1])
    r = int(draw) % W
    t = (np.arange(K, dtype=np.int64) * W + r) // K
    return np.searchsorted(C, t, side="right").astype(np.int64)


def rparams(**kw):
    """lv_mcl_resample_params with the defaults of lv_default_mcl_resample_params."""
    p = dict(shift=0, mode=1, below_num=1, below_den=2)
    p.update(kw)
    return types.SimpleNamespace(**p)


def stats_dict(s):
    """A stats record (the reference's or capi.MclFilterStats) as a dict of python numbers; origin and resolution by their bits."""
    return dict(W=int(s.W), sum_w2=int(s.sum_w2), s_min=int(s.s_min), S=[int(v) for v in s.S], n_eligible=int(s.n_eligible),
                n_clamped=int(s.n_clamped), resampled=int(s.resampled), epoch=int(s.epoch), since_resample=int(s.since_resample),
                origin=[int(np.array(v, F).view(np.uint32)) for v in s.origin], resolution=int(np.array(s.resolution, F).view(np.uint32)))


class StateError(RuntimeError):
    """LV_ESTATE of the reference context."""


class RefFilterContext:
    """The seven calls on a field of mcl_ref (occ_mcl_weigh too, so that mcl.step runs on it as on mcl_ref.RefContext)."""

    def __init__(self, field):
        self.field = field
        self.x = None

    occ_mcl_weigh = mr.RefContext.occ_mcl_weigh

    def _need(self):
        if self.x is None:
            raise StateError("no particles: call lv_occ_mcl_filter_set first")

    def occ_mcl_filter_set(self, poses, seed):
        x = np.array(poses, F).reshape(-1, 4)
        if not 1 <= len(x) <= MAX_K:
            raise ValueError("K: 1..2^20")
        self.x, self.seed, self.epoch, self.since = x, int(seed), 0, 0
        self.acc, self.n_in = np.zeros(len(x), U), np.zeros(len(x), np.uint32)

    def occ_mcl_filter_move(self, delta, sigma):
        self._need()
        if self.epoch == MAX_EPOCH:
            raise StateError("the epoch has reached 2^32 - 1: call lv_occ_mcl_filter_set again")
        self.x = move(self.x, self.seed, self.epoch, delta, sigma)
        self.epoch += 1

    def occ_mcl_filter_weigh(self, beams, table, params=None, want_best=True):
        self._need()
        if self.since == MAX_SINCE - 1:
            raise StateError("2^20 scans since the last resampling: call lv_occ_mcl_filter_resample")
        mp = mr.mparams() if params is None else {f: getattr(params, f) for f in mr.mparams()}
        out = mr.weigh(self.field, mp, self.x, beams, table)
        self.acc, self.n_in = accumulate(self.acc, out["score"]), out["n_in"]
        self.since += 1
        return out["best"] if want_best else None

    def occ_mcl_filter_resample(self, wtable, params=None, want_ancestors=True):
        self._need()
        if self.epoch == MAX_EPOCH:
            raise StateError("the epoch has reached 2^32 - 1: call lv_occ_mcl_filter_set again")
        p = rparams() if params is None else params
        K = len(self.x)
        w, s_min = weights(self.acc, wtable, p.shift)
        q, clamped = terms(self.field, self.x)
        W, sum_w2, n_eligible = int(w.sum()), int((w * w).sum()), int((self.acc != U(NO_SCORE)).sum())
        S = [int((w * q[:, a]).sum()) for a in range(5)]
        resampled = decide(int(p.mode), W, sum_w2, K, int(p.below_num), int(p.below_den))
        anc = None
        if resampled:
            anc = ancestors(w, resample_draw(self.seed, self.epoch))
            self.x, self.acc, self.since = self.x[anc], np.zeros(K, U), 0
        self.epoch += 1
        stats = types.SimpleNamespace(W=W, sum_w2=sum_w2, s_min=s_min, S=S, n_eligible=n_eligible, n_clamped=int(clamped.sum()), resampled=int(resampled), epoch=self.epoch,
                                      since_resample=self.since, origin=[float(F(v)) for v in self.field["origin"]],
                                      resolution=float(F(self.field["resolution"])))
        return stats, (anc.astype(np.uint32) if anc is not None and want_ancestors else None)

    def occ_mcl_filter_get(self, want=("poses", "acc", "n_in")):
        self._need()
        out = dict(poses=self.x.copy(), acc=self.acc.copy(), n_in=self.n_in.copy())
        return {k: out[k] for k in want}

    def occ_mcl_filter_info(self):
        if self.x is None:
            return types.SimpleNamespace(set=0, K=0, seed=0, epoch=0, since_resample=0)
        return types.SimpleNamespace(set=1, K=len(self.x), seed=self.seed, epoch=self.epoch, since_resample=self.since)

    def occ_mcl_filter_clear(self):
        self.x = None
