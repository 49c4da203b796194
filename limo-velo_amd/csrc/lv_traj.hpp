// lv_traj.hpp — the device trajectory (lv_traj_*, include/limovelo_hip.h "Trajectory"; kernels and host side in lv_traj.hip).
//
// The first part is the rule as plain __host__ __device__ code in f64: the bracket search, the sample rule, the per-interval
// records, one smoothing step of a knot, a correction applied to a knot, the registration of a point, the knot range a workgroup
// stages, and the argument rules.  The kernels of lv_traj.hip run exactly these functions; tests/emu/traj_emu.cpp compiles them
// with g++ through tests/emu/hip/hip_runtime.h and tests/test_traj_host.py holds them to tests/traj_ref.py at 1e-9 (libm differs
// between host and device, so not by bits).  The quaternion algebra is lv_graph.hpp's (gr_*).  Every sum is written out in one
// order, and the library is built with -ffp-contract=off: a run on the device repeats its own bits.
//
// Times are f64 seconds everywhere; only DIFFERENCES of times enter the arithmetic, so a recording stamped with the Unix epoch
// gives the bits of the same recording stamped from zero (as long as the stamps themselves are exact in f64).
#pragma once

#include "lv_graph.hpp"

namespace lv {

static_assert(sizeof(lv_traj_knot) == 64, "a knot is 64 bytes");
static_assert(sizeof(lv_traj_info) == 64, "the info record is 64 bytes");
static_assert(sizeof(lv_traj_smooth_params) == 24, "the smoothing parameters are 24 bytes");
static_assert(sizeof(lv_traj_register_params) == 72, "the register parameters are 72 bytes");

constexpr size_t TRAJ_MAX_KNOTS = LV_TRAJ_MAX_KNOTS;
constexpr size_t TRAJ_MAX_ITEMS = (size_t)1 << 28;   // times of a sample call, points of a register call
constexpr double TRAJ_QUAT_TOL = 1e-6;
constexpr uint32_t TRAJ_WG = 256;                     // points of a workgroup of the register kernel
// Knots a workgroup stages in LDS: times 8 B + knot 64 B + interval record 48 B = 120 B a knot, 30 KB a workgroup, five
// workgroups a CU by LDS (160 KB).  At a tenth of the point rate a workgroup's 256 consecutive points span 27 knots.
constexpr uint32_t TRAJ_TILE = 256;
constexpr int TRAJ_MAX_HALF_WINDOW = 64, TRAJ_MAX_ITERATIONS = 100;

// What is computed once per knot i for the interval [i, i + 1): p_b - p_a and Log(q_a^-1 q_b).  Zeros for the last knot.
struct TrajDerived {
    double dp[3];
    double w[3];
};

// ---- the bracket search: the first index in [0, cnt) whose time is > t (cnt when none is); times ascending.  t finite.
LV_GR_HD uint32_t traj_bracket(const double* times, uint32_t cnt, double t) {
    uint32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (times[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

LV_GR_HD bool traj_finite(double v) { return v - v == 0.0; }

LV_GR_HD void traj_derive(const lv_traj_knot& a, const lv_traj_knot& b, TrajDerived* d) {
    double qd[4];
    for (int k = 0; k < 3; ++k) d->dp[k] = b.t[k] - a.t[k];
    gr_qmul_conj(a.q, b.q, qd);
    gr_qlog(qd, d->w);
}

LV_GR_HD void traj_normalise(const double* q, double* o) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) o[k] = q[k] / n;
}

LV_GR_HD void traj_nan_pose(lv_graph_pose* o) {
    for (int k = 0; k < 3; ++k) o->t[k] = NAN;
    for (int k = 0; k < 4; ++k) o->q[k] = NAN;
}
LV_GR_HD void traj_knot_pose(const lv_traj_knot& a, lv_graph_pose* o) {
    for (int k = 0; k < 3; ++k) o->t[k] = a.t[k];
    for (int k = 0; k < 4; ++k) o->q[k] = a.q[k];
}

// ---- the sample rule.  The arrays hold the knots base .. base + cnt - 1 of a trajectory of n knots (the whole of it: base = 0,
// cnt = n; a workgroup's tile: traj_tile_range); t's bracket must lie inside them.  Returns the status.
LV_GR_HD int traj_pose_at(const double* times, const lv_traj_knot* knots, const TrajDerived* der, uint32_t base, uint32_t cnt, uint32_t n,
                          double t, int extrapolate, lv_graph_pose* o) {
    if (!traj_finite(t)) {
        traj_nan_pose(o);
        return LV_TRAJ_NONFINITE;
    }
    const uint32_t ub = traj_bracket(times, cnt, t);
    if (base + ub == 0) {   // before the first knot
        if (extrapolate == LV_TRAJ_CLAMP) traj_knot_pose(knots[0], o);
        else traj_nan_pose(o);
        return LV_TRAJ_BEFORE;
    }
    const uint32_t r = ub - 1, i = base + r;   // the last knot with time <= t
    const lv_traj_knot& a = knots[r];
    if (t == a.time) {   // a knot's own time: its pose, not a bit changed (the last knot too)
        traj_knot_pose(a, o);
        return LV_TRAJ_INSIDE;
    }
    if (i + 1 == n) {    // behind the last knot
        if (extrapolate == LV_TRAJ_CLAMP) traj_knot_pose(a, o);
        else traj_nan_pose(o);
        return LV_TRAJ_AFTER;
    }
    const TrajDerived& d = der[r];
    const double u = (t - a.time) / (times[r + 1] - a.time);
    const double v[3] = {u * d.w[0], u * d.w[1], u * d.w[2]};
    double e[4], q[4];
    for (int k = 0; k < 3; ++k) o->t[k] = a.t[k] + u * d.dp[k];
    gr_qexp(v, e);
    gr_qmul(a.q, e, q);
    traj_normalise(q, o->q);
    return LV_TRAJ_INSIDE;
}

// ---- the knot range [k_lo, k_end) that brackets every finite time of a chunk, from ub_min / ub_max = traj_bracket of the chunk's
// least and greatest finite time: the last knot at or before the least time up to the knot that closes the greatest time's
// interval.  A chunk with no finite time (t_min > t_max: +inf, -inf) needs no knot at all.
LV_GR_HD void traj_tile_range_from(uint32_t ub_min, uint32_t ub_max, uint32_t n, bool any_finite, uint32_t* k_lo, uint32_t* k_end) {
    if (!any_finite) {
        *k_lo = *k_end = 0;
        return;
    }
    *k_lo = ub_min > 0 ? ub_min - 1 : 0;
    *k_end = ub_max + 1 < n ? ub_max + 1 : n;
}
LV_GR_HD void traj_tile_range(const double* times, uint32_t n, double t_min, double t_max, uint32_t* k_lo, uint32_t* k_end) {
    const bool any = t_min <= t_max;
    traj_tile_range_from(any ? traj_bracket(times, n, t_min) : 0, any ? traj_bracket(times, n, t_max) : 0, n, any, k_lo, k_end);
}

// ---- one Jacobi step of the kernel smoother for knot i (reads the old knots only)
LV_GR_HD void traj_smooth_knot(const lv_traj_knot* knots, uint32_t n, uint32_t i, double sigma, uint32_t half_window, lv_traj_knot* o) {
    const lv_traj_knot& a = knots[i];
    const uint32_t lo = i >= half_window ? i - half_window : 0, hi = i + half_window < n - 1 ? i + half_window : n - 1;
    double W = 0.0, sp[3] = {0.0, 0.0, 0.0}, sw[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = lo; j <= hi; ++j) {
        const lv_traj_knot& b = knots[j];
        const double d = (b.time - a.time) / sigma;
        const double w = exp(-0.5 * (d * d));
        double qd[4], l[3];
        gr_qmul_conj(a.q, b.q, qd);
        gr_qlog(qd, l);
        W = W + w;
        for (int k = 0; k < 3; ++k) {
            sp[k] = sp[k] + w * (b.t[k] - a.t[k]);
            sw[k] = sw[k] + w * l[k];
        }
    }
    const double v[3] = {sw[0] / W, sw[1] / W, sw[2] / W};
    double e[4], q[4];
    o->time = a.time;
    for (int k = 0; k < 3; ++k) o->t[k] = a.t[k] + sp[k] / W;
    gr_qexp(v, e);
    gr_qmul(a.q, e, q);
    traj_normalise(q, o->q);
}

// ---- a correction D applied to a knot: t' = D_R t + D_t, q' = D_q * q renormalised; the identity leaves every bit
LV_GR_HD bool traj_is_identity(const lv_graph_pose& D) {
    return D.t[0] == 0.0 && D.t[1] == 0.0 && D.t[2] == 0.0 && D.q[0] == 0.0 && D.q[1] == 0.0 && D.q[2] == 0.0 && D.q[3] == 1.0;
}
LV_GR_HD void traj_correct_knot(const lv_graph_pose& D, const lv_traj_knot& a, lv_traj_knot* o) {
    if (traj_is_identity(D)) {
        *o = a;
        return;
    }
    double R[9], t[3], q[4];
    gr_rot(D.q, R);
    gr_mv(R, a.t, t);
    gr_qmul(D.q, a.q, q);
    o->time = a.time;
    for (int k = 0; k < 3; ++k) o->t[k] = t[k] + D.t[k];
    traj_normalise(q, o->q);
}

// ---- registration.  A rigid map is 12 doubles, R row-major then t; every row is ((a x + b y) + c z) + d.
LV_GR_HD void traj_rigid(const double* t, const double* q, double* M) {
    gr_rot(q, M);
    for (int k = 0; k < 3; ++k) M[9 + k] = t[k];
}
LV_GR_HD void traj_apply(const double* M, const double* p, double* o) {
    for (int k = 0; k < 3; ++k) o[k] = ((M[k * 3] * p[0] + M[k * 3 + 1] * p[1]) + M[k * 3 + 2] * p[2]) + M[9 + k];
}
// F = (T E)^-1 of the pose T at frame_time and the extrinsic E: M = R_T R_E, m = R_T t_E + t_T; F = (M^T, -(M^T m))
LV_GR_HD void traj_frame(const lv_graph_pose& T, const double* E, double* F) {
    double Tm[12], M[9], m[3], mt[3];
    traj_rigid(T.t, T.q, Tm);
    gr_mm(Tm, E, M);
    traj_apply(Tm, E + 9, m);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[i * 3 + j] = M[j * 3 + i];
    gr_mv(F, m, mt);
    for (int k = 0; k < 3; ++k) F[9 + k] = -mt[k];
}
// b = E p, w = T(t) b, and with F: w = F w; rounded once.  status: that of the pose; a non-finite coordinate: NaN, LV_TRAJ_NONFINITE
LV_GR_HD int traj_register_point(const double* E, const lv_graph_pose& T, int status, const double* F, const float* p, float* o) {
    const double x[3] = {(double)p[0], (double)p[1], (double)p[2]};
    if (!(traj_finite(x[0]) && traj_finite(x[1]) && traj_finite(x[2])) || status == LV_TRAJ_NONFINITE) {
        o[0] = o[1] = o[2] = NAN;
        return LV_TRAJ_NONFINITE;
    }
    double Tm[12], b[3], w[3], f[3];
    traj_apply(E, x, b);
    traj_rigid(T.t, T.q, Tm);   // (a refused pose is NaN: so is the point)
    traj_apply(Tm, b, w);
    if (F) {
        traj_apply(F, w, f);
        for (int k = 0; k < 3; ++k) w[k] = f[k];
    }
    for (int k = 0; k < 3; ++k) o[k] = (float)w[k];
    return status;
}

// ---- the argument rules
inline void default_traj_smooth_params(lv_traj_smooth_params* p) {
    if (!p) return;
    p->sigma = 0.1;
    p->half_window = 8;
    p->iterations = 1;
    p->pin_ends = 1;
}
inline void default_traj_register_params(lv_traj_register_params* p) {
    if (!p) return;
    *p = lv_traj_register_params{};
    p->extrapolate = LV_TRAJ_CLAMP;
    p->frame = LV_TRAJ_WORLD;
    p->ext_q[3] = 1.0;
}

// lv_traj_set's judgement of its records, and lv_traj_correct's (what: "trajectory" / "correction")
inline int traj_check(const lv_traj_knot* knots, size_t n, const char* what) {
    if (n == 0 || n > TRAJ_MAX_KNOTS) { set_error("%s: n = %zu outside 1..2^20", what, n); return LV_EINVAL; }
    if (!knots) { set_error("%s: null knots", what); return LV_EINVAL; }
    for (size_t k = 0; k < n; ++k) {
        const lv_traj_knot& a = knots[k];
        if (!traj_finite(a.time)) { set_error("%s: knot %zu: time: a non-finite number", what, k); return LV_EINVAL; }
        if (!graph_detail::finite_all(a.t, 3)) { set_error("%s: knot %zu: t: a non-finite number", what, k); return LV_EINVAL; }
        if (!graph_detail::finite_all(a.q, 4)) { set_error("%s: knot %zu: q: a non-finite number", what, k); return LV_EINVAL; }
        if (!graph_detail::unit_quat(a.q)) { set_error("%s: knot %zu: q: norm off 1 by more than 1e-6", what, k); return LV_EINVAL; }
        if (k && !(knots[k - 1].time < a.time)) { set_error("%s: knot %zu: time: not above knot %zu's", what, k, k - 1); return LV_EINVAL; }
    }
    return LV_OK;
}
inline int traj_smooth_params_ok(const lv_traj_smooth_params* p) {
    if (!p) { set_error("trajectory smooth: null params"); return LV_EINVAL; }
    if (!(p->sigma > 0.0 && traj_finite(p->sigma))) { set_error("trajectory smooth: sigma must be finite and > 0"); return LV_EINVAL; }
    if (p->half_window < 1 || p->half_window > TRAJ_MAX_HALF_WINDOW) { set_error("trajectory smooth: half_window %d outside 1..64", p->half_window); return LV_EINVAL; }
    if (p->iterations < 0 || p->iterations > TRAJ_MAX_ITERATIONS) { set_error("trajectory smooth: iterations %d outside 0..100", p->iterations); return LV_EINVAL; }
    return LV_OK;
}
inline int traj_extrapolate_ok(int extrapolate) {
    if (extrapolate != LV_TRAJ_CLAMP && extrapolate != LV_TRAJ_REFUSE) { set_error("trajectory: extrapolate %d is neither LV_TRAJ_CLAMP nor LV_TRAJ_REFUSE", extrapolate); return LV_EINVAL; }
    return LV_OK;
}
inline int traj_register_params_ok(const lv_traj_register_params* p) {
    if (int rc = traj_extrapolate_ok(p->extrapolate)) return rc;
    if (p->frame != LV_TRAJ_WORLD && p->frame != LV_TRAJ_FRAME_AT) { set_error("trajectory register: frame %d is neither LV_TRAJ_WORLD nor LV_TRAJ_FRAME_AT", p->frame); return LV_EINVAL; }
    if (!graph_detail::finite_all(p->ext_t, 3)) { set_error("trajectory register: ext_t: a non-finite number"); return LV_EINVAL; }
    if (!graph_detail::finite_all(p->ext_q, 4)) { set_error("trajectory register: ext_q: a non-finite number"); return LV_EINVAL; }
    if (!graph_detail::unit_quat(p->ext_q)) { set_error("trajectory register: ext_q: norm off 1 by more than 1e-6"); return LV_EINVAL; }
    if (p->frame == LV_TRAJ_FRAME_AT && !traj_finite(p->frame_time)) { set_error("trajectory register: frame_time: a non-finite number"); return LV_EINVAL; }
    return LV_OK;
}
// the records of lv_traj_register: x, y, z f32 at 0, an f64 time at time_offset
inline int traj_register_layout_ok(const void* pts, size_t stride, size_t time_offset, size_t n) {
    if (n > TRAJ_MAX_ITEMS) { set_error("trajectory register: n = %zu above 2^28", n); return LV_EINVAL; }
    if (n && !pts) { set_error("trajectory register: null points"); return LV_EINVAL; }
    if (time_offset < 12) { set_error("trajectory register: time_offset %zu below 12 (x, y, z come first)", time_offset); return LV_EINVAL; }
    if (stride < time_offset + 8) { set_error("trajectory register: stride %zu below time_offset + 8 = %zu", stride, time_offset + 8); return LV_EINVAL; }
    return LV_OK;
}
// frame_time must lie on the trajectory
inline int traj_frame_time_ok(double frame_time, double t_first, double t_last) {
    if (!(frame_time >= t_first && frame_time <= t_last)) { set_error("trajectory register: frame_time %.9f outside the trajectory [%.9f, %.9f]", frame_time, t_first, t_last); return LV_EINVAL; }
    return LV_OK;
}

// ---- the store (host side in lv_traj.hip)
constexpr size_t TRAJ_CHUNK = (size_t)1 << 22;   // points of one upload / launch / download of register and sample (a multiple of TRAJ_WG)

// where a launch of the register kernel reads its points: strides in elements of the pointer's type
struct TrajPoints {
    const float* xyz;
    const double* times;
    uint32_t xyz_stride, time_stride;
};

struct TrajStore {
    bool set = false;
    bool tile = true;   // lv_set_option "traj_tile"
    size_t n = 0;
    lv_traj_info info{};
    DevBuf<lv_traj_knot> d_knots, d_next, d_corr;   // the knots; the smoother's second buffer; lv_traj_correct's records
    DevBuf<TrajDerived> d_der, d_cder;
    DevBuf<double> d_times, d_ctimes;                // packed, for the bracket search
    DevBuf<uint8_t> d_fixed;
    // lv_traj_sample / lv_traj_register
    PinBuf<float> h_xyz;
    PinBuf<double> h_t;
    DevBuf<float> d_xyz, d_out;
    DevBuf<double> d_t, d_F;
    DevBuf<uint8_t> d_status;
    DevBuf<lv_graph_pose> d_poses;
    Counters4 counters;

    int assign(hipStream_t stream, const lv_traj_knot* knots, size_t n);
    int fetch(hipStream_t stream, lv_traj_knot* knots);
    int sample(hipStream_t stream, const double* times, size_t count, int extrapolate, lv_graph_pose* out, uint8_t* status);
    int smooth(hipStream_t stream, const lv_traj_smooth_params& prm, const uint8_t* fixed);
    int correct(hipStream_t stream, const lv_traj_knot* corr, size_t m);
    int register_host(hipStream_t stream, const lv_traj_register_params& prm, const void* pts, size_t stride, size_t time_offset, size_t count,
                      float* out, uint8_t* status, uint64_t stats[4]);
    // points already on the device (the LiDAR buffer)
    int register_device(hipStream_t stream, const lv_traj_register_params& prm, const TrajPoints& in, size_t count, float* out, uint8_t* status,
                        uint64_t stats[4]);
    void clear() { set = false; n = 0; info = lv_traj_info{}; }
    void release();

   private:
    int derive(hipStream_t stream);
    int begin_register(hipStream_t stream, const lv_traj_register_params& prm, double* E);
    int launch_register(hipStream_t stream, const lv_traj_register_params& prm, const double* E, const TrajPoints& in, size_t count,
                        bool want_out, bool want_status);
    int end_register(hipStream_t stream, uint64_t stats[4]);
};

}  // namespace lv
