// lv_surf_align.hpp — registration against the TSDF surface (lv_surf_sample, lv_surf_align, include/limovelo_hip.h "Surface
// registration"; kernels and host side in lv_surf_align.hip, the scratch a member of TsdfStore).
//
// The rule as plain __host__ __device__ code in f64: the trilinear sample of phi = S / W with the exact gradient of the
// interpolant, what one source point adds to H, g and E at a pose, the cost with its gate charge, the method's rule for the
// Levenberg-Marquardt loop of lv_align.hpp (SurfAlignRule), and the argument rules.  The kernels of lv_surf_align.hip run exactly these functions;
// tests/emu/surf_align_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_surf_align_host.py holds
// them to tests/surf_align_ref.py (the sample by equality: only + - * / and floor occur).  Every sum is written out in one order
// and the library is built with -ffp-contract=off.
//
// The order of the 21 entries, the damped solve, the turn of one hypothesis, `best`, the shared argument rules, the kernel bodies
// and the host driver of lv_surf_align are lv_align.hpp's, as they are NDT registration's; the quaternion algebra is lv_graph.hpp's.
#pragma once

#include "lv_align.hpp"
#include "lv_tsdf.hpp"

namespace lv {

static_assert(sizeof(lv_surf_align_params) == 64, "lv_surf_align_params is 64 bytes");
static_assert(sizeof(lv_surf_align_result) == 264, "lv_surf_align_result is 264 bytes");
static_assert(sizeof(lv_surf_align_result) == sizeof(lv_ndt_result), "laid out as lv_ndt_result");

constexpr double SURF_U_LIMIT = 16777216.0;                  // 2^24: a point this many voxels from the origin is OUTSIDE
constexpr uint64_t SURF_SAMPLE_MAX_N = 0x7FFFFFFFull;        // lv_surf_sample: n below this

// The volume as the sample reads it
struct SurfView {
    double o[3];          // (double)origin_a at the volume's present shift
    double r;             // (double)resolution
    int nx, ny, nz;
    int32_t min_weight;
    const int32_t* S;
    const int32_t* W;
};

inline SurfView surf_view_of(const TsdfGrid& g, int32_t min_weight, const int32_t* S, const int32_t* W) {
    SurfView v{};
    for (int a = 0; a < 3; ++a) v.o[a] = (double)g.occ.origin[a];
    v.r = (double)g.occ.resolution;
    v.nx = g.occ.nx;
    v.ny = g.occ.ny;
    v.nz = g.occ.nz;
    v.min_weight = min_weight;
    v.S = S;
    v.W = W;
    return v;
}

// ---- the sample at world point x: the state; for a KNOWN point d (metres) and n (the gradient of the interpolant,
// dimensionless, not normalised), otherwise zeros
LV_OCC_HD int surf_sample(const SurfView& v, const double x[3], double& d, double n[3]) {
    d = 0.0;
    n[0] = n[1] = n[2] = 0.0;
    const int dim[3] = {v.nx, v.ny, v.nz};
    int i[3];
    double f[3];
    for (int a = 0; a < 3; ++a) {
        const double u = (x[a] - v.o[a]) / v.r - 0.5;
        if (!(fabs(u) < SURF_U_LIMIT)) return LV_SURF_SAMPLE_OUTSIDE;   // (a NaN compares false)
        const double fl = floor(u);
        i[a] = (int)fl;
        f[a] = u - fl;
    }
    for (int a = 0; a < 3; ++a)
        if (i[a] < 0 || i[a] + 1 > dim[a] - 1) return LV_SURF_SAMPLE_OUTSIDE;
    const size_t at = grid_at(v, i[0], i[1], i[2]);
    const size_t sy = (size_t)v.nx, sz = (size_t)v.nx * (size_t)v.ny;
    // corner (a, b, c) at a + 2 b + 4 c; the eight weights first: they are in flight together
    int32_t w[8];
    bool known = true;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        w[m] = v.W[at + (size_t)(m & 1) + ((m >> 1) & 1) * sy + (size_t)(m >> 2) * sz];
        known = known && w[m] >= v.min_weight;
    }
    if (!known) return LV_SURF_SAMPLE_UNKNOWN;
    double phi[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) phi[m] = (double)v.S[at + (size_t)(m & 1) + ((m >> 1) & 1) * sy + (size_t)(m >> 2) * sz] / (double)w[m];
    // along x: c_bc, e_bc at b + 2 c
    double c2[4], e2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        e2[m] = phi[2 * m + 1] - phi[2 * m];
        c2[m] = phi[2 * m] + f[0] * e2[m];
    }
    // along y: c_c, ex_c, ey_c
    double c1[2], ex[2], ey[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        ey[m] = c2[2 * m + 1] - c2[2 * m];
        c1[m] = c2[2 * m] + f[1] * ey[m];
        ex[m] = e2[2 * m] + f[1] * (e2[2 * m + 1] - e2[2 * m]);
    }
    // along z
    const double gz = c1[1] - c1[0];
    const double val = c1[0] + f[2] * gz;
    const double gx = ex[0] + f[2] * (ex[1] - ex[0]);
    const double gy = ey[0] + f[2] * (ey[1] - ey[0]);
    d = (v.r / 256.0) * val;
    n[0] = gx / 256.0;
    n[1] = gy / 256.0;
    n[2] = gz / 256.0;
    return LV_SURF_SAMPLE_KNOWN;
}

// ---- the evaluation
// rho and the weight w of a residual d under the Huber width h (h = 0: quadratic)
LV_OCC_HD double surf_rho(double d, double h, double& w) {
    const double a = fabs(d);
    w = 1.0;
    if (h == 0.0 || a <= h) return 0.5 * d * d;
    w = h / a;
    return h * (a - 0.5 * h);
}

// what a source point that is not IN pays: a point at the gate
LV_OCC_HD double surf_gate_rho(double max_dist, double huber) {
    double w;
    return surf_rho(max_dist, huber, w);
}

LV_OCC_HD double surf_cost(double E, uint32_t n_src, uint32_t n_in, double max_dist, double huber) {
    return E + (double)(n_src - n_in) * surf_gate_rho(max_dist, huber);
}

// What source point p adds to acc (21 of H, 6 of g, E) at the pose (R, t).  true: the point is IN and counts in n_in.
LV_OCC_HD bool surf_point_terms(const SurfView& v, const double* R, const double* t, const float* p, double max_dist, double huber, double* acc) {
    const double pd[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double x[3];
    for (int k = 0; k < 3; ++k) x[k] = ((R[k * 3] * pd[0] + R[k * 3 + 1] * pd[1]) + R[k * 3 + 2] * pd[2]) + t[k];
    double d, n[3];
    if (surf_sample(v, x, d, n) != LV_SURF_SAMPLE_KNOWN) return false;
    if (!(fabs(d) <= max_dist)) return false;
    double w;
    const double rho = surf_rho(d, huber, w);
    // A = -R [p]x; J = [ n^T , n^T A ]
    double P[9], RP[9], J[6], wJ[6];
    gr_hat(pd, P);
    gr_mm(R, P, RP);
    for (int c = 0; c < 3; ++c) {
        J[c] = n[c];
        J[3 + c] = (n[0] * -RP[c] + n[1] * -RP[3 + c]) + n[2] * -RP[6 + c];
    }
    for (int a = 0; a < 6; ++a) wJ[a] = w * J[a];
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) acc[align_tri(a, b)] = acc[align_tri(a, b)] + wJ[a] * J[b];
    const double wd = w * d;
    for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + wd * J[a];
    acc[27] = acc[27] + rho;
    return true;
}

LV_OCC_HD bool surf_accept(double c_new, double c_old) { return c_new <= c_old + 64.0 * 2.220446049250313e-16 * fabs(c_old); }

// The method as the loop of lv_align.hpp takes it: the cost (E plus the gate charge of the n_src - n_in points that are not IN) is
// minimised, a guess and a trial both need min_points
struct SurfAlignRule {
    using Result = lv_surf_align_result;
    AlignLoop loop;
    SurfView v;
    double max_dist, huber;
    uint32_t n_src;
    LV_OCC_HD bool point_terms(const double* R, const double* t, const float* p, double* acc) const { return surf_point_terms(v, R, t, p, max_dist, huber, acc); }
    LV_OCC_HD double objective(const double* tot, uint32_t n_in) const { return surf_cost(tot[27], n_src, n_in, max_dist, huber); }
    LV_OCC_HD static double& objective_of(Result& r) { return r.cost; }
    LV_OCC_HD static bool accept(double c_new, double c_old) { return surf_accept(c_new, c_old); }
    static bool better(const Result& a, const Result& b) { return a.cost < b.cost; }
};
inline SurfAlignRule surf_align_rule_of(const lv_surf_align_params& p, const SurfView& v, uint32_t n_src) {
    return SurfAlignRule{AlignLoop{p.max_iterations, p.min_points, p.min_points, 0, p.step_tol, p.lambda_init, p.lambda_min, p.lambda_max}, v, p.max_dist,
                    p.huber, n_src};
}

// The shared loop under the method's own names, for a caller written against surface registration alone (lv_api.hip's argument
// check; a host program that steps the loop itself, as tests/emu/surf_align_emu.cpp did before align_one).  One line each into
// lv_align.hpp.
constexpr int SURF_ACC = ALIGN_ACC;
constexpr int32_t SURF_RUNNING = ALIGN_RUNNING;
using NdtHyp = AlignHyp;   // (the record's first name)
inline bool surf_turn(const lv_surf_align_params& prm, uint32_t n_src, bool first, const double* tot, uint32_t n_in, lv_surf_align_result& res,
                      AlignHyp& h) {
    return align_turn(surf_align_rule_of(prm, SurfView{}, n_src), first, tot, n_in, res, h);
}
inline void surf_align_best(const lv_surf_align_result* res, size_t K, int32_t best[2]) { align_best<SurfAlignRule>(res, K, best); }
inline int surf_check_align_args(const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses, size_t K,
                                 const lv_surf_align_result* results, const int32_t* best) {
    return align_check_args("lv_surf_align", src, stride, n_src, guesses, K, results, best);
}

// ---- the argument rules
inline void default_surf_align_params(lv_surf_align_params* p) {
    if (!p) return;
    *p = lv_surf_align_params{};
    p->min_weight = 1;
    p->max_iterations = 50;
    p->min_points = 6;
    p->max_dist = 0.4;
    p->huber = 0.1;
    p->step_tol = 1e-6;
    p->lambda_init = 1e-4;
    p->lambda_min = 1e-10;
    p->lambda_max = 1e8;
}
// NULL when they hold, otherwise what is wrong
inline const char* surf_check_align_params(const lv_surf_align_params* p) {
    const auto fin = [](double v) { return v - v == 0.0; };
    if (p->min_weight < 1) return "min_weight: at least 1";
    if (const char* why = align_check_iterations(p->max_iterations)) return why;
    if (p->min_points < 1) return "min_points: at least 1";
    if (!(p->max_dist > 0.0 && fin(p->max_dist))) return "max_dist: finite and > 0";
    if (!(p->huber >= 0.0 && fin(p->huber))) return "huber: finite and >= 0";
    return align_check_loop(p->step_tol, p->lambda_init, p->lambda_min, p->lambda_max);
}
// lv_surf_sample's arguments; the message is set
inline int surf_check_sample_args(int min_weight, const void* pts, size_t stride, size_t n, const double* out, const uint8_t* status) {
    if (min_weight < 1) { set_error("lv_surf_sample: min_weight = %d: at least 1", min_weight); return LV_EINVAL; }
    if (!out && !status) { set_error("lv_surf_sample: out and status are both null"); return LV_EINVAL; }
    if (n >= SURF_SAMPLE_MAX_N) { set_error("lv_surf_sample: too many points"); return LV_EINVAL; }
    if (n && (!pts || stride < 12)) { set_error("lv_surf_sample: bad point array (stride %zu)", stride); return LV_EINVAL; }
    return LV_OK;
}

}  // namespace lv
