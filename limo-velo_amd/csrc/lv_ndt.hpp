// lv_ndt.hpp — NDT scan registration (lv_ndt_*, include/limovelo_hip.h "NDT registration"; kernels and host side in lv_ndt.hip).
//
// The first part is the rule as plain __host__ __device__ code in f64: the voxel and local coordinate of a point (lv_grid.hpp's
// occ_quant, as it is), the Gaussian of a voxel from its integer moments, what one source point adds to S, g and H at a pose, the
// method's rule for the Levenberg-Marquardt loop of lv_align.hpp (NdtRule), and the argument rules.  The kernels of lv_ndt.hip run
// exactly these functions; tests/emu/ndt_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and
// tests/test_ndt_host.py holds them to tests/ndt_ref.py (moments by equality, f64 algebra at 1e-12: libm differs between host and
// device).  Every sum is written out in one order and the library is built with -ffp-contract=off.
//
// The order of the 21 entries, the damped solve, the turn of one hypothesis, `best`, the shared argument rules, the kernel bodies
// and the host driver of lv_ndt_align are lv_align.hpp's; the quaternion algebra is lv_graph.hpp's.
#pragma once

#include "lv_align.hpp"

namespace lv {

static_assert(sizeof(lv_ndt_params) == 40, "lv_ndt_params is 40 bytes");
static_assert(sizeof(lv_ndt_align_params) == 48, "lv_ndt_align_params is 48 bytes");
static_assert(sizeof(lv_ndt_result) == 264, "lv_ndt_result is 264 bytes");
static_assert(sizeof(lv_ndt_target_info) == 80, "lv_ndt_target_info is 80 bytes");

constexpr uint64_t NDT_MAX_POINTS = 0x7FFFFFFFull; // the points of a target: build plus adds
constexpr double NDT_D2_DEFAULT = 0.43312300470355464;

// The grid as the kernels take it
struct NdtGrid {
    float origin[3];
    float resolution;
    int nx, ny, nz;
    int min_points;
    double reg;
};

// the target's Gaussians as the evaluation reads them (a voxel that is not USED holds zeros: icov[0] > 0 tells)
struct NdtView {
    NdtGrid g;
    const double* mean;   // 3 per voxel
    const double* icov;   // 6 per voxel
};

// ---- the target
// The voxel and the local coordinate of world point p; false: the point is ignored
LV_OCC_HD bool ndt_point(const NdtGrid& g, const float p[3], uint32_t& cell, int32_t c[3], int32_t r[3]) {
    int32_t q[3] = {0, 0, 0};
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = occ_quant(p[a], g.origin[a], g.resolution, q[a]) && ok;
    if (!ok) return false;
    for (int a = 0; a < 3; ++a) {
        c[a] = q[a] >> 8;
        r[a] = q[a] & 255;
    }
    if (!grid_inside(g, c[0], c[1], c[2])) return false;
    cell = (uint32_t)grid_at(g, c[0], c[1], c[2]);
    return true;
}

// The Gaussian of voxel c from its moments: mean[3], cov[6] (Sigma) and icov[6] (Omega), upper triangles 00 01 02 11 12 22.
// false (and zeros): the voxel is not USED.
LV_OCC_HD bool ndt_gaussian(const NdtGrid& g, const int32_t c[3], uint32_t n, const long long* S1, const long long* S2, double* mean,
                            double* cov, double* icov) {
    for (int k = 0; k < 3; ++k) mean[k] = 0.0;
    for (int k = 0; k < 6; ++k) cov[k] = icov[k] = 0.0;
    if (n < (uint32_t)g.min_points) return false;
    const double u = (double)g.resolution / 256.0, u2 = u * u, nn = (double)n;
    for (int a = 0; a < 3; ++a) {
        const double m = ((double)S1[a] + 0.5 * nn) / nn;
        mean[a] = ((double)g.origin[a] + (double)g.resolution * (double)c[a]) + u * m;
    }
    double C[6];
    int k = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b, ++k) C[k] = (u2 * ((double)S2[k] - ((double)S1[a] * (double)S1[b]) / nn)) / (nn - 1.0);
    const double add = (g.reg * ((C[0] + C[3]) + C[5])) / 3.0 + u2 / 12.0;
    C[0] = C[0] + add;
    C[3] = C[3] + add;
    C[5] = C[5] + add;
    // Sigma = L L^T, column by column
    const double l00 = sqrt(C[0]), l10 = C[1] / l00, l20 = C[2] / l00;
    const double d1 = C[3] - l10 * l10;
    const double l11 = sqrt(d1), l21 = (C[4] - l20 * l10) / l11;
    const double d2 = (C[5] - l20 * l20) - l21 * l21;
    const double l22 = sqrt(d2);
    if (!(C[0] > 0.0 && d1 > 0.0 && d2 > 0.0 && l22 < INFINITY)) return false;   // (cannot happen for reg >= 0: Sigma >= u^2 / 12 I)
    for (int q = 0; q < 6; ++q) cov[q] = C[q];
    // Li = L^-1, Omega = Li^T Li
    const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
    const double i10 = -(l10 * i00) / l11, i21 = -(l21 * i11) / l22, i20 = -(l20 * i00 + l21 * i10) / l22;
    icov[0] = (i00 * i00 + i10 * i10) + i20 * i20;
    icov[1] = i10 * i11 + i20 * i21;
    icov[2] = i20 * i22;
    icov[3] = i11 * i11 + i21 * i21;
    icov[4] = i21 * i22;
    icov[5] = i22 * i22;
    return true;
}

// ---- the evaluation
// What source point p adds to acc (21 of H, 6 of g, S) at the pose (R, t); hd = -0.5 d2.  true: the point counts in n_in.
LV_OCC_HD bool ndt_point_terms(const NdtView& v, const double* R, const double* t, const float* p, int search, double hd, double* acc) {
    const double pd[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double x[3];
    float xf[3];
    for (int k = 0; k < 3; ++k) {
        x[k] = ((R[k * 3] * pd[0] + R[k * 3 + 1] * pd[1]) + R[k * 3 + 2] * pd[2]) + t[k];
        xf[k] = (float)x[k];
    }
    int32_t q[3] = {0, 0, 0};
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = occ_quant(xf[a], v.g.origin[a], v.g.resolution, q[a]) && ok;
    if (!ok) return false;
    const int c0[3] = {q[0] >> 8, q[1] >> 8, q[2] >> 8};
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, sw = 0.0;
    bool any = false;
    for (int s = 0; s < search; ++s) {
        // 0, +x, -x, +y, -y, +z, -z
        const int ax = (s - 1) >> 1, sg = (s & 1) ? 1 : -1;
        const int ci = c0[0] + (s && ax == 0 ? sg : 0), cj = c0[1] + (s && ax == 1 ? sg : 0), ck = c0[2] + (s && ax == 2 ? sg : 0);
        if (!grid_inside(v.g, ci, cj, ck)) continue;
        const size_t cell = grid_at(v.g, ci, cj, ck);
        const double* O = v.icov + cell * 6;
        if (!(O[0] > 0.0)) continue;
        const double* mu = v.mean + cell * 3;
        const double e[3] = {x[0] - mu[0], x[1] - mu[1], x[2] - mu[2]};
        const double Oe[3] = {(O[0] * e[0] + O[1] * e[1]) + O[2] * e[2], (O[1] * e[0] + O[3] * e[1]) + O[4] * e[2],
                              (O[2] * e[0] + O[4] * e[1]) + O[5] * e[2]};
        const double ss = (e[0] * Oe[0] + e[1] * Oe[1]) + e[2] * Oe[2];
        const double w = exp(hd * ss);
        for (int k = 0; k < 6; ++k) M[k] = M[k] + w * O[k];
        for (int k = 0; k < 3; ++k) b[k] = b[k] + w * Oe[k];
        sw = sw + w;
        any = true;
    }
    if (!any) return false;
    // A = -R [p]x; MA = M A; H_thth = A^T MA
    double P[9], RP[9], A[9], Mf[9], MA[9];
    gr_hat(pd, P);
    gr_mm(R, P, RP);
    for (int k = 0; k < 9; ++k) A[k] = -RP[k];
    Mf[0] = M[0]; Mf[1] = M[1]; Mf[2] = M[2];
    Mf[3] = M[1]; Mf[4] = M[3]; Mf[5] = M[4];
    Mf[6] = M[2]; Mf[7] = M[4]; Mf[8] = M[5];
    gr_mm(Mf, A, MA);
    for (int a = 0; a < 3; ++a)
        for (int c = a; c < 3; ++c) acc[align_tri(a, c)] = acc[align_tri(a, c)] + Mf[a * 3 + c];
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) acc[align_tri(a, 3 + c)] = acc[align_tri(a, 3 + c)] + MA[a * 3 + c];
    for (int a = 0; a < 3; ++a)
        for (int c = a; c < 3; ++c) {
            const double h = (A[a] * MA[c] + A[3 + a] * MA[3 + c]) + A[6 + a] * MA[6 + c];
            acc[align_tri(3 + a, 3 + c)] = acc[align_tri(3 + a, 3 + c)] + h;
        }
    for (int a = 0; a < 3; ++a) {
        acc[21 + a] = acc[21 + a] + b[a];
        const double gth = (A[a] * b[0] + A[3 + a] * b[1]) + A[6 + a] * b[2];
        acc[24 + a] = acc[24 + a] + gth;
    }
    acc[27] = acc[27] + sw;
    return true;
}

LV_OCC_HD bool ndt_accept(double s_new, double s_old) { return s_new >= s_old - 64.0 * 2.220446049250313e-16 * fabs(s_old); }

// The method as the loop of lv_align.hpp takes it: S is maximised, a guess needs one point, a trial none
struct NdtRule {
    using Result = lv_ndt_result;
    AlignLoop loop;
    NdtView v;
    int search;
    double hd;   // -0.5 d2
    LV_OCC_HD bool point_terms(const double* R, const double* t, const float* p, double* acc) const { return ndt_point_terms(v, R, t, p, search, hd, acc); }
    LV_OCC_HD double objective(const double* tot, uint32_t) const { return tot[27]; }
    LV_OCC_HD static double& objective_of(Result& r) { return r.score; }
    LV_OCC_HD static bool accept(double s_new, double s_old) { return ndt_accept(s_new, s_old); }
    static bool better(const Result& a, const Result& b) { return a.score > b.score; }
};
inline NdtRule ndt_rule_of(const lv_ndt_align_params& p, const NdtView& v) {
    return NdtRule{AlignLoop{p.max_iterations, 1, 0, 0, p.step_tol, p.lambda_init, p.lambda_min, p.lambda_max}, v, p.search, -0.5 * p.d2};
}

// The shared loop under the method's own names, for a caller written against NDT registration alone (lv_api.hip's argument check;
// a host program that steps the loop itself, as tests/emu/ndt_emu.cpp did before align_one).  Each is one line into lv_align.hpp.
constexpr int NDT_ACC = ALIGN_ACC;
constexpr int32_t NDT_RUNNING = ALIGN_RUNNING;
using NdtHyp = AlignHyp;
inline bool ndt_turn(const lv_ndt_align_params& prm, bool first, const double* tot, uint32_t n_in, lv_ndt_result& res, NdtHyp& h) {
    return align_turn(ndt_rule_of(prm, NdtView{}), first, tot, n_in, res, h);
}
inline void ndt_best(const lv_ndt_result* res, size_t K, int32_t best[2]) { align_best<NdtRule>(res, K, best); }
inline int ndt_check_align_args(const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses, size_t K, const lv_ndt_result* results,
                                const int32_t* best) {
    return align_check_args("lv_ndt_align", src, stride, n_src, guesses, K, results, best);
}

// ---- the argument rules
inline void default_ndt_params(lv_ndt_params* p) {
    if (!p) return;
    *p = lv_ndt_params{};
    p->origin[0] = -64.f;
    p->origin[1] = -64.f;
    p->origin[2] = -8.f;
    p->resolution = 1.f;
    p->nx = 128;
    p->ny = 128;
    p->nz = 16;
    p->min_points = 5;
    p->reg = 0.01;
}
inline void default_ndt_align_params(lv_ndt_align_params* p) {
    if (!p) return;
    *p = lv_ndt_align_params{};
    p->search = 7;
    p->max_iterations = 100;
    p->d2 = NDT_D2_DEFAULT;
    p->step_tol = 1e-6;
    p->lambda_init = 1e-4;
    p->lambda_min = 1e-10;
    p->lambda_max = 1e8;
}
// NULL when they hold, otherwise what is wrong
inline const char* ndt_check_params(const lv_ndt_params* p) {
    if (!p) return "null params";
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(p->origin[a]) < __builtin_huge_valf())) return "origin: must be finite";
    if (!(p->resolution > 0.f && p->resolution < __builtin_huge_valf())) return "resolution: finite and > 0";
    if (p->nx < 1 || p->nx > LV_NDT_MAX_DIM || p->ny < 1 || p->ny > LV_NDT_MAX_DIM || p->nz < 1 || p->nz > LV_NDT_MAX_DIM) return "nx, ny, nz: 1..1024 each";
    if ((uint64_t)p->nx * (uint64_t)p->ny * (uint64_t)p->nz > LV_NDT_MAX_VOXELS) return "nx * ny * nz: at most 2^22 voxels";
    if (p->min_points < 2 || p->min_points > (1 << 20)) return "min_points: 2..2^20";
    if (!(p->reg >= 0.0 && p->reg <= 1.0)) return "reg: 0..1";
    return nullptr;
}
inline const char* ndt_check_points(const void* pts, size_t stride, size_t n) {
    if (pts && stride < 12) return "bad point array (stride below 12)";
    if (pts && n > NDT_MAX_POINTS) return "too many points (2^31 - 1 at most)";
    return nullptr;
}
inline const char* ndt_check_align_params(const lv_ndt_align_params* p) {
    const auto fin = [](double v) { return v - v == 0.0; };
    if (p->search != 1 && p->search != 7) return "search: 1 or 7";
    if (const char* why = align_check_iterations(p->max_iterations)) return why;
    if (!(p->d2 > 0.0 && fin(p->d2))) return "d2: finite and > 0";
    return align_check_loop(p->step_tol, p->lambda_init, p->lambda_min, p->lambda_max);
}

inline NdtGrid ndt_grid_of(const lv_ndt_params& p) {
    NdtGrid g{};
    for (int a = 0; a < 3; ++a) g.origin[a] = p.origin[a];
    g.resolution = p.resolution;
    g.nx = p.nx;
    g.ny = p.ny;
    g.nz = p.nz;
    g.min_points = p.min_points;
    g.reg = p.reg;
    return g;
}

// elements and bytes per element of a layer of lv_ndt_fetch; 0: no such layer
inline size_t ndt_layer_width(int layer) {
    switch (layer) {
        case LV_NDT_COUNT: return 1;
        case LV_NDT_S1: case LV_NDT_MEAN: return 3;
        case LV_NDT_S2: case LV_NDT_COV: case LV_NDT_ICOV: return 6;
        default: return 0;
    }
}
inline size_t ndt_layer_elem(int layer) { return layer == LV_NDT_COUNT ? 4 : 8; }

// ---- the store (host side in lv_ndt.hip).  Nothing is allocated before the first build().
struct NdtStore {
    bool built = false;
    lv_ndt_target_info info{};
    NdtGrid grid{};
    size_t n_cells = 0;
    uint64_t n_given = 0;                 // points handed to the target so far (the map's ids when it was the source)
    DevBuf<uint32_t> d_n;
    DevBuf<unsigned long long> d_S1, d_S2;   // (the local coordinates are not negative: the int64 sums as the unsigned atomics take them)
    DevBuf<double> d_mean, d_cov, d_icov;
    Counters4 stats;
    PointStage pts;                       // the caller's points of a build or add
    AlignStage<lv_ndt_result> loop;       // lv_ndt_align's scratch

    int build(hipStream_t stream, const lv_ndt_params* p, const float4* map_orig, uint32_t n_ids, const void* points, size_t stride, size_t n,
              uint64_t out[4]);
    int fetch(hipStream_t stream, int layer, void* out);
    int align(hipStream_t stream, const lv_ndt_align_params& prm, const void* points, size_t stride, size_t n_src, const lv_graph_pose* guesses,
              size_t K, lv_ndt_result* results, int32_t best[2]);
    void release();
};

}  // namespace lv
