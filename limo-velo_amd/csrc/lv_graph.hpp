// lv_graph.hpp — pose-graph optimisation (lv_graph_*, include/limovelo_hip.h "Pose graph"; kernels and host side in lv_graph.hip).
//
// The first part is the rule as plain __host__ __device__ code in f64: residuals, Jacobians, the weighted Gauss-Newton blocks of
// a between-edge and of a prior, the Huber weight, the retraction, the 6 x 6 block inverse, the warp of a point, and the argument
// rules of lv_graph_set / lv_graph_optimise.  The kernels of lv_graph.hip run exactly these functions; tests/emu/graph_emu.cpp
// compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_graph_host.py holds them to tests/graph_ref.py at 1e-9
// (libm differs between host and device, so not by bits).  Every sum below is written out in one order, and the library is built
// with -ffp-contract=off: a run on the device repeats its own bits.
//
// Matrices are row-major.  A 6-vector is (t, th); a 6 x 6 block has rows and columns in that order.
#pragma once

#include <math.h>
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "../../include/limovelo_hip.h"
#include "lv_buffers.hpp"

#if defined(__HIPCC__)
#define LV_GR_HD __host__ __device__ inline
#else
#define LV_GR_HD inline
#endif

namespace lv {

void set_error(const char* fmt, ...);

static_assert(sizeof(lv_graph_pose) == 56, "a pose is 56 bytes");
static_assert(sizeof(lv_graph_edge) == 240, "an edge is 240 bytes");
static_assert(sizeof(lv_graph_prior) == 264, "a prior is 264 bytes");

constexpr size_t GRAPH_MAX_NODES = LV_GRAPH_MAX_NODES, GRAPH_MAX_EDGES = LV_GRAPH_MAX_EDGES, GRAPH_MAX_PRIORS = LV_GRAPH_MAX_PRIORS;
constexpr size_t GRAPH_MAX_WARP = (size_t)1 << 28;
constexpr double GRAPH_QUAT_TOL = 1e-6;
constexpr double GRAPH_SERIES_TH = 1e-4;      // below it Jr^-1 takes its series
constexpr uint32_t GRAPH_WAVE_LIST = 64;      // a longer incidence list is folded by a wavefront
// an entry of an incidence list: (factor id << 2) | kind
constexpr uint32_t GRAPH_SIDE_I = 0, GRAPH_SIDE_J = 1, GRAPH_PRIOR = 2;

// ---- small algebra
LV_GR_HD void gr_rot(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - z * w);
    R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);
    R[7] = 2.0 * (y * z + x * w);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}
// o = a * b (o may not alias)
LV_GR_HD void gr_qmul(const double* a, const double* b, double* o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
// o = conj(a) * b
LV_GR_HD void gr_qmul_conj(const double* a, const double* b, double* o) {
    const double c[4] = {-a[0], -a[1], -a[2], a[3]};
    gr_qmul(c, b, o);
}
// Log of a unit quaternion, taken with w >= 0
LV_GR_HD void gr_qlog(const double* q, double* o) {
    const double sg = q[3] < 0.0 ? -1.0 : 1.0;
    const double x = sg * q[0], y = sg * q[1], z = sg * q[2], w = sg * q[3];
    const double nv = sqrt(x * x + y * y + z * z);
    const double f = nv < 1e-12 ? 2.0 / w : 2.0 * atan2(nv, w) / nv;
    o[0] = f * x;
    o[1] = f * y;
    o[2] = f * z;
}
// the unit quaternion of Exp(v)
LV_GR_HD void gr_qexp(const double* v, double* q) {
    const double th = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double h = 0.5 * th;
    const double f = th < 1e-8 ? 0.5 - th * th / 48.0 : sin(h) / th;
    q[0] = f * v[0];
    q[1] = f * v[1];
    q[2] = f * v[2];
    q[3] = cos(h);
}
LV_GR_HD void gr_hat(const double* v, double* H) {
    H[0] = 0.0;   H[1] = -v[2]; H[2] = v[1];
    H[3] = v[2];  H[4] = 0.0;   H[5] = -v[0];
    H[6] = -v[1]; H[7] = v[0];  H[8] = 0.0;
}
// C = A B, C = A^T B, C = A B^T of 3 x 3 (C may not alias); sums left to right
LV_GR_HD void gr_mm(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
LV_GR_HD void gr_mtm(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
LV_GR_HD void gr_mv(const double* A, const double* v, double* o) {
    for (int i = 0; i < 3; ++i) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
LV_GR_HD void gr_mtv(const double* A, const double* v, double* o) {
    for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
// Jr^-1(p) = I + [p]x / 2 + c [p]x^2
LV_GR_HD void gr_jrinv(const double* p, double* J) {
    const double th2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    const double th = sqrt(th2);
    const double c = th < GRAPH_SERIES_TH ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
    double H[9], HH[9];
    gr_hat(p, H);
    gr_mm(H, H, HH);
    for (int k = 0; k < 9; ++k) J[k] = ((k & 3) == 0 ? 1.0 : 0.0) + 0.5 * H[k] + c * HH[k];
}
// the full symmetric 6 x 6 from the 21 entries of its upper triangle
LV_GR_HD void gr_info(const double* u, double* W) {
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) {
            W[a * 6 + b] = u[k];
            W[b * 6 + a] = u[k];
        }
}
// s = r^T W r, rows in order, each row left to right
LV_GR_HD double gr_quad(const double* W, const double* r) {
    double s = 0.0;
    for (int a = 0; a < 6; ++a) {
        double row = 0.0;
        for (int b = 0; b < 6; ++b) row = row + W[a * 6 + b] * r[b];
        s = s + r[a] * row;
    }
    return s;
}
// rho(s) and the weight w of the Huber rule (huber = 0: none)
LV_GR_HD double gr_rho(double s, double huber, double* w) {
    *w = 1.0;
    if (!(huber > 0.0)) return s;
    const double e = sqrt(s);
    if (e <= huber) return s;
    *w = huber / e;
    return 2.0 * huber * e - huber * huber;
}

// ---- residuals
LV_GR_HD void graph_edge_residual(const lv_graph_pose& xi, const lv_graph_pose& xj, const lv_graph_edge& e, double* r) {
    double Ri[9];
    gr_rot(xi.q, Ri);
    const double dt[3] = {xj.t[0] - xi.t[0], xj.t[1] - xi.t[1], xj.t[2] - xi.t[2]};
    double dv[3];
    gr_mtv(Ri, dt, dv);
    for (int k = 0; k < 3; ++k) r[k] = dv[k] - e.t[k];
    double qij[4], qe[4];
    gr_qmul_conj(xi.q, xj.q, qij);
    gr_qmul_conj(e.q, qij, qe);
    gr_qlog(qe, r + 3);
}
LV_GR_HD void graph_prior_residual(const lv_graph_pose& xi, const lv_graph_prior& p, double* r) {
    double Ri[9], Rl[3];
    gr_rot(xi.q, Ri);
    gr_mv(Ri, p.lever, Rl);
    for (int k = 0; k < 3; ++k) r[k] = xi.t[k] + Rl[k] - p.t[k];
    double qe[4];
    gr_qmul_conj(p.q, xi.q, qe);
    gr_qlog(qe, r + 3);
}

// ---- Jacobians (6 x 6, the zero blocks written)
LV_GR_HD void graph_edge_jacobians(const lv_graph_pose& xi, const lv_graph_pose& xj, const double* r, double* Ji, double* Jj) {
    double Ri[9], Rj[9], J[9], RjtRi[9], JR[9], dv[3], D[9];
    gr_rot(xi.q, Ri);
    gr_rot(xj.q, Rj);
    const double dt[3] = {xj.t[0] - xi.t[0], xj.t[1] - xi.t[1], xj.t[2] - xi.t[2]};
    gr_mtv(Ri, dt, dv);
    gr_hat(dv, D);
    gr_jrinv(r + 3, J);
    gr_mtm(Rj, Ri, RjtRi);
    gr_mm(J, RjtRi, JR);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            Ji[a * 6 + b] = -Ri[b * 3 + a];
            Ji[a * 6 + 3 + b] = D[a * 3 + b];
            Ji[(3 + a) * 6 + b] = 0.0;
            Ji[(3 + a) * 6 + 3 + b] = -JR[a * 3 + b];
            Jj[a * 6 + b] = Ri[b * 3 + a];
            Jj[a * 6 + 3 + b] = 0.0;
            Jj[(3 + a) * 6 + b] = 0.0;
            Jj[(3 + a) * 6 + 3 + b] = J[a * 3 + b];
        }
}
LV_GR_HD void graph_prior_jacobian(const lv_graph_pose& xi, const lv_graph_prior& p, const double* r, double* Ji) {
    double Ri[9], L[9], RL[9], J[9];
    gr_rot(xi.q, Ri);
    gr_hat(p.lever, L);
    gr_mm(Ri, L, RL);
    gr_jrinv(r + 3, J);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            Ji[a * 6 + b] = a == b ? 1.0 : 0.0;
            Ji[a * 6 + 3 + b] = -RL[a * 3 + b];
            Ji[(3 + a) * 6 + b] = 0.0;
            Ji[(3 + a) * 6 + 3 + b] = J[a * 3 + b];
        }
}

// C = A^T B of 6 x 6, each entry summed over k = 0..5 in order
LV_GR_HD void gr_atb6(const double* A, const double* B, double* C) {
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s = s + A[k * 6 + a] * B[k * 6 + b];
            C[a * 6 + b] = s;
        }
}
LV_GR_HD void gr_ab6(const double* A, const double* B, double* C) {
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s = s + A[a * 6 + k] * B[k * 6 + b];
            C[a * 6 + b] = s;
        }
}
LV_GR_HD void gr_atv6(const double* A, const double* v, double* o) {
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s = s + A[k * 6 + a] * v[k];
        o[a] = s;
    }
}
LV_GR_HD void gr_av6(const double* A, const double* v, double* o) {
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s = s + A[a * 6 + k] * v[k];
        o[a] = s;
    }
}

// ---- linearisation: what one lane writes for its factor
// An edge: 36 Hii, 36 Hjj, 36 Hij (= Ji^T W Jj, used transposed from j's side), 6 gi, 6 gj
constexpr int GRAPH_EDGE_LIN = 120;
constexpr int GRAPH_PRIOR_LIN = 42;   // 36 Hii, 6 gi
// returns rho; *s_out = s, *w_out = w; lin may be NULL (the cost alone)
LV_GR_HD double graph_edge_linearise(const lv_graph_pose& xi, const lv_graph_pose& xj, const lv_graph_edge& e, double* r, double* s_out,
                                     double* w_out, double* lin) {
    double W[36];
    graph_edge_residual(xi, xj, e, r);
    gr_info(e.info, W);
    const double s = gr_quad(W, r);
    double w;
    const double rho = gr_rho(s, e.huber, &w);
    *s_out = s;
    *w_out = w;
    if (!lin) return rho;
    double Ji[36], Jj[36], WJ[36], Wr[6];
    for (int k = 0; k < 36; ++k) W[k] = w * W[k];
    graph_edge_jacobians(xi, xj, r, Ji, Jj);
    gr_av6(W, r, Wr);
    gr_atv6(Ji, Wr, lin + 108);
    gr_atv6(Jj, Wr, lin + 114);
    gr_ab6(W, Ji, WJ);
    gr_atb6(Ji, WJ, lin);
    gr_ab6(W, Jj, WJ);
    gr_atb6(Jj, WJ, lin + 36);
    gr_atb6(Ji, WJ, lin + 72);
    return rho;
}
LV_GR_HD double graph_prior_linearise(const lv_graph_pose& xi, const lv_graph_prior& p, double* r, double* s_out, double* w_out, double* lin) {
    double W[36];
    graph_prior_residual(xi, p, r);
    gr_info(p.info, W);
    const double s = gr_quad(W, r);
    double w;
    const double rho = gr_rho(s, p.huber, &w);
    *s_out = s;
    *w_out = w;
    if (!lin) return rho;
    double Ji[36], WJ[36], Wr[6];
    for (int k = 0; k < 36; ++k) W[k] = w * W[k];
    graph_prior_jacobian(xi, p, r, Ji);
    gr_av6(W, r, Wr);
    gr_atv6(Ji, Wr, lin + 36);
    gr_ab6(W, Ji, WJ);
    gr_atb6(Ji, WJ, lin);
    return rho;
}

// ---- retraction: t <- t + dt, q <- q * exp(dth / 2), renormalised
LV_GR_HD void graph_retract(const lv_graph_pose& x, const double* d, lv_graph_pose* o) {
    double e[4], q[4];
    gr_qexp(d + 3, e);
    gr_qmul(x.q, e, q);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 3; ++k) o->t[k] = x.t[k] + d[k];
    for (int k = 0; k < 4; ++k) o->q[k] = q[k] / n;
}

// ---- the inverse of a symmetric 6 x 6 block by Cholesky, column by column (k = 0..5).  A pivot that is not positive (or not
// finite) gives that component a zero row and column in the inverse.  M: the block (its lower triangle is read); Minv: full.
LV_GR_HD void graph_block_inverse(const double* M, double* Minv) {
    double L[36], Li[36];
    bool live[6];
    for (int k = 0; k < 36; ++k) L[k] = Li[k] = 0.0;
    for (int k = 0; k < 6; ++k) {
        double d = M[k * 6 + k];
        for (int m = 0; m < k; ++m) d = d - L[k * 6 + m] * L[k * 6 + m];
        live[k] = d > 0.0 && d < INFINITY;
        if (!live[k]) continue;
        const double lk = sqrt(d);
        L[k * 6 + k] = lk;
        for (int a = k + 1; a < 6; ++a) {
            double v = M[a * 6 + k];
            for (int m = 0; m < k; ++m) v = v - L[a * 6 + m] * L[k * 6 + m];
            L[a * 6 + k] = v / lk;
        }
    }
    // Li = L^-1 over the live components (forward substitution, column by column)
    for (int c = 0; c < 6; ++c) {
        if (!live[c]) continue;
        Li[c * 6 + c] = 1.0 / L[c * 6 + c];
        for (int a = c + 1; a < 6; ++a) {
            if (!live[a]) continue;
            double v = 0.0;
            for (int m = c; m < a; ++m) v = v - L[a * 6 + m] * Li[m * 6 + c];
            Li[a * 6 + c] = v / L[a * 6 + a];
        }
    }
    gr_atb6(Li, Li, Minv);
}

// ---- the warp of a point by a node's correction: D = (R_now R_0^T, t_now - D_R t_0), 12 doubles, formed once per key
LV_GR_HD void graph_warp_delta(const lv_graph_pose& now, const lv_graph_pose& x0, double* D) {
    double Rn[9], R0[9], t[3];
    bool same = true;   // a node that has not moved: the identity, exactly
    for (int k = 0; k < 3; ++k) same = same && now.t[k] == x0.t[k];
    for (int k = 0; k < 4; ++k) same = same && now.q[k] == x0.q[k];
    if (same) {
        for (int k = 0; k < 12; ++k) D[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        return;
    }
    gr_rot(now.q, Rn);
    gr_rot(x0.q, R0);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[i * 3 + j] = Rn[i * 3] * R0[j * 3] + Rn[i * 3 + 1] * R0[j * 3 + 1] + Rn[i * 3 + 2] * R0[j * 3 + 2];
    gr_mv(D, x0.t, t);
    for (int k = 0; k < 3; ++k) D[9 + k] = now.t[k] - t[k];
}
LV_GR_HD void graph_warp_point(const double* D, const float* p, float* o) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    for (int k = 0; k < 3; ++k) o[k] = (float)(D[k * 3] * x + D[k * 3 + 1] * y + D[k * 3 + 2] * z + D[9 + k]);
}

// ---- the argument rules
inline void default_graph_params(lv_graph_params* p) {
    if (!p) return;
    p->max_iterations = 100;
    p->pcg_max_iterations = 1000;
    p->pcg_tol = 1e-2;
    p->step_tol = 1e-8;
    p->lambda_init = 1e-4;
    p->lambda_min = 1e-10;
    p->lambda_max = 1e8;
}
inline int graph_params_ok(const lv_graph_params* p) {
    const auto fin = [](double v) { return v - v == 0.0; };
    if (p->max_iterations < 1 || p->max_iterations > 10000) { set_error("graph params: max_iterations %d outside 1..10000", p->max_iterations); return LV_EINVAL; }
    if (p->pcg_max_iterations < 1 || p->pcg_max_iterations > 100000) { set_error("graph params: pcg_max_iterations %d outside 1..100000", p->pcg_max_iterations); return LV_EINVAL; }
    if (!(p->pcg_tol > 0.0 && p->pcg_tol < 1.0)) { set_error("graph params: pcg_tol must lie in (0, 1)"); return LV_EINVAL; }
    if (!(p->step_tol >= 0.0 && fin(p->step_tol))) { set_error("graph params: step_tol must be finite and >= 0"); return LV_EINVAL; }
    if (!(p->lambda_min > 0.0 && p->lambda_min <= p->lambda_init && p->lambda_init <= p->lambda_max && fin(p->lambda_max))) {
        set_error("graph params: 0 < lambda_min <= lambda_init <= lambda_max < inf");
        return LV_EINVAL;
    }
    return LV_OK;
}

namespace graph_detail {
inline bool finite_all(const double* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!(v[k] - v[k] == 0.0)) return false;
    return true;
}
inline bool unit_quat(const double* q) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    return fabs(n - 1.0) <= GRAPH_QUAT_TOL;
}
// the 21-entry index of diagonal entry a
inline int diag_at(int a) { return a * 6 - a * (a - 1) / 2; }
inline const char* info_bad(const double* u) {
    if (!finite_all(u, 21)) return "info: a non-finite number";
    for (int a = 0; a < 6; ++a)
        if (u[diag_at(a)] < 0.0) return "info: a negative diagonal entry";
    return nullptr;
}
}  // namespace graph_detail

// The whole of lv_graph_set's judgement; LV_OK or LV_EINVAL with the record and the field in the message
inline int graph_check(const lv_graph_pose* poses, size_t n, const uint8_t* fixed, const lv_graph_edge* edges, size_t n_edges,
                       const lv_graph_prior* priors, size_t n_priors) {
    using namespace graph_detail;
    if (n == 0 || n > GRAPH_MAX_NODES) { set_error("graph: n = %zu outside 1..2^20", n); return LV_EINVAL; }
    if (n_edges > GRAPH_MAX_EDGES) { set_error("graph: n_edges = %zu above 2^22", n_edges); return LV_EINVAL; }
    if (n_priors > GRAPH_MAX_PRIORS) { set_error("graph: n_priors = %zu above 2^20", n_priors); return LV_EINVAL; }
    if (!poses) { set_error("graph: null poses"); return LV_EINVAL; }
    if (n_edges && !edges) { set_error("graph: null edges"); return LV_EINVAL; }
    if (n_priors && !priors) { set_error("graph: null priors"); return LV_EINVAL; }
    for (size_t k = 0; k < n; ++k) {
        if (!finite_all(poses[k].t, 3)) { set_error("graph: pose %zu: t: a non-finite number", k); return LV_EINVAL; }
        if (!finite_all(poses[k].q, 4)) { set_error("graph: pose %zu: q: a non-finite number", k); return LV_EINVAL; }
        if (!unit_quat(poses[k].q)) { set_error("graph: pose %zu: q: norm off 1 by more than 1e-6", k); return LV_EINVAL; }
    }
    for (size_t k = 0; k < n_edges; ++k) {
        const lv_graph_edge& e = edges[k];
        if (e.i >= n) { set_error("graph: edge %zu: i = %u out of range (n = %zu)", k, e.i, n); return LV_EINVAL; }
        if (e.j >= n) { set_error("graph: edge %zu: j = %u out of range (n = %zu)", k, e.j, n); return LV_EINVAL; }
        if (e.i == e.j) { set_error("graph: edge %zu: i == j (%u)", k, e.i); return LV_EINVAL; }
        if (!finite_all(e.t, 3)) { set_error("graph: edge %zu: t: a non-finite number", k); return LV_EINVAL; }
        if (!finite_all(e.q, 4)) { set_error("graph: edge %zu: q: a non-finite number", k); return LV_EINVAL; }
        if (!unit_quat(e.q)) { set_error("graph: edge %zu: q: norm off 1 by more than 1e-6", k); return LV_EINVAL; }
        if (const char* why = info_bad(e.info)) { set_error("graph: edge %zu: %s", k, why); return LV_EINVAL; }
        if (!(e.huber >= 0.0 && e.huber - e.huber == 0.0)) { set_error("graph: edge %zu: huber: must be finite and >= 0", k); return LV_EINVAL; }
    }
    for (size_t k = 0; k < n_priors; ++k) {
        const lv_graph_prior& p = priors[k];
        if (p.i >= n) { set_error("graph: prior %zu: i = %u out of range (n = %zu)", k, p.i, n); return LV_EINVAL; }
        if (p.reserved != 0) { set_error("graph: prior %zu: reserved must be 0", k); return LV_EINVAL; }
        if (!finite_all(p.t, 3)) { set_error("graph: prior %zu: t: a non-finite number", k); return LV_EINVAL; }
        if (!finite_all(p.q, 4)) { set_error("graph: prior %zu: q: a non-finite number", k); return LV_EINVAL; }
        if (!unit_quat(p.q)) { set_error("graph: prior %zu: q: norm off 1 by more than 1e-6", k); return LV_EINVAL; }
        if (!finite_all(p.lever, 3)) { set_error("graph: prior %zu: lever: a non-finite number", k); return LV_EINVAL; }
        if (const char* why = info_bad(p.info)) { set_error("graph: prior %zu: %s", k, why); return LV_EINVAL; }
        if (!(p.huber >= 0.0 && p.huber - p.huber == 0.0)) { set_error("graph: prior %zu: huber: must be finite and >= 0", k); return LV_EINVAL; }
    }
    bool held = n_priors > 0;
    if (fixed)
        for (size_t k = 0; k < n && !held; ++k) held = fixed[k] != 0;
    if (!held) { set_error("graph: neither a fixed node nor a prior: the gauge is free"); return LV_EINVAL; }
    return LV_OK;
}

// The incidence lists (CSR): node k's entries are items[start[k] .. start[k + 1]): its edges by ascending edge id (an edge is in
// the lists of both its ends), then its priors by ascending id.  start: n + 1, items: 2 n_edges + n_priors.  Returns the length
// of the longest list.
inline uint32_t graph_incidence(size_t n, const lv_graph_edge* edges, size_t n_edges, const lv_graph_prior* priors, size_t n_priors,
                                uint32_t* start, uint32_t* items) {
    for (size_t k = 0; k <= n; ++k) start[k] = 0;
    for (size_t e = 0; e < n_edges; ++e) {
        ++start[edges[e].i + 1];
        ++start[edges[e].j + 1];
    }
    for (size_t p = 0; p < n_priors; ++p) ++start[priors[p].i + 1];
    uint32_t longest = 0;
    for (size_t k = 0; k < n; ++k) {
        longest = start[k + 1] > longest ? start[k + 1] : longest;
        start[k + 1] += start[k];
    }
    // fill[k] runs in start[k + 1]'s place while filling: walk back afterwards
    for (size_t k = n; k > 0; --k) start[k] = start[k - 1];
    for (size_t e = 0; e < n_edges; ++e) {
        items[start[edges[e].i + 1]++] = ((uint32_t)e << 2) | GRAPH_SIDE_I;
        items[start[edges[e].j + 1]++] = ((uint32_t)e << 2) | GRAPH_SIDE_J;
    }
    for (size_t p = 0; p < n_priors; ++p) items[start[priors[p].i + 1]++] = ((uint32_t)p << 2) | GRAPH_PRIOR;
    return longest;
}

// the loop's acceptance rule
inline bool graph_accept(double cost_new, double cost_old) {
    return cost_new <= cost_old + 64.0 * 2.220446049250313e-16 * fabs(cost_old);
}

// ---- the store (host side in lv_graph.hip)
// What the conjugate-gradient kernels keep between launches.  rz, alpha and stop are held twice, by the parity of the iteration:
// a launch reads the slot of its iteration and writes the other, so no launch reads a word that the same launch writes.
struct GraphScalars {
    double rz[2];       // r^T z
    double alpha[2];    // of the iteration (0: p^T A p was not positive, the solve ends)
    double rz0;         // r^T z before the first iteration
    double cost;        // 1/2 sum rho of the last linearisation
    double step;        // max-norm of the last increment
    uint32_t stop[2];   // the solve has stopped: every later launch of the chunk returns at once
    uint32_t iters;     // iterations done by this solve
    uint32_t pad;
};

constexpr int GRAPH_PCG_CHUNK = 16;   // iterations enqueued between two looks at the stop flag

struct GraphStore {
    bool set = false;
    size_t n = 0, n_edges = 0, n_priors = 0;
    uint32_t n_long = 0;     // free nodes whose list is longer than GRAPH_WAVE_LIST
    lv_graph_info info{};
    DevBuf<lv_graph_pose> d_x, d_x0, d_xt;   // current, as given, trial
    DevBuf<uint8_t> d_fixed;
    DevBuf<lv_graph_edge> d_edges;
    DevBuf<lv_graph_prior> d_priors;
    DevBuf<uint32_t> d_ij;                   // 2 per edge: its ends
    DevBuf<uint32_t> d_start, d_items, d_long;
    DevBuf<double> d_elin, d_plin, d_s;      // per factor: blocks; s (edges, then priors)
    DevBuf<double> d_Hd, d_g, d_Minv;        // per node: 36, 6, 36
    DevBuf<double> d_d, d_r, d_z, d_p, d_Ap; // per node: 6 each
    DevBuf<double> d_part[2];                // workgroup partials
    DevBuf<GraphScalars> d_scal;
    PinBuf<GraphScalars> h_scal;
    // lv_graph_warp_points
    PointStage warp_pts;
    DevBuf<uint32_t> d_keys;
    DevBuf<double> d_D;                      // 12 per node
    DevBuf<float> d_out;

    int assign(hipStream_t stream, const lv_graph_pose* poses, size_t n, const uint8_t* fixed, const lv_graph_edge* edges, size_t n_edges,
               const lv_graph_prior* priors, size_t n_priors);
    int optimise(hipStream_t stream, const lv_graph_params& prm);
    int fetch(hipStream_t stream, lv_graph_pose* poses);
    int chi2(hipStream_t stream, double* edge_s, double* prior_s);
    int warp(hipStream_t stream, const void* pts, size_t stride, const uint32_t* keys, size_t count, float* out);
    void clear() { set = false; info = lv_graph_info{}; info.status = -1; }
    void release();

   private:
    int linearise(hipStream_t stream, const lv_graph_pose* x, bool full);
    int read_scalars(hipStream_t stream);
};

}  // namespace lv
