// tests/emu/graph_emu.cpp — the rule of limo-velo_amd/csrc/lv_graph.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h, with -fsanitize=address,undefined).  tests/test_graph_host.py holds its output to tests/graph_ref.py.
//
// stdin: "<mode> <count>", then count records; every double in decimal with 17 significant digits, printed the same way.
//   0  edge:    xi[7] xj[7] i j t[3] q[4] info[21] huber      -> r[6] s w rho, then the 120 values of graph_edge_linearise
//   1  prior:   xi[7] i t[3] q[4] lever[3] info[21] huber      -> r[6] s w rho, then the 42 values of graph_prior_linearise
//   2  retract: x[7] d[6]                                      -> the pose
//   3  inverse: M[36]                                          -> graph_block_inverse
//   4  warp:    now[7] x0[7] p[3]                              -> the point (f32, 9 digits)
//   5  params:  max_iterations pcg_max_iterations pcg_tol step_tol lambda_init lambda_min lambda_max -> "ok" or "bad: <why>"
//   6  graph (count ignored): n, n poses[7], has_fixed, n flags when has_fixed; n_edges, edges as in 0 without the poses; n_priors,
//      priors "i reserved" + as in 1 without the pose and i -> "bad: <why>", or "ok <longest>", the n + 1 starts, the items
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "lv_graph.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace lv {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace lv

using namespace lv;

static double rd() {
    double v = 0;
    if (scanf("%lf", &v) != 1) exit(2);
    return v;
}
static long long ri() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) exit(2);
    return v;
}
static void rv(double* p, int n) {
    for (int k = 0; k < n; ++k) p[k] = rd();
}
static void pv(const double* p, int n) {
    for (int k = 0; k < n; ++k) printf("%.17g%c", p[k], k + 1 == n ? '\n' : ' ');
}
static lv_graph_pose read_pose() {
    lv_graph_pose x;
    rv(x.t, 3);
    rv(x.q, 4);
    return x;
}
static lv_graph_edge read_edge() {
    lv_graph_edge e;
    e.i = (uint32_t)ri();
    e.j = (uint32_t)ri();
    rv(e.t, 3);
    rv(e.q, 4);
    rv(e.info, 21);
    e.huber = rd();
    return e;
}
static lv_graph_prior read_prior(bool with_reserved) {
    lv_graph_prior p;
    p.i = (uint32_t)ri();
    p.reserved = with_reserved ? (uint32_t)ri() : 0u;
    rv(p.t, 3);
    rv(p.q, 4);
    rv(p.lever, 3);
    rv(p.info, 21);
    p.huber = rd();
    return p;
}

int main() {
    const int mode = (int)ri();
    const long long count = ri();
    if (mode == 6) {
        const size_t n = (size_t)ri();
        std::vector<lv_graph_pose> poses(n);
        for (auto& x : poses) x = read_pose();
        const bool has_fixed = ri() != 0;
        std::vector<uint8_t> fixed(n, 0);
        if (has_fixed)
            for (auto& f : fixed) f = (uint8_t)ri();
        std::vector<lv_graph_edge> edges((size_t)ri());
        for (auto& e : edges) e = read_edge();
        std::vector<lv_graph_prior> priors((size_t)ri());
        for (auto& p : priors) p = read_prior(true);
        const int rc = graph_check(poses.data(), n, has_fixed ? fixed.data() : nullptr, edges.data(), edges.size(), priors.data(), priors.size());
        if (rc) {
            printf("bad: %s\n", g_err);
            return 0;
        }
        std::vector<uint32_t> start(n + 1), items(2 * edges.size() + priors.size());
        const uint32_t longest = graph_incidence(n, edges.data(), edges.size(), priors.data(), priors.size(), start.data(), items.data());
        printf("ok %u\n", longest);
        for (size_t k = 0; k <= n; ++k) printf("%u%c", start[k], k == n ? '\n' : ' ');
        for (size_t k = 0; k < items.size(); ++k) printf("%u ", items[k]);
        printf("\n");
        return 0;
    }
    for (long long c = 0; c < count; ++c) {
        if (mode == 0) {
            const lv_graph_pose xi = read_pose(), xj = read_pose();
            const lv_graph_edge e = read_edge();
            double r[6], s, w, lin[GRAPH_EDGE_LIN], r2[6], s2, w2;
            const double rho = graph_edge_linearise(xi, xj, e, r, &s, &w, lin);
            const double rho2 = graph_edge_linearise(xi, xj, e, r2, &s2, &w2, nullptr);   // the cost alone: the same numbers
            if (rho2 != rho || s2 != s || w2 != w) return 3;
            const double head[3] = {s, w, rho};
            pv(r, 6);
            pv(head, 3);
            pv(lin, GRAPH_EDGE_LIN);
        } else if (mode == 1) {
            const lv_graph_pose xi = read_pose();
            const lv_graph_prior p = read_prior(false);
            double r[6], s, w, lin[GRAPH_PRIOR_LIN];
            const double rho = graph_prior_linearise(xi, p, r, &s, &w, lin);
            const double head[3] = {s, w, rho};
            pv(r, 6);
            pv(head, 3);
            pv(lin, GRAPH_PRIOR_LIN);
        } else if (mode == 2) {
            const lv_graph_pose x = read_pose();
            double d[6];
            rv(d, 6);
            lv_graph_pose o;
            graph_retract(x, d, &o);
            pv(o.t, 3);
            pv(o.q, 4);
        } else if (mode == 3) {
            double M[36], Mi[36];
            rv(M, 36);
            graph_block_inverse(M, Mi);
            pv(Mi, 36);
        } else if (mode == 4) {
            const lv_graph_pose now = read_pose(), x0 = read_pose();
            double D[12];
            graph_warp_delta(now, x0, D);
            const float p[3] = {(float)rd(), (float)rd(), (float)rd()};
            float o[3];
            graph_warp_point(D, p, o);
            printf("%.9g %.9g %.9g\n", o[0], o[1], o[2]);
        } else if (mode == 5) {
            lv_graph_params p;
            p.max_iterations = (int32_t)ri();
            p.pcg_max_iterations = (int32_t)ri();
            p.pcg_tol = rd();
            p.step_tol = rd();
            p.lambda_init = rd();
            p.lambda_min = rd();
            p.lambda_max = rd();
            if (graph_params_ok(&p)) printf("bad: %s\n", g_err);
            else printf("ok\n");
        } else {
            return 2;
        }
    }
    return 0;
}
