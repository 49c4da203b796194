// tests/emu/ndt_emu.cpp — the rule of limo-velo_amd/csrc/lv_ndt.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h, with -fsanitize=address,undefined).  tests/test_ndt_host.py holds its output to tests/ndt_ref.py.
//
// stdin: "<mode>", then the mode's input; doubles are printed with 17 significant digits.
//   0  target:   params, n, n points                       -> "used ignored used_voxels sparse_voxels", then per occupied voxel
//                                                             "cell n S1[3] S2[6]" and "mean[3] cov[6] icov[6]"
//   1  evaluate: params, n, n points, m, m source points, pose[7], search, d2 -> acc[28], then n_in
//   2  params:   count, then count x params                -> "ok" or "bad: <why>"
//   3  align params: count, then count x (search max_iterations d2 step_tol lambda_init lambda_min lambda_max) -> "ok" / "bad: <why>"
//   4  align arguments: count, then count x (has_src stride n_src has_guesses K has_results has_best q[4] t0) -> "ok" / "bad: <why>"
//   5  align:    as 1 up to the source points, then the align params as in 3, K, K poses -> per guess
//                "pose[7] score last_step lambda", "n_in status accepted rejected" and info[21]; then best[2]
// params: origin[3] resolution nx ny nz min_points reg
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "lv_ndt.hpp"

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
static void pv(const double* p, int n) {
    for (int k = 0; k < n; ++k) printf("%.17g%c", p[k], k + 1 == n ? '\n' : ' ');
}
static lv_ndt_params read_params() {
    lv_ndt_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = (float)rd();
    p.resolution = (float)rd();
    p.nx = (int32_t)ri();
    p.ny = (int32_t)ri();
    p.nz = (int32_t)ri();
    p.min_points = (int32_t)ri();
    p.reg = rd();
    return p;
}
static lv_ndt_align_params read_align_params() {
    lv_ndt_align_params p{};
    p.search = (int32_t)ri();
    p.max_iterations = (int32_t)ri();
    p.d2 = rd();
    p.step_tol = rd();
    p.lambda_init = rd();
    p.lambda_min = rd();
    p.lambda_max = rd();
    return p;
}
static std::vector<float> read_points() {
    std::vector<float> v(3 * (size_t)ri());
    for (auto& f : v) f = (float)rd();
    return v;
}
static lv_graph_pose read_pose() {
    lv_graph_pose x;
    for (int k = 0; k < 3; ++k) x.t[k] = rd();
    for (int k = 0; k < 4; ++k) x.q[k] = rd();
    return x;
}

struct Target {
    NdtGrid g;
    std::vector<uint32_t> n;
    std::vector<long long> S1, S2;
    std::vector<double> mean, cov, icov;
    uint64_t used = 0, ignored = 0, used_voxels = 0, sparse_voxels = 0;
};

// what ndt_moments_kernel and ndt_gauss_kernel do, one "lane" after the other
static Target build(const lv_ndt_params& p, const std::vector<float>& pts) {
    Target T;
    T.g = ndt_grid_of(p);
    const size_t nc = grid_cells(T.g);
    T.n.assign(nc, 0);
    T.S1.assign(nc * 3, 0);
    T.S2.assign(nc * 6, 0);
    T.mean.assign(nc * 3, 0.0);
    T.cov.assign(nc * 6, 0.0);
    T.icov.assign(nc * 6, 0.0);
    for (size_t i = 0; i < pts.size() / 3; ++i) {
        uint32_t cell;
        int32_t c[3], r[3];
        if (!ndt_point(T.g, &pts[3 * i], cell, c, r)) {
            ++T.ignored;
            continue;
        }
        ++T.used;
        ++T.n[cell];
        int k = 0;
        for (int a = 0; a < 3; ++a) {
            T.S1[(size_t)cell * 3 + a] += r[a];
            for (int b = a; b < 3; ++b, ++k) T.S2[(size_t)cell * 6 + k] += r[a] * r[b];
        }
    }
    for (size_t cell = 0; cell < nc; ++cell) {
        int c[3];
        grid_ijk(T.g, (uint32_t)cell, c[0], c[1], c[2]);
        const bool used = ndt_gaussian(T.g, c, T.n[cell], &T.S1[cell * 3], &T.S2[cell * 6], &T.mean[cell * 3], &T.cov[cell * 6], &T.icov[cell * 6]);
        T.used_voxels += used;
        T.sparse_voxels += !used && T.n[cell] > 0;
    }
    return T;
}


int main() {
    const int mode = (int)ri();
    if (mode == 0) {
        const lv_ndt_params p = read_params();
        const Target T = build(p, read_points());
        printf("%llu %llu %llu %llu\n", (unsigned long long)T.used, (unsigned long long)T.ignored, (unsigned long long)T.used_voxels,
               (unsigned long long)T.sparse_voxels);
        for (size_t c = 0; c < T.n.size(); ++c) {
            if (!T.n[c]) continue;
            printf("%zu %u", c, T.n[c]);
            for (int k = 0; k < 3; ++k) printf(" %lld", T.S1[c * 3 + k]);
            for (int k = 0; k < 6; ++k) printf(" %lld", T.S2[c * 6 + k]);
            printf("\n");
            double row[15];
            for (int k = 0; k < 3; ++k) row[k] = T.mean[c * 3 + k];
            for (int k = 0; k < 6; ++k) row[3 + k] = T.cov[c * 6 + k], row[9 + k] = T.icov[c * 6 + k];
            pv(row, 15);
        }
    } else if (mode == 1 || mode == 5) {
        const lv_ndt_params p = read_params();
        const Target T = build(p, read_points());
        const std::vector<float> src = read_points();
        const NdtView v{T.g, T.mean.data(), T.icov.data()};
        if (mode == 1) {
            const lv_graph_pose x = read_pose();
            lv_ndt_align_params a{};
            a.search = (int32_t)ri();
            a.d2 = rd();
            double acc[ALIGN_ACC];
            const uint32_t n_in = align_evaluate(ndt_rule_of(a, v), src.data(), src.size() / 3, x, acc);
            pv(acc, ALIGN_ACC);
            printf("%u\n", n_in);
            return 0;
        }
        const NdtRule q = ndt_rule_of(read_align_params(), v);
        const size_t K = (size_t)ri();
        std::vector<lv_ndt_result> res(K);
        for (size_t k = 0; k < K; ++k) {
            const lv_ndt_result r = align_one(q, [&](const lv_graph_pose& x, double* tot) { return align_evaluate(q, src.data(), src.size() / 3, x, tot); }, read_pose());
            if (r.status == ALIGN_RUNNING) return 3;   // the loop must have ended by now
            res[k] = r;
            const double head[10] = {r.pose.t[0], r.pose.t[1], r.pose.t[2], r.pose.q[0], r.pose.q[1], r.pose.q[2], r.pose.q[3], r.score, r.last_step, r.lambda};
            pv(head, 10);
            printf("%u %d %u %u\n", r.n_in, r.status, r.accepted, r.rejected);
            pv(r.info, 21);
        }
        int32_t best[2];
        align_best<NdtRule>(res.data(), K, best);
        printf("%d %d\n", best[0], best[1]);
    } else if (mode == 2) {
        for (long long c = ri(); c > 0; --c) {
            const lv_ndt_params p = read_params();
            const char* why = ndt_check_params(&p);
            printf("%s%s\n", why ? "bad: " : "ok", why ? why : "");
        }
    } else if (mode == 3) {
        for (long long c = ri(); c > 0; --c) {
            const lv_ndt_align_params p = read_align_params();
            const char* why = ndt_check_align_params(&p);
            printf("%s%s\n", why ? "bad: " : "ok", why ? why : "");
        }
    } else if (mode == 4) {
        for (long long c = ri(); c > 0; --c) {
            const bool has_src = ri() != 0;
            const size_t stride = (size_t)ri(), n_src = (size_t)ri();
            const bool has_guesses = ri() != 0;
            const size_t K = (size_t)ri();
            const bool has_results = ri() != 0, has_best = ri() != 0;
            std::vector<lv_graph_pose> g(K ? K : 1);
            for (auto& x : g) x = lv_graph_pose{{0, 0, 0}, {0, 0, 0, 1}};
            for (int k = 0; k < 4; ++k) g.back().q[k] = rd();
            g.back().t[0] = rd();
            std::vector<lv_ndt_result> res(1);
            float pt[3] = {0, 0, 0};
            int32_t best[2];
            const int rc = align_check_args("lv_ndt_align", has_src ? pt : nullptr, stride, n_src, has_guesses ? g.data() : nullptr, K,
                                            has_results ? res.data() : nullptr, has_best ? best : nullptr);
            if (rc) printf("bad: %s\n", g_err);
            else printf("ok\n");
        }
    } else {
        return 2;
    }
    return 0;
}
