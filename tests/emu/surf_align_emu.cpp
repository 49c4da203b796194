// tests/emu/surf_align_emu.cpp — the rule of limo-velo_amd/csrc/lv_surf_align.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++
// through tests/emu/hip/hip_runtime.h, with -fsanitize=address,undefined).  tests/test_surf_align_host.py holds its output to
// tests/surf_align_ref.py.
//
// stdin: "<mode>", then the mode's input; doubles are printed with 17 significant digits.
//   0  sample:   volume, n, n world points (f64)           -> per point "status d n_x n_y n_z"
//   1  evaluate: volume, m, m source points, pose[7], max_dist, huber -> acc[28], then n_in, then the cost
//   2  align params: count, then count x params            -> "ok" or "bad: <why>"
//   3  align arguments: count, then count x (has_src stride n_src has_guesses K has_results has_best q[4] t0) -> "ok" / "bad: <why>"
//   4  sample arguments: count, then count x (min_weight has_pts stride n has_out has_status) -> "ok" / "bad: <why>"
//   5  align:    as 1 up to the source points, then params, K, K poses -> per guess "pose[7] cost last_step lambda",
//                "n_in status accepted rejected" and info[21]; then best[2]
//   6  defaults  -> the default params
// volume: origin[3] resolution nx ny nz min_weight, then nx * ny * nz values of S, then of W
// params: min_weight max_iterations min_points max_dist huber step_tol lambda_init lambda_min lambda_max
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "lv_surf_align.hpp"

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

struct Volume {
    TsdfGrid g{};
    int32_t min_weight = 1;
    std::vector<int32_t> S, W;
    SurfView view() const { return surf_view_of(g, min_weight, S.data(), W.data()); }
};
static Volume read_volume() {
    Volume v;
    for (int a = 0; a < 3; ++a) v.g.occ.origin[a] = (float)rd();
    v.g.occ.resolution = (float)rd();
    v.g.occ.nx = (int)ri();
    v.g.occ.ny = (int)ri();
    v.g.occ.nz = (int)ri();
    v.min_weight = (int32_t)ri();
    const size_t n = grid_cells(v.g.occ);
    v.S.resize(n);
    v.W.resize(n);
    for (auto& s : v.S) s = (int32_t)ri();
    for (auto& w : v.W) w = (int32_t)ri();
    return v;
}
static lv_surf_align_params read_params() {
    lv_surf_align_params p{};
    p.min_weight = (int32_t)ri();
    p.max_iterations = (int32_t)ri();
    p.min_points = (uint32_t)ri();
    p.max_dist = rd();
    p.huber = rd();
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


int main() {
    const int mode = (int)ri();
    if (mode == 0) {
        const Volume vol = read_volume();
        const SurfView v = vol.view();
        for (long long c = ri(); c > 0; --c) {
            const double x[3] = {rd(), rd(), rd()};
            double row[4];
            const int s = surf_sample(v, x, row[0], row + 1);
            printf("%d ", s);
            pv(row, 4);
        }
    } else if (mode == 1 || mode == 5) {
        const Volume vol = read_volume();
        const std::vector<float> src = read_points();
        const uint32_t n_src = (uint32_t)(src.size() / 3);
        if (mode == 1) {
            const lv_graph_pose x = read_pose();
            lv_surf_align_params a{};
            a.max_dist = rd();
            a.huber = rd();
            const SurfAlignRule q = surf_align_rule_of(a, vol.view(), n_src);
            double acc[ALIGN_ACC];
            const uint32_t n_in = align_evaluate(q, src.data(), n_src, x, acc);
            pv(acc, ALIGN_ACC);
            printf("%u\n", n_in);
            const double cost = q.objective(acc, n_in);
            pv(&cost, 1);
            return 0;
        }
        const lv_surf_align_params prm = read_params();
        Volume with = vol;
        with.min_weight = prm.min_weight;
        const SurfAlignRule q = surf_align_rule_of(prm, with.view(), n_src);
        const size_t K = (size_t)ri();
        std::vector<lv_surf_align_result> res(K);
        for (size_t k = 0; k < K; ++k) {
            const lv_surf_align_result r = align_one(q, [&](const lv_graph_pose& x, double* tot) { return align_evaluate(q, src.data(), n_src, x, tot); }, read_pose());
            if (r.status == ALIGN_RUNNING) return 3;   // the loop must have ended by now
            res[k] = r;
            const double head[10] = {r.pose.t[0], r.pose.t[1], r.pose.t[2], r.pose.q[0], r.pose.q[1], r.pose.q[2], r.pose.q[3], r.cost, r.last_step, r.lambda};
            pv(head, 10);
            printf("%u %d %u %u\n", r.n_in, r.status, r.accepted, r.rejected);
            pv(r.info, 21);
        }
        int32_t best[2];
        align_best<SurfAlignRule>(res.data(), K, best);
        printf("%d %d\n", best[0], best[1]);
    } else if (mode == 2) {
        for (long long c = ri(); c > 0; --c) {
            const lv_surf_align_params p = read_params();
            const char* why = surf_check_align_params(&p);
            printf("%s%s\n", why ? "bad: " : "ok", why ? why : "");
        }
    } else if (mode == 3) {
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
            std::vector<lv_surf_align_result> res(1);
            float pt[3] = {0, 0, 0};
            int32_t best[2];
            const int rc = align_check_args("lv_surf_align", has_src ? pt : nullptr, stride, n_src, has_guesses ? g.data() : nullptr, K,
                                            has_results ? res.data() : nullptr, has_best ? best : nullptr);
            if (rc) printf("bad: %s\n", g_err);
            else printf("ok\n");
        }
    } else if (mode == 4) {
        for (long long c = ri(); c > 0; --c) {
            const int min_weight = (int)ri();
            const bool has_pts = ri() != 0;
            const size_t stride = (size_t)ri(), n = (size_t)ri();
            const bool has_out = ri() != 0, has_status = ri() != 0;
            float pt[3] = {0, 0, 0};
            double out[4];
            uint8_t st[1];
            const int rc = surf_check_sample_args(min_weight, has_pts ? pt : nullptr, stride, n, has_out ? out : nullptr, has_status ? st : nullptr);
            if (rc) printf("bad: %s\n", g_err);
            else printf("ok\n");
        }
    } else if (mode == 6) {
        lv_surf_align_params p;
        default_surf_align_params(&p);
        printf("%d %d %u %d\n", p.min_weight, p.max_iterations, p.min_points, p.reserved);
        const double d[6] = {p.max_dist, p.huber, p.step_tol, p.lambda_init, p.lambda_min, p.lambda_max};
        pv(d, 6);
    } else {
        return 2;
    }
    return 0;
}
