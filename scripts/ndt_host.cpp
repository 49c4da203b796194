// scripts/ndt_host.cpp — the NDT rule of limo-velo_amd/csrc/lv_ndt.hpp on one CPU core (g++ -O2 -ffp-contract=off through
// tests/emu/hip/hip_runtime.h): what scripts/ndt_timing.py times the device against and checks it with.
//
//   ndt_host <target.f32> <source.f32> <moments.bin> ox oy oz resolution nx ny nz min_points reg search d2 iterations K  < K poses
// target / source: packed x, y, z as f32.  Builds the target (the moments go to moments.bin: n uint32, S1 int64 x 3, S2 int64 x 6,
// by voxel), then runs the loop of lv_ndt_align from every pose with step_tol = 0 and the default lambdas.
// stdout: "build_ms <ms>", "eval_ms <ms per evaluation of one hypothesis>", then per pose "t[3] q[4] score n_in status accepted rejected".
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "lv_ndt.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace lv {
void set_error(const char*, ...) {}
}  // namespace lv

using namespace lv;
using Clock = std::chrono::steady_clock;

static std::vector<float> read_f32(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<float> v((size_t)bytes / 4);
    if (fread(v.data(), 4, v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

int main(int argc, char** argv) {
    if (argc != 17) return 2;
    const std::vector<float> tgt = read_f32(argv[1]), src = read_f32(argv[2]);
    lv_ndt_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = (float)atof(argv[4 + a]);
    p.resolution = (float)atof(argv[7]);
    p.nx = atoi(argv[8]);
    p.ny = atoi(argv[9]);
    p.nz = atoi(argv[10]);
    p.min_points = atoi(argv[11]);
    p.reg = atof(argv[12]);
    lv_ndt_align_params prm;
    default_ndt_align_params(&prm);
    prm.search = atoi(argv[13]);
    prm.d2 = atof(argv[14]);
    prm.max_iterations = atoi(argv[15]);
    prm.step_tol = 0.0;
    const int K = atoi(argv[16]);
    if (ndt_check_params(&p) || ndt_check_align_params(&prm)) return 3;

    const NdtGrid g = ndt_grid_of(p);
    const size_t nc = grid_cells(g);
    std::vector<uint32_t> n(nc, 0);
    std::vector<long long> S1(nc * 3, 0), S2(nc * 6, 0);
    std::vector<double> mean(nc * 3), cov(nc * 6), icov(nc * 6);
    auto t0 = Clock::now();
    for (size_t i = 0; i < tgt.size() / 3; ++i) {
        uint32_t cell;
        int32_t c[3], r[3];
        if (!ndt_point(g, &tgt[3 * i], cell, c, r)) continue;
        ++n[cell];
        int k = 0;
        for (int a = 0; a < 3; ++a) {
            S1[(size_t)cell * 3 + a] += r[a];
            for (int b = a; b < 3; ++b, ++k) S2[(size_t)cell * 6 + k] += r[a] * r[b];
        }
    }
    for (size_t cell = 0; cell < nc; ++cell) {
        int c[3];
        grid_ijk(g, (uint32_t)cell, c[0], c[1], c[2]);
        ndt_gaussian(g, c, n[cell], &S1[cell * 3], &S2[cell * 6], &mean[cell * 3], &cov[cell * 6], &icov[cell * 6]);
    }
    printf("build_ms %.3f\n", ms_since(t0));
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 2;
    fwrite(n.data(), 4, nc, f);
    fwrite(S1.data(), 8, nc * 3, f);
    fwrite(S2.data(), 8, nc * 6, f);
    fclose(f);

    const NdtRule q = ndt_rule_of(prm, NdtView{g, mean.data(), icov.data()});
    double eval_ms = 0.0;
    long evals = 0;
    const auto evaluate = [&](const lv_graph_pose& x, double* tot) {
        t0 = Clock::now();
        const uint32_t n_in = align_evaluate(q, src.data(), src.size() / 3, x, tot);
        eval_ms += ms_since(t0);
        ++evals;
        return n_in;
    };
    std::vector<lv_ndt_result> res((size_t)K);
    for (int k = 0; k < K; ++k) {
        lv_graph_pose x;
        for (int a = 0; a < 3; ++a)
            if (scanf("%lf", &x.t[a]) != 1) return 2;
        for (int a = 0; a < 4; ++a)
            if (scanf("%lf", &x.q[a]) != 1) return 2;
        res[(size_t)k] = align_one(q, evaluate, x);
    }
    printf("eval_ms %.4f\n", evals ? eval_ms / (double)evals : 0.0);
    for (const auto& r : res)
        printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %u %d %u %u\n", r.pose.t[0], r.pose.t[1], r.pose.t[2], r.pose.q[0], r.pose.q[1],
               r.pose.q[2], r.pose.q[3], r.score, r.n_in, r.status, r.accepted, r.rejected);
    return 0;
}
