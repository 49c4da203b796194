// scripts/surf_align_host.cpp — the rule of limo-velo_amd/csrc/lv_surf_align.hpp on one CPU core (g++ -O2 -ffp-contract=off through
// tests/emu/hip/hip_runtime.h): what scripts/surf_align_timing.py times the device against and checks it with.
//
//   surf_align_host <params> <S.i32> <W.i32> <source.f32> min_weight max_dist huber K  < K poses
// params: origin[3], resolution as f32, then nx, ny, nz as int32 (what lv_tsdf_get_params reports); S, W: what lv_tsdf_fetch
// gave; source: packed x, y, z as f32.  One evaluation at every pose, the points in ascending order.
// stdout: "eval_ms <ms per evaluation of one hypothesis>", then per pose "n_in cost".
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <vector>

#include "lv_surf_align.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace lv {
void set_error(const char*, ...) {}
}  // namespace lv

using namespace lv;
using Clock = std::chrono::steady_clock;

template <class T>
static std::vector<T> read_all(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const std::vector<uint8_t> raw = read_all<uint8_t>(argv[1]);
    if (raw.size() != 28) return 2;
    TsdfGrid g{};
    std::memcpy(g.occ.origin, raw.data(), 12);
    std::memcpy(&g.occ.resolution, raw.data() + 12, 4);
    int32_t dims[3];
    std::memcpy(dims, raw.data() + 16, 12);
    g.occ.nx = dims[0];
    g.occ.ny = dims[1];
    g.occ.nz = dims[2];
    const std::vector<int32_t> S = read_all<int32_t>(argv[2]), W = read_all<int32_t>(argv[3]);
    const std::vector<float> src = read_all<float>(argv[4]);
    if (S.size() != grid_cells(g.occ) || W.size() != S.size()) return 2;
    const int min_weight = atoi(argv[5]);
    const double max_dist = atof(argv[6]), huber = atof(argv[7]);
    const int K = atoi(argv[8]);
    const uint32_t n_src = (uint32_t)(src.size() / 3);
    // the loop with no iteration and no least n_in: the guess is scored whatever it holds
    lv_surf_align_params prm;
    default_surf_align_params(&prm);
    prm.max_iterations = 0;
    prm.min_points = 0;
    prm.max_dist = max_dist;
    prm.huber = huber;
    const SurfAlignRule q = surf_align_rule_of(prm, surf_view_of(g, min_weight, S.data(), W.data()), n_src);
    double eval_ms = 0.0;
    const auto evaluate = [&](const lv_graph_pose& x, double* tot) {
        const auto t0 = Clock::now();
        const uint32_t n_in = align_evaluate(q, src.data(), n_src, x, tot);
        eval_ms += std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        return n_in;
    };
    std::vector<lv_surf_align_result> res((size_t)K);
    for (int k = 0; k < K; ++k) {
        lv_graph_pose x;
        for (int a = 0; a < 3; ++a)
            if (scanf("%lf", &x.t[a]) != 1) return 2;
        for (int a = 0; a < 4; ++a)
            if (scanf("%lf", &x.q[a]) != 1) return 2;
        res[(size_t)k] = align_one(q, evaluate, x);
    }
    printf("eval_ms %.4f\n", K ? eval_ms / (double)K : 0.0);
    for (const auto& r : res) printf("%u %.17g\n", r.n_in, r.cost);
    return 0;
}
