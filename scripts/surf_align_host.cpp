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
    const SurfView v = surf_view_of(g, min_weight, S.data(), W.data());
    const uint32_t n_src = (uint32_t)(src.size() / 3);
    double eval_ms = 0.0;
    std::vector<double> cost((size_t)K);
    std::vector<uint32_t> n_in((size_t)K, 0);
    for (int k = 0; k < K; ++k) {
        lv_graph_pose x;
        for (int a = 0; a < 3; ++a)
            if (scanf("%lf", &x.t[a]) != 1) return 2;
        for (int a = 0; a < 4; ++a)
            if (scanf("%lf", &x.q[a]) != 1) return 2;
        double acc[SURF_ACC], R[9];
        for (int a = 0; a < SURF_ACC; ++a) acc[a] = 0.0;
        gr_rot(x.q, R);
        const auto t0 = Clock::now();
        for (uint32_t i = 0; i < n_src; ++i) n_in[(size_t)k] += surf_point_terms(v, R, x.t, &src[3 * (size_t)i], max_dist, huber, acc) ? 1u : 0u;
        eval_ms += std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
        cost[(size_t)k] = surf_cost(acc[27], n_src, n_in[(size_t)k], max_dist, huber);
    }
    printf("eval_ms %.4f\n", K ? eval_ms / (double)K : 0.0);
    for (int k = 0; k < K; ++k) printf("%u %.17g\n", n_in[(size_t)k], cost[(size_t)k]);
    return 0;
}
