// scripts/occ_ray_host.cpp — the host side of scripts/occ_ray_timing.py: the rule of limo-velo_amd/csrc/lv_ray.hpp (what
// tests/emu/occ_ray_emu.cpp runs) built with g++ -O2 through tests/emu/hip/hip_runtime.h, on binary files, timing itself: what
// a caller pays who fetches the grid and casts the rays on one CPU core.
//
//   occ_ray_host PARAMS GRID RAYS VIEWS
// PARAMS: origin[3] resolution min_range max_range l_occ l_free (f32), then nx ny nz (i32).  GRID: nx * ny * nz f32.
// RAYS: n x (from[3] to[3]) f32.  VIEWS: i32 n_views, i32 n; then per view R[9] t[3] f32; then n x 3 f32 returns shared by all views.
// stdout: one JSON object: pack_ms, raycast_ms, stopped, gain_ms, gain_unknown (summed over the views).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <vector>

#include "lv_ray.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

template <class T>
static std::vector<T> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct SeenSet {
    const OccGrid& g;
    std::vector<unsigned char>& set;
    void operator()(int i, int j, int k) { set[grid_at(g, i, j, k)] = 1; }
};

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const std::vector<float> pf = slurp<float>(argv[1]);
    lv_occupancy_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = pf[a];
    p.resolution = pf[3]; p.min_range = pf[4]; p.max_range = pf[5]; p.l_occ = pf[6]; p.l_free = pf[7];
    p.l_hit = 0.85f; p.l_miss = -0.4f; p.l_min = -2.0f; p.l_max = 3.5f;   // (not read by the rays)
    int32_t dims[3];
    std::memcpy(dims, &pf[8], sizeof(dims));
    p.nx = dims[0]; p.ny = dims[1]; p.nz = dims[2];
    if (const char* why = occ_check_params(&p)) { fprintf(stderr, "%s\n", why); return 2; }
    const OccGrid g = occ_grid_of(p);
    const std::vector<float> L = slurp<float>(argv[2]);
    if (L.size() != grid_cells(g)) return 2;

    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> words((size_t)ray_wx16(g.nx) * g.ny * g.nz, 0u);
    for (int k = 0; k < g.nz; ++k)
        for (int j = 0; j < g.ny; ++j)
            for (int i = 0; i < g.nx; ++i) words[ray_word_of(g, i, j, k)] |= ray_pack(fr_state_voxel(L[grid_at(g, i, j, k)], p.l_free, p.l_occ), i);
    const double pack_ms = ms_since(t0);

    const std::vector<float> rays = slurp<float>(argv[3]);
    const size_t n = rays.size() / 6;
    std::vector<lv_ray_result> res(n);
    t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n; ++i) {
        RayStates st(words.data());
        ray_cast(g, &rays[6 * i], &rays[6 * i + 3], false, st, res[i]);
    }
    const double raycast_ms = ms_since(t0);
    long stopped = 0;
    for (const lv_ray_result& r : res) stopped += r.status == LV_RAY_STOPPED;

    const std::vector<float> vf = slurp<float>(argv[4]);
    int32_t head[2];
    std::memcpy(head, vf.data(), sizeof(head));
    const float* poses = vf.data() + 2;
    const float* pts = poses + 12 * (size_t)head[0];
    std::vector<unsigned char> set(L.size(), 0);
    SeenSet seen{g, set};
    long unknown = 0;
    t0 = std::chrono::steady_clock::now();
    for (int v = 0; v < head[0]; ++v) {
        const float* R = poses + 12 * (size_t)v;
        const float* t = R + 9;
        int32_t qs[3];
        if (!occ_view_origin(g, t, qs)) continue;
        for (int i = 0; i < head[1]; ++i) {
            int32_t qe[3];
            if (occ_return(g, R, t, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], qe) == OCC_RAY_IGNORED) continue;
            RayStates st(words.data());
            lv_ray_result r;
            ray_walk(g, qs, qe, false, st, seen, r);
        }
        for (size_t c = 0; c < set.size(); ++c) {
            if (!set[c]) continue;
            unknown += fr_state_voxel(L[c], p.l_free, p.l_occ) == FR_UNKNOWN;
            set[c] = 0;
        }
    }
    const double gain_ms = ms_since(t0);
    printf("{\"pack_ms\": %.3f, \"raycast_ms\": %.3f, \"stopped\": %ld, \"gain_ms\": %.3f, \"gain_unknown\": %ld}\n", pack_ms, raycast_ms, stopped, gain_ms,
           unknown);
    return 0;
}
