// scripts/tsdf_ray_host.cpp — the host side of scripts/tsdf_ray_timing.py: the rule of limo-velo_amd/csrc/lv_tsdf_ray.hpp (what
// tests/emu/tsdf_ray_emu.cpp runs) built with g++ -O2 through tests/emu/hip/hip_runtime.h, on binary files, timing itself: what
// a caller pays who fetches the volume and casts the rays on one CPU core.
//
//   tsdf_ray_host PARAMS S W RAYS OUT
// PARAMS: origin[3] resolution min_range max_range (f32), then nx ny nz trunc_cells max_weight carve min_weight (i32).
// S, W: nx * ny * nz i32 each.  RAYS: n x (from[3] to[3]) f32.  OUT (written): n records of 8 i32, then n x 3 f32 normals.
// stdout: one JSON object: pack_ms, raycast_ms (records only), raycast_normals_ms, hit, blocked.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lv_tsdf_ray.hpp"

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

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const std::vector<float> pf = slurp<float>(argv[1]);
    lv_tsdf_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = pf[a];
    p.resolution = pf[3]; p.min_range = pf[4]; p.max_range = pf[5];
    int32_t ints[7];
    std::memcpy(ints, &pf[6], sizeof(ints));
    p.nx = ints[0]; p.ny = ints[1]; p.nz = ints[2]; p.trunc_cells = ints[3]; p.max_weight = ints[4]; p.carve = ints[5];
    const int32_t min_weight = ints[6];
    if (const char* why = tsdf_check_params(&p)) { fprintf(stderr, "%s\n", why); return 2; }
    const OccGrid g = tsdf_grid_of(p).occ;
    const std::vector<int32_t> S = slurp<int32_t>(argv[2]), W = slurp<int32_t>(argv[3]);
    if (S.size() != grid_cells(g) || W.size() != S.size() || min_weight < 1) return 2;

    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> words((size_t)ray_wx16(g.nx) * g.ny * g.nz, 0u);
    for (int k = 0; k < g.nz; ++k)
        for (int j = 0; j < g.ny; ++j)
            for (int i = 0; i < g.nx; ++i) {
                const size_t at = grid_at(g, i, j, k);
                words[ray_word_of(g, i, j, k)] |= ray_pack(surf_state_voxel(S[at], W[at], min_weight), i);
            }
    const double pack_ms = ms_since(t0);

    const std::vector<float> rays = slurp<float>(argv[4]);
    const size_t n = rays.size() / 6;
    std::vector<lv_tsdf_ray_result> res(n);
    std::vector<float> nrm(3 * n);
    double ms[2];
    for (int pass = 0; pass < 2; ++pass) {   // records only, then with the normals
        t0 = std::chrono::steady_clock::now();
        for (size_t i = 0; i < n; ++i) {
            RayStates st(words.data());
            uint32_t rgba;
            surf_cast(g, &rays[6 * i], &rays[6 * i + 3], min_weight, st, S.data(), W.data(), nullptr, pass == 1, false, res[i], &nrm[3 * i], rgba);
        }
        ms[pass] = ms_since(t0);
    }
    long hit = 0, blocked = 0;
    for (const lv_tsdf_ray_result& r : res) {
        hit += r.status == LV_SURF_HIT;
        blocked += r.status == LV_SURF_BLOCKED;
    }
    FILE* f = fopen(argv[5], "wb");
    if (!f || fwrite(res.data(), sizeof(lv_tsdf_ray_result), n, f) != n || fwrite(nrm.data(), sizeof(float), 3 * n, f) != 3 * n) return 2;
    fclose(f);
    printf("{\"pack_ms\": %.3f, \"raycast_ms\": %.3f, \"raycast_normals_ms\": %.3f, \"hit\": %ld, \"blocked\": %ld}\n", pack_ms, ms[0], ms[1], hit, blocked);
    return 0;
}
