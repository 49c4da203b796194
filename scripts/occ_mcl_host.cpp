// scripts/occ_mcl_host.cpp — the host side of scripts/occ_mcl_timing.py: the rule of limo-velo_amd/csrc/lv_mcl.hpp (what
// tests/emu/occ_mcl_emu.cpp runs) built with g++ -O2 through tests/emu/hip/hip_runtime.h, on binary files, timing itself: what a
// caller pays who fetches the field and weighs the particles on one CPU core.
//
//   occ_mcl_host HEAD S2 TABLE JOB...
// HEAD: origin[3] resolution (f32), nx ny nz planar (i32).  S2: nx * ny * nz i32.  TABLE: n_table u32.
// JOB: out_cost (u32), min_inside, B, K, runs (i32), B x (ex ey ez) f32, K x (x y z th) f32.
// stdout: one JSON list, per job {"ms": median of the runs, "sum": the sum of the eligible scores, "eligible", "best", "best_score"}.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "lv_mcl.hpp"

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

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::vector<float> head = slurp<float>(argv[1]);
    const std::vector<int32_t> s2 = slurp<int32_t>(argv[2]);
    const std::vector<uint32_t> table = slurp<uint32_t>(argv[3]);
    if (head.size() != 8) return 2;
    int32_t dims[4];
    std::memcpy(dims, &head[4], sizeof(dims));
    MclView f{};
    for (int a = 0; a < 3; ++a) f.origin[a] = head[a];
    f.resolution = head[3];
    f.field = GridDims{dims[0], dims[1], dims[2]};
    f.planar = dims[3];
    if (s2.size() != grid_cells(f.field)) return 2;
    f.s2 = s2.data();
    printf("[");
    for (int j = 4; j < argc; ++j) {
        const std::vector<float> job = slurp<float>(argv[j]);
        int32_t h[5];
        std::memcpy(h, job.data(), sizeof(h));
        lv_mcl_params r{};
        r.out_cost = (uint32_t)h[0];
        r.min_inside = h[1];
        const size_t B = (size_t)h[2], K = (size_t)h[3];
        const int runs = h[4];
        const float* beams = job.data() + 5;
        const float* poses = beams + 3 * B;
        uint64_t dummy;
        if (runs < 1 || job.size() != 5 + 3 * B + 4 * K || mcl_check(&r, poses, K, beams, B, table.data(), table.size(), &dummy, nullptr, nullptr)) return 2;
        std::vector<uint64_t> score(K);
        std::vector<double> ms((size_t)runs);
        uint64_t least = MCL_NO_SCORE;
        for (double& m : ms) {
            least = MCL_NO_SCORE;
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t q = 0; q < K; ++q) {
                uint32_t n;
                mcl_particle(f, r, poses + 4 * q, beams, (int)B, table.data(), (uint32_t)table.size(), true, MclOneLane(), score[q], n);
                const uint64_t k = mcl_key(score[q], (uint32_t)q);
                if (k < least) least = k;
            }
            m = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        std::sort(ms.begin(), ms.end());
        unsigned long long sum = 0, eligible = 0;
        for (uint64_t s : score)
            if (s != MCL_NO_SCORE) {
                sum += s;
                ++eligible;
            }
        int64_t best[2];
        mcl_best_of(least, best);
        printf("%s{\"ms\": %.3f, \"sum\": %llu, \"eligible\": %llu, \"best\": %lld, \"best_score\": %lld}", j > 4 ? ", " : "", ms[ms.size() / 2], sum,
               eligible, (long long)best[0], (long long)best[1]);
    }
    printf("]\n");
    return 0;
}
