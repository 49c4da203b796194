// scripts/occ_rollout_host.cpp — the host side of scripts/occ_rollout_timing.py: the rule of limo-velo_amd/csrc/lv_rollout.hpp (what
// tests/emu/occ_rollout_emu.cpp runs) built with g++ -O2 through tests/emu/hip/hip_runtime.h, on binary files, timing itself: what
// a caller pays who fetches the plan and the field and rolls the sequences out on one CPU core.
//
//   occ_rollout_host HEAD COST POT S2 JOB...
// HEAD: origin[3] resolution (f32), nx ny (i32): the plan's and the field's.  COST: nx * ny u8.  POT: nx * ny u32.  S2: nx * ny i32.
// JOB: lv_rollout_params (36 bytes), start[3] f32, n_fp K (i32), n_fp x (fx fy) f32, K x Tc x (v w) f32.
// stdout: one JSON list, per job {"ms": median of 3 runs, "steps": the sum of steps, "clear": sequences CLEAR, "best", "best_score"}.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "lv_rollout.hpp"

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
    if (argc < 6) return 2;
    const std::vector<float> head = slurp<float>(argv[1]);
    const std::vector<uint8_t> cost = slurp<uint8_t>(argv[2]);
    const std::vector<uint32_t> pot = slurp<uint32_t>(argv[3]);
    const std::vector<int32_t> s2 = slurp<int32_t>(argv[4]);
    RolloutView f{};
    int32_t dims[2];
    std::memcpy(dims, &head[4], sizeof(dims));
    f.plan.nx = dims[0]; f.plan.ny = dims[1]; f.plan.nz = 1; f.plan.planar = 1; f.plan.max_m = 2;
    for (int a = 0; a < 3; ++a) f.plan.origin[a] = f.f_origin[a] = head[a];
    f.plan.resolution = f.f_resolution = head[3];
    f.field = GridDims{dims[0], dims[1], 1};
    const size_t n = (size_t)dims[0] * (size_t)dims[1];
    if (cost.size() != n || pot.size() != n || s2.size() != n) return 2;
    f.cost = cost.data(); f.pot = pot.data(); f.s2 = s2.data();
    printf("[");
    for (int j = 5; j < argc; ++j) {
        const std::vector<float> job = slurp<float>(argv[j]);
        lv_rollout_params r;
        std::memcpy(&r, job.data(), sizeof(r));
        const float* start = job.data() + sizeof(r) / 4;
        int32_t counts[2];
        std::memcpy(counts, start + 3, sizeof(counts));
        const size_t n_fp = (size_t)counts[0], K = (size_t)counts[1];
        const float* fp = start + 5;
        const float* ctrl = fp + 2 * n_fp;
        if (rollout_check(&r, start, ctrl, K, fp, n_fp, &r, nullptr, nullptr, nullptr) || job.size() != sizeof(r) / 4 + 5 + 2 * n_fp + K * r.Tc * 2) return 2;
        std::vector<lv_rollout_result> res(K);
        double ms[3];
        uint64_t best_s = ROLL_NO_SCORE;
        uint32_t best_i = 0xFFFFFFFFu;
        for (double& m : ms) {
            best_s = ROLL_NO_SCORE;
            best_i = 0xFFFFFFFFu;
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t q = 0; q < K; ++q) {
                rollout_sequence(f, r, (int)n_fp, start, ctrl + q * (size_t)r.Tc * 2, fp, true, RolloutOneLane(), res[q], nullptr);
                const uint64_t s = rollout_score(r, res[q]);
                if (rollout_before(s, (uint32_t)q, best_s, best_i)) {
                    best_s = s;
                    best_i = (uint32_t)q;
                }
            }
            m = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        std::sort(ms, ms + 3);
        long long steps = 0, clear = 0;
        for (const lv_rollout_result& o : res) {
            steps += o.steps;
            clear += o.status == LV_ROLLOUT_CLEAR;
        }
        printf("%s{\"ms\": %.3f, \"steps\": %lld, \"clear\": %lld, \"best\": %lld, \"best_score\": %lld}", j > 5 ? ", " : "", ms[1], steps, clear,
               best_s == ROLL_NO_SCORE ? -1ll : (long long)best_i, (long long)best_s);
    }
    printf("]\n");
    return 0;
}
