// tests/emu/occ_rollout_emu.cpp — the rule of limo-velo_amd/csrc/lv_rollout.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++
// through tests/emu/hip/hip_runtime.h).  Every sequence runs rollout_sequence as the kernel of lv_rollout.hip does, as a group of
// one lane (RolloutOneLane); the score is rollout_score's and `best` the least by rollout_before.  The arrays have exactly the
// sizes the rule may touch: a read or write past them is the sanitizer's to find.
// tests/test_occ_rollout_host.py holds its output to tests/rollout_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   origin[3] resolution nx ny, then nx * ny cost bytes, then nx * ny potentials            (the plan)
//   has_field; with 1: origin[3] resolution nx ny, then nx * ny s2                          (the field)
//   then any number of
//     "J" T Tc dt fp_clear_s2 w_cost w_goal w_stop min_steps goal_mode start[3] n_fp (fx fy) x n_fp K n_floats (v w) x K * Tc
// stdout per job:
//   "check ok" or "check bad: <why>" (and nothing more for the job)
//   per sequence one line: status steps why cell_end p_end p_min s_min cost_sum score, then the (T + 1) * 3 pose floats' bits
//   one line: best[0] best[1]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_rollout.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

static float read_f() {
    unsigned int u = 0;
    if (scanf("%u", &u) != 1) exit(2);
    return __uint_as_float(u);
}
static long long read_i() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) exit(2);
    return v;
}

int main() {
    RolloutView f{};
    f.plan.planar = 1;
    f.plan.max_m = 2;
    f.plan.nz = 1;
    for (float& x : f.plan.origin) x = read_f();
    f.plan.resolution = read_f();
    f.plan.nx = (int)read_i();
    f.plan.ny = (int)read_i();
    const size_t n = (size_t)f.plan.nx * (size_t)f.plan.ny;
    std::vector<uint8_t> cost(n);
    std::vector<uint32_t> pot(n);
    for (uint8_t& c : cost) c = (uint8_t)read_i();
    for (uint32_t& p : pot) p = (uint32_t)read_i();
    f.cost = cost.data();
    f.pot = pot.data();
    std::vector<int32_t> s2;
    if (read_i()) {
        for (float& x : f.f_origin) x = read_f();
        f.f_resolution = read_f();
        f.field.nx = (int)read_i();
        f.field.ny = (int)read_i();
        f.field.nz = 1;
        s2.resize((size_t)f.field.nx * (size_t)f.field.ny);
        for (int32_t& v : s2) v = (int32_t)read_i();
        f.s2 = s2.data();
    }
    char cmd = 0;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd != 'J') return 2;
        lv_rollout_params r{};
        r.T = (int)read_i();
        r.Tc = (int)read_i();
        r.dt = read_f();
        r.fp_clear_s2 = (int)read_i();
        r.w_cost = (uint32_t)read_i();
        r.w_goal = (uint32_t)read_i();
        r.w_stop = (uint32_t)read_i();
        r.min_steps = (int)read_i();
        r.goal_mode = (int)read_i();
        float start[3];
        for (float& x : start) x = read_f();
        const size_t n_fp = (size_t)read_i();
        std::vector<float> fp(2 * n_fp);
        for (float& x : fp) x = read_f();
        const size_t K = (size_t)read_i();
        std::vector<float> ctrl((size_t)read_i());   // (its length is given: a refused job leaves the stream in step)
        for (float& x : ctrl) x = read_f();
        lv_rollout_result dummy;
        if (const char* why = rollout_check(&r, start, ctrl.data(), K, fp.data(), n_fp, &dummy, nullptr, nullptr, nullptr)) {
            printf("check bad: %s\n", why);
            continue;
        }
        if ((n_fp && !f.s2) || ctrl.size() != K * (size_t)r.Tc * 2) return 3;
        printf("check ok\n");
        uint64_t best_s = ROLL_NO_SCORE;
        uint32_t best_i = 0xFFFFFFFFu;
        for (size_t q = 0; q < K; ++q) {
            std::vector<float> rows((size_t)(r.T + 1) * 3, __uint_as_float(ROLL_NAN_BITS));
            lv_rollout_result o;
            rollout_sequence(f, r, (int)n_fp, start, ctrl.data() + q * (size_t)r.Tc * 2, fp.data(), true, RolloutOneLane(), o, rows.data());
            const uint64_t s = rollout_score(r, o);
            if (rollout_before(s, (uint32_t)q, best_s, best_i)) {
                best_s = s;
                best_i = (uint32_t)q;
            }
            printf("%d %d %d %d %u %u %d %u %llu", o.status, o.steps, o.why, o.cell_end, o.p_end, o.p_min, o.s_min, o.cost_sum, (unsigned long long)s);
            for (float b : rows) printf(" %u", __float_as_uint(b));
            printf("\n");
        }
        printf("%lld %lld\n", best_s == ROLL_NO_SCORE ? -1ll : (long long)best_i, (long long)best_s);
    }
    return 0;
}
