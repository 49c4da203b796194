// tests/emu/occ_mcl_emu.cpp — the rule of limo-velo_amd/csrc/lv_mcl.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  Every particle runs mcl_particle as the kernel of lv_mcl.hip does, as a group of one lane
// (MclOneLane); `best` is the least mcl_key, decoded by mcl_best_of.  The arrays have exactly the sizes the rule may touch: a read
// or write past them is the sanitizer's to find.
// tests/test_occ_mcl_host.py holds its output to tests/mcl_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   planar origin[3] resolution nx ny nz, then nx * ny * nz s2                              (the field; nz = 1 when planar)
//   then any number of
//     "J" out_cost min_inside n_table n_entries (entry) x n_entries B n_floats (beam floats) K n_floats (pose floats)
//   (the arrays' lengths are given apart from n_table, B and K: a refused job leaves the stream in step)
// stdout per job:
//   "check ok" or "check bad: <why>" (and nothing more for the job)
//   per particle one line: score n_in
//   one line: best[0] best[1]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_mcl.hpp"

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
    MclView f{};
    f.planar = (int)read_i();
    for (float& x : f.origin) x = read_f();
    f.resolution = read_f();
    f.field.nx = (int)read_i();
    f.field.ny = (int)read_i();
    f.field.nz = (int)read_i();
    std::vector<int32_t> s2(grid_cells(f.field));
    for (int32_t& v : s2) v = (int32_t)read_i();
    f.s2 = s2.data();
    char cmd = 0;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd != 'J') return 2;
        lv_mcl_params r{};
        r.out_cost = (uint32_t)read_i();
        r.min_inside = (int)read_i();
        const size_t n_table = (size_t)read_i();
        std::vector<uint32_t> table((size_t)read_i());
        for (uint32_t& t : table) t = (uint32_t)read_i();
        const size_t B = (size_t)read_i();
        std::vector<float> beams((size_t)read_i());
        for (float& x : beams) x = read_f();
        const size_t K = (size_t)read_i();
        std::vector<float> poses((size_t)read_i());
        for (float& x : poses) x = read_f();
        // (a job past a limit comes without its arrays: the check must refuse it before it looks at them)
        static const float none_f = 0.0f;
        static const uint32_t none_u = 0;
        const bool sized = table.size() == n_table && beams.size() == 3 * B && poses.size() == 4 * K;
        uint64_t dummy;
        if (const char* why = mcl_check(&r, sized ? poses.data() : &none_f, K, sized ? beams.data() : &none_f, B, sized ? table.data() : &none_u,
                                        n_table, &dummy, nullptr, nullptr)) {
            printf("check bad: %s\n", why);
            continue;
        }
        if (!sized) return 3;
        printf("check ok\n");
        uint64_t least = MCL_NO_SCORE;
        for (size_t q = 0; q < K; ++q) {
            uint64_t s;
            uint32_t n;
            mcl_particle(f, r, poses.data() + 4 * q, beams.data(), (int)B, table.data(), (uint32_t)n_table, true, MclOneLane(), s, n);
            const uint64_t k = mcl_key(s, (uint32_t)q);
            if (k < least) least = k;
            printf("%llu %u\n", (unsigned long long)s, n);
        }
        int64_t best[2];
        mcl_best_of(least, best);
        printf("%lld %lld\n", (long long)best[0], (long long)best[1]);
    }
    return 0;
}
