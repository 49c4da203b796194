// tests/emu/mcl_filter_emu.cpp — the rule of limo-velo_amd/csrc/lv_mcl_filter.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++
// through tests/emu/hip/hip_runtime.h).  A particle set in plain vectors goes through the calls of the resident filter with exactly
// the functions the kernels of lv_mcl_filter.hip run: mclf_move per particle, mcl_particle as a group of one lane with
// mclf_accumulate, mclf_weight and mclf_terms per particle with the sums in 64-bit integers, mclf_decide, and mclf_ancestor over
// the two-level prefix sums (blocks of MCLF_BLOCK).  The checks and the states are those of the header.  The arrays have exactly
// the sizes the rule may touch: a read or write past them is the sanitizer's to find.
// tests/test_mcl_filter_host.py holds its output to tests/mcl_filter_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   planar origin[3] resolution nx ny nz, then nx * ny * nz s2                              (the field; nz = 1 when planar)
//   then any number of commands:
//     "S" seed K n_floats (pose floats)                                                      lv_occ_mcl_filter_set
//     "M" delta[3] sigma[3]                                                                  _move
//     "W" out_cost min_inside n_table n_entries (entry)... B n_floats (beam floats)          _weigh
//     "R" shift mode below_num below_den n_w n_entries (entry)...                            _resample
//     "G"                                                                                    _get
//     "E" epoch since                                                                        (sets the store's counters)
//   (the arrays' lengths are given apart from K, n_table, B and n_w: a refused command leaves the stream in step)
// stdout per command: "ok", "check bad: <why>" or "state bad: <why>" (and nothing more when refused), then
//   W: one line best[0] best[1]
//   R: one line W sum_w2 s_min S[0..4] n_eligible n_clamped resampled epoch since; when resampled one line of K ancestors
//   G: per particle one line: the four pose words, acc, n_in
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_mcl_filter.hpp"

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
static unsigned long long read_u() {
    unsigned long long v = 0;
    if (scanf("%llu", &v) != 1) exit(2);
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

    bool set = false;
    uint64_t seed = 0;
    uint32_t epoch = 0, since = 0;
    std::vector<float> poses;
    std::vector<uint64_t> acc;
    std::vector<uint32_t> n_in;
    static const float none_f = 0.0f;
    static const uint32_t none_u = 0;
    const char* no_particles = "no particles: call lv_occ_mcl_filter_set first";

    char cmd = 0;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'S') {
            const uint64_t sd = read_u();
            const size_t K = (size_t)read_i();
            std::vector<float> x((size_t)read_i());
            for (float& v : x) v = read_f();
            const bool sized = x.size() == 4 * K;
            if (const char* why = mclf_check_set(sized ? x.data() : &none_f, K)) {
                printf("check bad: %s\n", why);
                continue;
            }
            if (!sized) return 3;
            poses = x;
            acc.assign(K, 0);
            n_in.assign(K, 0);
            seed = sd;
            epoch = since = 0;
            set = true;
            printf("ok\n");
        } else if (cmd == 'M') {
            float delta[3], sigma[3];
            for (float& v : delta) v = read_f();
            for (float& v : sigma) v = read_f();
            if (const char* why = mclf_check_move(delta, sigma)) {
                printf("check bad: %s\n", why);
                continue;
            }
            const char* why = !set ? no_particles : mclf_state_epoch(epoch);
            if (why) {
                printf("state bad: %s\n", why);
                continue;
            }
            const uint64_t base = mclf_base(seed, epoch);
            for (size_t i = 0; i < acc.size(); ++i) mclf_move(poses.data() + 4 * i, base, (uint32_t)i, delta, sigma);
            ++epoch;
            printf("ok\n");
        } else if (cmd == 'W') {
            lv_mcl_params r{};
            r.out_cost = (uint32_t)read_i();
            r.min_inside = (int)read_i();
            const size_t n_table = (size_t)read_i();
            std::vector<uint32_t> table((size_t)read_i());
            for (uint32_t& t : table) t = (uint32_t)read_i();
            const size_t B = (size_t)read_i();
            std::vector<float> beams((size_t)read_i());
            for (float& x : beams) x = read_f();
            const bool sized = table.size() == n_table && beams.size() == 3 * B;
            if (const char* why = mclf_check_weigh(&r, sized ? beams.data() : &none_f, B, sized ? table.data() : &none_u, n_table)) {
                printf("check bad: %s\n", why);
                continue;
            }
            if (!set) {
                printf("state bad: %s\n", no_particles);
                continue;
            }
            if (const char* why = mclf_check_pairs(acc.size(), B)) {
                printf("check bad: %s\n", why);
                continue;
            }
            if (const char* why = mclf_state_since(since)) {
                printf("state bad: %s\n", why);
                continue;
            }
            if (!sized) return 3;
            uint64_t least = MCL_NO_SCORE;
            for (size_t q = 0; q < acc.size(); ++q) {
                uint64_t s;
                uint32_t n;
                mcl_particle(f, r, poses.data() + 4 * q, beams.data(), (int)B, table.data(), (uint32_t)n_table, true, MclOneLane(), s, n);
                n_in[q] = n;
                acc[q] = mclf_accumulate(acc[q], s);
                const uint64_t k = mcl_key(s, (uint32_t)q);
                if (k < least) least = k;
            }
            ++since;
            int64_t best[2];
            mcl_best_of(least, best);
            printf("ok\n%lld %lld\n", (long long)best[0], (long long)best[1]);
        } else if (cmd == 'R') {
            lv_mcl_resample_params p{};
            p.shift = (int)read_i();
            p.mode = (int)read_i();
            p.below_num = (uint32_t)read_i();
            p.below_den = (uint32_t)read_i();
            const size_t n_w = (size_t)read_i();
            std::vector<uint32_t> wtable((size_t)read_i());
            for (uint32_t& t : wtable) t = (uint32_t)read_i();
            const bool sized = wtable.size() == n_w;
            lv_mcl_filter_stats st{};
            if (const char* why = mclf_check_resample(&p, sized ? wtable.data() : &none_u, n_w, &st)) {
                printf("check bad: %s\n", why);
                continue;
            }
            const char* why = !set ? no_particles : mclf_state_epoch(epoch);
            if (why) {
                printf("state bad: %s\n", why);
                continue;
            }
            if (!sized) return 3;
            const size_t K = acc.size(), nb = (K + MCLF_BLOCK - 1) / MCLF_BLOCK;
            uint64_t s_min = MCL_NO_SCORE;
            for (uint64_t a : acc)
                if (a < s_min) s_min = a;
            std::vector<uint32_t> cin(K);
            std::vector<unsigned long long> cb(nb);
            uint64_t W = 0, sum_w2 = 0;
            int64_t S[5] = {0, 0, 0, 0, 0};
            uint32_t n_eligible = 0, n_clamped = 0;
            for (size_t i = 0; i < K; ++i) {
                const uint32_t w = mclf_weight(acc[i], s_min, p.shift, wtable.data(), (uint32_t)n_w);
                int64_t q[5];
                n_clamped += mclf_terms(f.origin, f.resolution, poses.data() + 4 * i, q) ? 1u : 0u;
                n_eligible += acc[i] != MCL_NO_SCORE ? 1u : 0u;
                W += w;
                sum_w2 += (uint64_t)w * w;
                for (int a = 0; a < 5; ++a) S[a] += (int64_t)w * q[a];
                cin[i] = (i % MCLF_BLOCK ? cin[i - 1] : 0u) + w;
                cb[i / MCLF_BLOCK] = W;
            }
            const bool go = mclf_decide(p.mode, W, sum_w2, (uint64_t)K, p.below_num, p.below_den);
            std::vector<uint32_t> anc;
            if (go) {
                const uint64_t r = mclf_draw(mclf_base(seed, epoch)) % W;
                std::vector<float> next(4 * K);
                anc.resize(K);
                for (size_t j = 0; j < K; ++j) {
                    anc[j] = mclf_ancestor(cb.data(), (uint32_t)nb, cin.data(), (uint32_t)K, mclf_target(j, W, r, K));
                    for (int a = 0; a < 4; ++a) next[4 * j + a] = poses[4 * (size_t)anc[j] + a];
                }
                poses = next;
                acc.assign(K, 0);
                since = 0;
            }
            ++epoch;
            printf("ok\n%llu %llu %lld", (unsigned long long)W, (unsigned long long)sum_w2, n_eligible ? (long long)s_min : -1ll);
            for (int a = 0; a < 5; ++a) printf(" %lld", (long long)S[a]);
            printf(" %u %u %d %u %u\n", n_eligible, n_clamped, go ? 1 : 0, epoch, since);
            if (go) {
                for (size_t j = 0; j < K; ++j) printf("%u%c", anc[j], j + 1 < K ? ' ' : '\n');
            }
        } else if (cmd == 'G') {
            if (!set) {
                printf("state bad: %s\n", no_particles);
                continue;
            }
            printf("ok\n");
            for (size_t i = 0; i < acc.size(); ++i)
                printf("%u %u %u %u %llu %u\n", __float_as_uint(poses[4 * i]), __float_as_uint(poses[4 * i + 1]), __float_as_uint(poses[4 * i + 2]),
                       __float_as_uint(poses[4 * i + 3]), (unsigned long long)acc[i], n_in[i]);
        } else if (cmd == 'E') {
            epoch = (uint32_t)read_i();
            since = (uint32_t)read_i();
            printf("ok\n");
        } else {
            return 2;
        }
    }
    return 0;
}
