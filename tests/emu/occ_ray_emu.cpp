// tests/emu/occ_ray_emu.cpp — the rule of limo-velo_amd/csrc/lv_ray.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The states are packed as ray_classify_kernel packs them and read through RayStates, the rays run
// ray_cast / ray_walk as the kernels of lv_ray.hip do, with a plain byte set in place of the seen bitmap.
// tests/test_occ_ray_host.py holds its output to tests/occ_ray_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   origin[3] resolution nx ny nz min_range max_range l_hit l_miss l_min l_max l_occ l_free
//   nx * ny * nz log-odds
//   then any number of
//     "R" stop_unknown n, then n x (from[3] to[3])
//     "G" n_views, then per view: R[9] t[3] n, then n x (x y z)
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   per "R": n lines "status cell steps axis n_free n_unknown num den"
//   per "G": per view one line "used stopped unknown free"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_ray.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

static float read_f() {
    unsigned int u = 0;
    if (scanf("%u", &u) != 1) exit(2);
    return __uint_as_float(u);
}
static long read_i() {
    long v = 0;
    if (scanf("%ld", &v) != 1) exit(2);
    return v;
}

struct SeenSet {
    const OccGrid& g;
    std::vector<unsigned char>& set;
    void operator()(int i, int j, int k) { set[grid_at(g, i, j, k)] = 1; }
};

int main() {
    lv_occupancy_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = read_f();
    p.resolution = read_f();
    p.nx = (int)read_i(); p.ny = (int)read_i(); p.nz = (int)read_i();
    p.min_range = read_f(); p.max_range = read_f();
    p.l_hit = read_f(); p.l_miss = read_f(); p.l_min = read_f(); p.l_max = read_f();
    p.l_occ = read_f(); p.l_free = read_f();
    if (const char* why = occ_check_params(&p)) {
        printf("params bad: %s\n", why);
        return 0;
    }
    printf("params ok\n");
    const OccGrid g = occ_grid_of(p);
    const size_t nv = grid_cells(g);
    std::vector<float> L(nv);
    for (float& x : L) x = read_f();
    // exactly as many words as RayStore::classify allocates: a read past them is the sanitizer's to find
    std::vector<uint32_t> words((size_t)ray_wx16(g.nx) * g.ny * g.nz, 0u);
    for (int k = 0; k < g.nz; ++k)
        for (int j = 0; j < g.ny; ++j)
            for (int i = 0; i < g.nx; ++i) words[ray_word_of(g, i, j, k)] |= ray_pack(fr_state_voxel(L[grid_at(g, i, j, k)], p.l_free, p.l_occ), i);
    char cmd = 0;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'R') {
            const bool stop_unknown = read_i() != 0;
            const long n = read_i();
            for (long i = 0; i < n; ++i) {
                float from[3], to[3];
                for (float& x : from) x = read_f();
                for (float& x : to) x = read_f();
                RayStates st(words.data());
                lv_ray_result r;
                ray_cast(g, from, to, stop_unknown, st, r);
                printf("%d %d %d %d %d %d %d %d\n", r.status, r.cell, r.steps, r.axis, r.n_free, r.n_unknown, r.num, r.den);
            }
        } else if (cmd == 'G') {
            const long n_views = read_i();
            for (long v = 0; v < n_views; ++v) {
                float R[9], t[3];
                for (float& x : R) x = read_f();
                for (float& x : t) x = read_f();
                const long n = read_i();
                std::vector<float> pts((size_t)n * 3);
                for (float& x : pts) x = read_f();
                std::vector<unsigned char> set(nv, 0);
                SeenSet seen{g, set};
                long used = 0, stopped = 0, nu = 0, nf = 0;
                int32_t qs[3];
                if (n && occ_view_origin(g, t, qs)) {
                    for (long i = 0; i < n; ++i) {
                        int32_t qe[3] = {0, 0, 0};
                        if (occ_return(g, R, t, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], qe) == OCC_RAY_IGNORED) continue;
                        ++used;
                        RayStates st(words.data());
                        lv_ray_result r;
                        ray_walk(g, qs, qe, false, st, seen, r);
                        stopped += r.status == LV_RAY_STOPPED;
                    }
                }
                for (size_t c = 0; c < nv; ++c) {
                    if (!set[c]) continue;
                    const int s = fr_state_voxel(L[c], p.l_free, p.l_occ);
                    nu += s == FR_UNKNOWN;
                    nf += s == FR_FREE;
                }
                printf("%ld %ld %ld %ld\n", used, stopped, nu, nf);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
