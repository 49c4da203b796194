// tests/emu/occupancy_emu.cpp — the rule of limo-velo_amd/csrc/lv_occupancy.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The loop below is the loop of occ_march_kernel with plain byte sets in place of the bitmaps, then
// the fold.  tests/test_occupancy_host.py holds its output to tests/occupancy_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   origin[3] resolution nx ny nz min_range max_range l_hit l_miss l_min l_max l_occ l_free
//   n_views, then per view: R[9] t[3] n, then n x (x y z)
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   per view: "view <used> <cut> <n_free> <n_hit>", the free voxels' linear indices on one line, the hit voxels' on the next
//   "grid", then the bits of every voxel's log-odds
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_occupancy.hpp"

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
    const size_t nv = (size_t)p.nx * p.ny * p.nz;
    std::vector<float> L(nv, __uint_as_float(0x7FC00000u));
    std::vector<unsigned char> crossed(nv), hit(nv);
    auto at = [&](const OccWalk& w) { return ((size_t)w.vz * g.ny + w.vy) * g.nx + w.vx; };
    const long n_views = read_i();
    for (long v = 0; v < n_views; ++v) {
        float R[9], t[3];
        for (float& x : R) x = read_f();
        for (float& x : t) x = read_f();
        const long n = read_i();
        std::vector<float> pts((size_t)n * 3);
        for (float& x : pts) x = read_f();
        std::fill(crossed.begin(), crossed.end(), 0);
        std::fill(hit.begin(), hit.end(), 0);
        long used = 0, cut = 0;
        int32_t qs[3];
        if (n && occ_view_origin(g, t, qs)) {
            for (long i = 0; i < n; ++i) {
                int32_t qe[3] = {0, 0, 0};
                const int kind = occ_return(g, R, t, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], qe);
                if (kind == OCC_RAY_IGNORED) continue;
                ++used;
                cut += kind == OCC_RAY_CUT;
                OccWalk w;
                occ_walk_init(w, qs, qe);
                bool left = false;
                while (!occ_walk_done(w)) {
                    if (occ_in_grid(g, w.vx, w.vy, w.vz)) crossed[at(w)] = 1;
                    else if (occ_walk_left(g, w)) { left = true; break; }
                    occ_walk_step(w);
                }
                if (!left && occ_in_grid(g, w.vx, w.vy, w.vz)) (kind == OCC_RAY_HIT ? hit : crossed)[at(w)] = 1;
                if (!left && (w.vx != w.ex || w.vy != w.ey || w.vz != w.ez)) { printf("walk did not end in ve\n"); return 3; }
            }
        }
        long nf = 0, nh = 0;
        for (size_t i = 0; i < nv; ++i) {
            if (hit[i]) crossed[i] = 0;
            nf += crossed[i];
            nh += hit[i];
        }
        printf("view %ld %ld %ld %ld\n", used, cut, nf, nh);
        for (size_t i = 0; i < nv; ++i) if (crossed[i]) printf("%zu ", i);
        printf("\n");
        for (size_t i = 0; i < nv; ++i) if (hit[i]) printf("%zu ", i);
        printf("\n");
        for (size_t i = 0; i < nv; ++i)
            if (hit[i] || crossed[i]) L[i] = occ_update(L[i], hit[i] ? g.l_hit : g.l_miss, g.l_min, g.l_max);
    }
    printf("grid\n");
    for (size_t i = 0; i < nv; ++i) printf("%u ", __float_as_uint(L[i]));
    printf("\n");
    return 0;
}
