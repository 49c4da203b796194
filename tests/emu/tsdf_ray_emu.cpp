// tests/emu/tsdf_ray_emu.cpp — the rule of limo-velo_amd/csrc/lv_tsdf_ray.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The states are packed as surf_pack_kernel packs them and read through RayStates, the rays run
// surf_cast / surf_cast_q as the kernels of lv_tsdf_ray.hip do.  Every ray is also walked with the states taken from S and W
// directly; the two routes must agree on every bit (exit 3 otherwise).  tests/test_tsdf_ray_host.py holds the output to
// tests/tsdf_ray_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   origin[3] resolution nx ny nz min_range max_range trunc_cells max_weight carve
//   nx * ny * nz S, then nx * ny * nz W
//   has_layer, then 4 * nx * ny * nz sums when has_layer != 0
//   then any number of
//     "R" min_weight n, then n x (from[3] to[3])
//     "V" min_weight n_views, then per view: R[9] t[3] n, then n x (x y z)
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   per ray or return one line "status cell steps axis depth t n_known n_unknown nx ny nz rgba" (the normal as the bits of its
//   floats, the colour as r | g << 8 | b << 16 | a << 24); per "V" after its returns one line "used hit blocked clear"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "lv_tsdf_ray.hpp"

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

// the states of the walk from S and W, without the packed copy
struct DirectStates {
    const int32_t* S;
    const int32_t* W;
    int32_t min_weight;
    int state(const OccGrid& g, int i, int j, int k) const {
        const size_t at = grid_at(g, i, j, k);
        return surf_state_voxel(S[at], W[at], min_weight);
    }
};

struct Out {
    lv_tsdf_ray_result r;
    float n[3];
    uint32_t rgba;
};

static void print(const Out& o) {
    printf("%d %d %d %d %d %d %d %d %u %u %u %u\n", o.r.status, o.r.cell, o.r.steps, o.r.axis, o.r.depth, o.r.t, o.r.n_known, o.r.n_unknown,
           __float_as_uint(o.n[0]), __float_as_uint(o.n[1]), __float_as_uint(o.n[2]), o.rgba);
}

static void same_or_die(const Out& a, const Out& b) {
    if (std::memcmp(&a.r, &b.r, sizeof(a.r)) || std::memcmp(a.n, b.n, sizeof(a.n)) || a.rgba != b.rgba) exit(3);
}

int main() {
    lv_tsdf_params p{};
    for (int a = 0; a < 3; ++a) p.origin[a] = read_f();
    p.resolution = read_f();
    p.nx = (int)read_i(); p.ny = (int)read_i(); p.nz = (int)read_i();
    p.min_range = read_f(); p.max_range = read_f();
    p.trunc_cells = (int)read_i(); p.max_weight = (int)read_i(); p.carve = (int)read_i();
    if (const char* why = tsdf_check_params(&p)) {
        printf("params bad: %s\n", why);
        return 0;
    }
    printf("params ok\n");
    const TsdfGrid tg = tsdf_grid_of(p);
    const OccGrid& g = tg.occ;
    const size_t nv = grid_cells(g);
    std::vector<int32_t> S(nv), W(nv);
    for (int32_t& x : S) x = (int32_t)read_i();
    for (int32_t& x : W) x = (int32_t)read_i();
    if (tsdf_check_volume(tg, S.data(), W.data(), nv) != nv) return 2;
    std::vector<uint32_t> layer;
    if (read_i() != 0) {
        layer.resize(4 * nv);
        for (uint32_t& x : layer) x = (uint32_t)read_i();
    }
    const uint32_t* sums = layer.empty() ? nullptr : layer.data();
    // exactly as many words as TsdfStore::rays_pack allocates: a read past them is the sanitizer's to find
    std::vector<uint32_t> words((size_t)ray_wx16(g.nx) * g.ny * g.nz);
    int packed_with = 0;
    auto pack = [&](int min_weight) {
        if (packed_with == min_weight) return;
        std::fill(words.begin(), words.end(), 0u);
        for (int k = 0; k < g.nz; ++k)
            for (int j = 0; j < g.ny; ++j)
                for (int i = 0; i < g.nx; ++i) {
                    const size_t at = grid_at(g, i, j, k);
                    words[ray_word_of(g, i, j, k)] |= ray_pack(surf_state_voxel(S[at], W[at], min_weight), i);
                }
        packed_with = min_weight;
    };
    char cmd = 0;
    while (scanf(" %c", &cmd) == 1) {
        const int min_weight = (int)read_i();
        lv_tsdf_ray_params rp{min_weight, 0};
        if (surf_check_params(&rp)) return 2;
        pack(min_weight);
        DirectStates direct{S.data(), W.data(), min_weight};
        if (cmd == 'R') {
            const long n = read_i();
            for (long i = 0; i < n; ++i) {
                float from[3], to[3];
                for (float& x : from) x = read_f();
                for (float& x : to) x = read_f();
                RayStates st(words.data());
                Out a, b;
                surf_cast(g, from, to, min_weight, st, S.data(), W.data(), sums, true, true, a.r, a.n, a.rgba);
                surf_cast(g, from, to, min_weight, direct, S.data(), W.data(), sums, true, true, b.r, b.n, b.rgba);
                same_or_die(a, b);
                print(a);
            }
        } else if (cmd == 'V') {
            const long n_views = read_i();
            long stats[4] = {0, 0, 0, 0};
            for (long v = 0; v < n_views; ++v) {
                float R[9], t[3];
                for (float& x : R) x = read_f();
                for (float& x : t) x = read_f();
                const long n = read_i();
                int32_t qs[3] = {0, 0, 0};
                const bool valid = occ_view_origin(g, t, qs);
                for (long i = 0; i < n; ++i) {
                    const float x = read_f(), y = read_f(), z = read_f();
                    Out a{}, b{};
                    surf_ignored(a.r);
                    int32_t qe[3] = {0, 0, 0};
                    if (valid && occ_return(g, R, t, x, y, z, qe) != OCC_RAY_IGNORED) {
                        RayStates st(words.data());
                        surf_cast_q(g, qs, qe, min_weight, st, S.data(), W.data(), sums, true, true, a.r, a.n, a.rgba);
                        surf_cast_q(g, qs, qe, min_weight, direct, S.data(), W.data(), sums, true, true, b.r, b.n, b.rgba);
                        same_or_die(a, b);
                        ++stats[0];
                        stats[1] += a.r.status == LV_SURF_HIT;
                        stats[2] += a.r.status == LV_SURF_BLOCKED;
                        stats[3] += a.r.status == LV_SURF_CLEAR;
                    }
                    print(a);
                }
            }
            printf("%ld %ld %ld %ld\n", stats[0], stats[1], stats[2], stats[3]);
        } else {
            return 2;
        }
    }
    return 0;
}
