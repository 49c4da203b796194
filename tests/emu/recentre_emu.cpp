// tests/emu/recentre_emu.cpp — the rolling-volume part of limo-velo_amd/csrc/lv_grid.hpp run on the host (TEST INFRASTRUCTURE ONLY;
// g++ through tests/emu/hip/hip_runtime.h).  One case per call, named by argv[1], its input on stdin (every float as the decimal
// value of its 32 bits); tests/test_recentre_host.py holds the output to tests/recentre_ref.py by equality.
//
//   shift  nx ny nz dx dy dz, nx * ny * nz words  -> "stats <kept> <exposed> <left>", then the word of every new voxel: the gather
//                                                    the kernels run (grid_shift_source per voxel, 0x7FC00000 where it is false;
//                                                    an exposed voxel counts its grid_shift_mirror when that word is no NaN)
//   check  origin0[3] resolution s[3] d[3]        -> "ok <s'[3]> <bits of origin'[3]>" or "refused <s[3]>" (s as it was)
//   clip   nx ny nz lo[3] hi[3]                   -> "0", or "1 <lo[3]> <hi[3]>" clipped
//   mark   min_points only_unknown l_mark l_min l_max, n, n x (count, bits of L) -> per voxel: written candidate observed bits-of-L
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "lv_grid.hpp"

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
static unsigned int bits_of(float f) {
    unsigned int u;
    memcpy(&u, &f, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "shift")) {
        GridDims g{};
        g.nx = (int)read_i();
        g.ny = (int)read_i();
        g.nz = (int)read_i();
        const int32_t dx = (int32_t)read_i(), dy = (int32_t)read_i(), dz = (int32_t)read_i();
        const size_t n = grid_cells(g);
        std::vector<unsigned int> src(n), dst(n);   // exactly the grid: the sanitizer watches a source or a mirror outside it
        for (unsigned int& v : src) v = (unsigned int)read_i();
        unsigned long long kept = 0, exposed = 0, left = 0;
        for (size_t c = 0; c < n; ++c) {
            int i, j, k, si, sj, sk;
            grid_ijk(g, (uint32_t)c, i, j, k);
            if (grid_shift_source(g, dx, dy, dz, i, j, k, si, sj, sk)) {
                dst[c] = src[grid_at(g, si, sj, sk)];
                ++kept;
            } else {
                dst[c] = 0x7FC00000u;
                grid_shift_mirror(g, i, j, k, si, sj, sk);
                const unsigned int m = src[grid_at(g, si, sj, sk)];
                left += (m & 0x7FFFFFFFu) > 0x7F800000u ? 0 : 1;
                ++exposed;
            }
        }
        printf("stats %llu %llu %llu\n", kept, exposed, left);
        for (unsigned int v : dst) printf("%u\n", v);
    } else if (!strcmp(what, "check")) {
        float origin0[3];
        for (float& o : origin0) o = read_f();
        const float resolution = read_f();
        int32_t s[3], d[3], s_new[3] = {0, 0, 0};
        float origin_new[3] = {0.f, 0.f, 0.f};
        for (int32_t& v : s) v = (int32_t)read_i();
        for (int32_t& v : d) v = (int32_t)read_i();
        if (grid_shift_check(origin0, resolution, s, d, s_new, origin_new))
            printf("refused %d %d %d\n", s[0], s[1], s[2]);
        else
            printf("ok %d %d %d %u %u %u\n", s_new[0], s_new[1], s_new[2], bits_of(origin_new[0]), bits_of(origin_new[1]), bits_of(origin_new[2]));
    } else if (!strcmp(what, "clip")) {
        GridDims g{};
        g.nx = (int)read_i();
        g.ny = (int)read_i();
        g.nz = (int)read_i();
        int lo[3], hi[3], clo[3], chi[3];
        for (int& v : lo) v = (int)read_i();
        for (int& v : hi) v = (int)read_i();
        if (grid_clip_box(g, lo, hi, clo, chi))
            printf("1 %d %d %d %d %d %d\n", clo[0], clo[1], clo[2], chi[0], chi[1], chi[2]);
        else
            printf("0\n");
    } else if (!strcmp(what, "mark")) {
        const uint32_t min_points = (uint32_t)read_i();
        const bool only_unknown = read_i() != 0;
        const float l_mark = read_f(), l_min = read_f(), l_max = read_f();
        for (long long n = read_i(); n > 0; --n) {
            const uint32_t count = (uint32_t)read_i();
            float L = read_f();
            bool candidate = false, observed = false;
            const bool written = grid_mark_voxel(count, min_points, only_unknown, l_mark, l_min, l_max, L, candidate, observed);
            printf("%d %d %d %u\n", written ? 1 : 0, candidate ? 1 : 0, observed ? 1 : 0, bits_of(L));
        }
    } else {
        return 2;
    }
    return 0;
}
