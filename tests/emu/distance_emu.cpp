// tests/emu/distance_emu.cpp — the rule of limo-velo_amd/csrc/lv_distance.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  The loops below are the kernels of lv_distance.hip one "lane" after another: classify into the
// bitmap, the X, Y and Z passes, truncation and the stats, then the metres and the query.  tests/test_distance_host.py holds its
// output to tests/distance_ref.py.
//
// stdin (every float as the decimal value of its 32 bits):
//   origin[3] resolution nx ny nz l_occ l_free
//   planar k_lo k_hi unknown_is_obstacle signed_field max_cells
//   nx * ny * nz log-odds
//   n_points, then n x (x y z)
// stdout:
//   "params ok" or "params bad: <why>" (and nothing more)
//   "field <nx> <ny> <nz>", the s2 values on one line, the bits of the metres on the next
//   "stats <obstacles> <finite> <max d2_out> <max d2_in>"
//   per point one line: the bits of dist and of grad[3]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "lv_distance.hpp"

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
    lv_occupancy_params op{};
    for (int a = 0; a < 3; ++a) op.origin[a] = read_f();
    op.resolution = read_f();
    op.nx = (int)read_i(); op.ny = (int)read_i(); op.nz = (int)read_i();
    op.l_occ = read_f(); op.l_free = read_f();
    lv_distance_params dp{};
    dp.planar = (int)read_i(); dp.k_lo = (int)read_i(); dp.k_hi = (int)read_i();
    dp.unknown_is_obstacle = (int)read_i(); dp.signed_field = (int)read_i(); dp.max_cells = (int)read_i();
    if (const char* why = dist_check_params(&dp)) {
        printf("params bad: %s\n", why);
        return 0;
    }
    printf("params ok\n");
    const size_t n_grid = (size_t)op.nx * op.ny * op.nz;
    std::vector<float> L(n_grid);
    for (float& x : L) x = read_f();
    OccGrid og{};
    for (int a = 0; a < 3; ++a) og.origin[a] = op.origin[a];
    og.resolution = op.resolution;
    og.nx = op.nx; og.ny = op.ny; og.nz = op.nz;
    og.wx = (op.nx + 31) / 32;
    const DistGrid g = dist_grid_of(og, dp);
    const size_t nv = (size_t)g.nx * g.ny * g.nz, rows = (size_t)g.ny * g.nz, plane = (size_t)g.nx * g.ny;

    // classify: exactly wx words per row, nothing beyond (the sanitizer watches the row ends)
    std::vector<uint32_t> bits(rows * g.wx, 0u);
    const int k0 = dp.k_lo < 0 ? 0 : dp.k_lo, k1 = dp.k_hi >= og.nz ? og.nz - 1 : dp.k_hi;
    for (size_t row = 0; row < rows; ++row)
        for (int i = 0; i < g.nx; ++i) {
            const bool ob = dp.planar ? dist_obstacle_planar(L.data(), plane, row * g.nx + i, k0, k1, op.l_occ, op.l_free, dp.unknown_is_obstacle != 0)
                                      : dist_obstacle(L[row * g.nx + i], op.l_occ, dp.unknown_is_obstacle != 0);
            if (ob) bits[row * g.wx + (i >> 5)] |= 1u << (i & 31);
        }
    std::vector<int32_t> a(nv), b(nv);
    for (size_t v = 0; v < nv; ++v) a[v] = dist_pass_x(g, bits.data() + (v / g.nx) * g.wx, (int)(v % g.nx));
    for (size_t v = 0; v < nv; ++v) {
        const size_t k = v / plane, r = v % plane, j = r / g.nx, i = r % g.nx;
        b[v] = dist_pass_line(a.data() + k * plane + i, (size_t)g.nx, g.ny, (int)j, g.reach);
    }
    unsigned long long ob = 0, fin = 0, mo = 0, mi = 0;
    for (size_t v = 0; v < nv; ++v) {
        const size_t k = v / plane, r = v % plane;
        const int32_t s = dist_truncate(dist_pass_line(b.data() + r, plane, g.nz, (int)k, g.reach), dp.max_cells);
        a[v] = s;
        ob += s <= 0;
        if (s != DIST_FAR && s != -DIST_FAR) {
            ++fin;
            if (s > 0 && (unsigned long long)s > mo) mo = (unsigned long long)s;
            if (s < 0 && (unsigned long long)(-s) > mi) mi = (unsigned long long)(-s);
        }
    }
    printf("field %d %d %d\n", g.nx, g.ny, g.nz);
    for (size_t v = 0; v < nv; ++v) printf("%d ", a[v]);
    printf("\n");
    for (size_t v = 0; v < nv; ++v) printf("%u ", __float_as_uint(dist_metres(a[v], g.resolution)));
    printf("\nstats %llu %llu %llu %llu\n", ob, fin, mo, mi);
    const long n = read_i();
    for (long i = 0; i < n; ++i) {
        float p[3], d, gr[3];
        for (float& x : p) x = read_f();
        dist_query_point(g, og.origin, dp.planar != 0, a.data(), p, &d, gr);
        printf("%u %u %u %u\n", __float_as_uint(d), __float_as_uint(gr[0]), __float_as_uint(gr[1]), __float_as_uint(gr[2]));
        float d2 = 0.f;
        dist_query_point(g, og.origin, dp.planar != 0, a.data(), p, &d2, nullptr);   // (without a gradient: the same dist)
        if (__float_as_uint(d2) != __float_as_uint(d)) { printf("dist differs without grad\n"); return 3; }
    }
    return 0;
}
