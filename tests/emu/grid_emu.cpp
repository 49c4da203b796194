// tests/emu/grid_emu.cpp — the host-and-device part of limo-velo_amd/csrc/lv_grid.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++
// through tests/emu/hip/hip_runtime.h).  One case per call, named by argv[1], its input on stdin (every float as the decimal value
// of its 32 bits); tests/test_grid_host.py holds the output to numpy by equality.
//
//   cells    nx ny nz                                   -> "cells <grid_cells>", then per cell index: i j k of grid_ijk and grid_at of them
//   inside   nx ny nz, n, n x (i j k)                   -> per triple grid_inside as 0 / 1
//   cell_of  origin[3] resolution nx ny nz planar, n, n x (x y z)   -> per point: ok i j k (zeros when not ok)
//   project  nz plane k_lo k_hi l_occ l_free, nz * plane values of L -> "band <k0> <k1>", then grid_project_column of every column
//   tile     TX TY TZ                                   -> "dims HZ LX LY LZ CELLS LCELLS"; per cell of the haloed local box
//                                                          "box i j k <at> <halo_of(at)>"; per lane and q "lane <lane> <q> <local_of>"
//   tiles    TX TY TZ nx ny nz                          -> "tiles <count>", then per tile "tx ty tz" of origin_of
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

static GridDims read_dims() {
    GridDims g{};
    g.nx = (int)read_i();
    g.ny = (int)read_i();
    g.nz = (int)read_i();
    return g;
}

template <class T>
static void tile_case() {
    printf("dims %d %d %d %d %d %d\n", T::HZ, T::LX, T::LY, T::LZ, T::CELLS, T::LCELLS);
    std::vector<int> slot_seen(T::LCELLS, 0);   // exactly LCELLS: the sanitizer watches a slot past the box
    for (int k = -T::HZ; k < T::LZ - T::HZ; ++k)
        for (int j = -1; j < T::LY - 1; ++j)
            for (int i = -1; i < T::LX - 1; ++i) {
                const int l = T::at(i, j, k);
                ++slot_seen[(size_t)l];
                int di, dj, dk;
                T::halo_of(l, di, dj, dk);
                printf("box %d %d %d %d %d %d %d\n", i, j, k, l, di, dj, dk);
            }
    for (int lane = 0; lane < 256; ++lane)
        for (int q = 0; q < T::CELLS / 256; ++q) {
            int i, j, k;
            T::local_of(lane + q * 256, i, j, k);
            printf("lane %d %d %d %d %d\n", lane, q, i, j, k);
        }
}

template <class T>
static void tiles_case(const GridDims& g) {
    const size_t n = T::tiles(g);
    printf("tiles %zu\n", n);
    for (size_t t = 0; t < n; ++t) {
        int tx, ty, tz;
        T::origin_of(g, (uint32_t)t, tx, ty, tz);
        printf("%d %d %d\n", tx, ty, tz);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "cells")) {
        const GridDims g = read_dims();
        const size_t n = grid_cells(g);
        printf("cells %zu\n", n);
        for (size_t c = 0; c < n; ++c) {
            int i, j, k;
            grid_ijk(g, (uint32_t)c, i, j, k);
            printf("%d %d %d %zu\n", i, j, k, grid_at(g, i, j, k));
        }
    } else if (!strcmp(what, "inside")) {
        const GridDims g = read_dims();
        for (long long n = read_i(); n > 0; --n) {
            const int i = (int)read_i(), j = (int)read_i(), k = (int)read_i();
            printf("%d\n", grid_inside(g, i, j, k) ? 1 : 0);
        }
    } else if (!strcmp(what, "cell_of")) {
        float origin[3];
        for (float& o : origin) o = read_f();
        const float resolution = read_f();
        const GridDims g = read_dims();
        const bool planar = read_i() != 0;
        for (long long n = read_i(); n > 0; --n) {
            float p[3];
            for (float& x : p) x = read_f();
            int i = 0, j = 0, k = 0;
            const bool ok = grid_cell_of(g, origin, resolution, planar, p, i, j, k);
            printf("%d %d %d %d\n", ok ? 1 : 0, ok ? i : 0, ok ? j : 0, ok ? k : 0);
        }
    } else if (!strcmp(what, "project")) {
        const int nz = (int)read_i();
        const size_t plane = (size_t)read_i();
        const int k_lo = (int)read_i(), k_hi = (int)read_i();
        const float l_occ = read_f(), l_free = read_f();
        std::vector<float> L((size_t)nz * plane);   // exactly the grid: the sanitizer watches a layer outside the clipped band
        for (float& v : L) v = read_f();
        int k0, k1;
        grid_clip_band(k_lo, k_hi, nz, k0, k1);
        printf("band %d %d\n", k0, k1);
        for (size_t c = 0; c < plane; ++c) printf("%d\n", grid_project_column(L.data(), plane, c, k0, k1, l_occ, l_free));
    } else if (!strcmp(what, "tile") || !strcmp(what, "tiles")) {
        const int tx = (int)read_i(), ty = (int)read_i(), tz = (int)read_i();
        const bool count = !strcmp(what, "tiles");
        const GridDims g = count ? read_dims() : GridDims{};
        if (tx == 32 && ty == 32 && tz == 1) count ? tiles_case<HaloTile<32, 32, 1>>(g) : tile_case<HaloTile<32, 32, 1>>();
        else if (tx == 8 && ty == 8 && tz == 8) count ? tiles_case<HaloTile<8, 8, 8>>(g) : tile_case<HaloTile<8, 8, 8>>();
        else if (tx == 32 && ty == 8 && tz == 4) count ? tiles_case<HaloTile<32, 8, 4>>(g) : tile_case<HaloTile<32, 8, 4>>();
        else return 2;
    } else {
        return 2;
    }
    return 0;
}
