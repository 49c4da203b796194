// tests/emu/surf_occ_emu.cpp — the rule of limo-velo_amd/csrc/lv_surf_occ.hpp run on the host, voxel by voxel (TEST INFRASTRUCTURE ONLY;
// g++ through tests/emu/hip/hip_runtime.h, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer; a stand-alone
// program).  tests/test_surf_occ_host.py holds its output to tests/surf_occ_ref.py by equality.
//
//   surf_occ_emu run <in> <out>   one lv_occ_from_surface as VolumeTools::occ_from_surface and the kernels do it: the box clipped
//                                 (grid_clip_box), per voxel surf_occ_voxel_of, surf_occ_class_by_gather and surf_occ_write.  Also
//                                 holds surf_occ_axis_range, which lv_surf_occ.hip limits its bitmap passes by, to the voxels met.
//       <in>  (native endianness): float og_origin[3], og_resolution, l_min, l_max; int32 og_n[3] (nx, ny, nz);
//             float tg_origin[3], tg_resolution; int32 tg_n[3]; lv_occ_surface_params; int32 S[], W[] of the volume; float L[]
//       <out> uint64 stats[4]; float L'[]
//   surf_occ_emu check            stdin lines "min_weight band reach mode l_solid_bits l_open_bits" or "null"; per line "ok" or
//                                 surf_occ_check_params' message
//   surf_occ_emu defaults         lv_default_occ_surface_params' fields on one line
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../limo-velo_amd/csrc/lv_surf_occ.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

namespace {

template <class T>
void get(FILE* f, T* p, size_t n) {
    if (fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

int run(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    OccGrid og{}, tg{};
    get(f, og.origin, 3);
    get(f, &og.resolution, 1);
    get(f, &og.l_min, 1);
    get(f, &og.l_max, 1);
    int n[3];
    get(f, n, 3);
    og.nx = n[0]; og.ny = n[1]; og.nz = n[2];
    get(f, tg.origin, 3);
    get(f, &tg.resolution, 1);
    get(f, n, 3);
    tg.nx = n[0]; tg.ny = n[1]; tg.nz = n[2];
    lv_occ_surface_params p;
    get(f, &p, 1);
    std::vector<int32_t> S(grid_cells(tg)), W(grid_cells(tg));
    std::vector<float> L(grid_cells(og));
    get(f, S.data(), S.size());
    get(f, W.data(), W.size());
    get(f, L.data(), L.size());
    fclose(f);
    char why[96];
    if (!surf_occ_check_params(&p, why, sizeof(why))) {
        fprintf(stderr, "%s\n", why);
        return 3;
    }

    uint64_t st[4] = {0, 0, 0, 0};
    int lo[3], hi[3];
    if (grid_clip_box(og, p.lo, p.hi, lo, hi)) {
        const float a = surf_occ_clamped(p.l_solid, og.l_min, og.l_max), b = surf_occ_clamped(p.l_open, og.l_min, og.l_max);
        const int tn[3] = {tg.nx, tg.ny, tg.nz};
        int u0[3], u1[3];
        for (int ax = 0; ax < 3; ++ax) surf_occ_axis_range(og.origin[ax], og.resolution, tg.origin[ax], tg.resolution, lo[ax], hi[ax], tn[ax], u0[ax], u1[ax]);
        for (int k = lo[2]; k <= hi[2]; ++k)
            for (int j = lo[1]; j <= hi[1]; ++j)
                for (int i = lo[0]; i <= hi[0]; ++i) {
                    int u[3], cls = SURF_OCC_NONE;
                    if (surf_occ_voxel_of(og, tg, i, j, k, u[0], u[1], u[2])) {
                        for (int ax = 0; ax < 3; ++ax)
                            if (u[ax] < u0[ax] || u[ax] > u1[ax]) {
                                fprintf(stderr, "voxel (%d, %d, %d): u[%d] = %d outside surf_occ_axis_range's %d..%d\n", i, j, k, ax, u[ax], u0[ax], u1[ax]);
                                return 4;
                            }
                        cls = surf_occ_class_by_gather(tg, S.data(), W.data(), p.min_weight, p.band, p.reach, u[0], u[1], u[2]);
                    } else {
                        ++st[3];
                    }
                    st[0] += cls == SURF_OCC_OCCUPIED;
                    st[1] += cls == SURF_OCC_FREE;
                    const size_t at = grid_at(og, i, j, k);
                    float v;
                    if (surf_occ_write(p.mode, cls, L[at], a, b, p.l_solid, p.l_open, og.l_min, og.l_max, v)) {
                        L[at] = v;
                        ++st[2];
                    }
                }
    }
    f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(st, sizeof(uint64_t), 4, f);
    fwrite(L.data(), sizeof(float), L.size(), f);
    fclose(f);
    return 0;
}

int check() {
    char line[256], why[96];
    while (fgets(line, sizeof(line), stdin)) {
        lv_occ_surface_params p;
        default_occ_surface_params(&p);
        unsigned int a = 0, b = 0;
        const bool null = line[0] == 'n';
        if (!null) {
            if (sscanf(line, "%d %d %d %d %u %u", &p.min_weight, &p.band, &p.reach, &p.mode, &a, &b) != 6) return 2;
            p.l_solid = __uint_as_float(a);
            p.l_open = __uint_as_float(b);
        }
        if (surf_occ_check_params(null ? nullptr : &p, why, sizeof(why))) printf("ok\n");
        else printf("%s\n", why);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "run" && argc == 4) return run(argv[2], argv[3]);
    if (what == "check") return check();
    if (what == "defaults") {
        lv_occ_surface_params p;
        default_occ_surface_params(nullptr);
        default_occ_surface_params(&p);
        printf("%d %d %d %d %d %d %d %d %d %d %u %u\n", p.lo[0], p.lo[1], p.lo[2], p.hi[0], p.hi[1], p.hi[2], p.min_weight, p.band, p.reach, p.mode,
               __float_as_uint(p.l_solid), __float_as_uint(p.l_open));
        return 0;
    }
    fprintf(stderr, "usage: surf_occ_emu run <in> <out> | check | defaults\n");
    return 2;
}
