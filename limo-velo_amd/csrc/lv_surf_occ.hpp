// lv_surf_occ.hpp — the occupancy grid filled from the TSDF surface (lv_occ_from_surface, include/limovelo_hip.h "Occupancy from
// the surface"; kernels and host side in lv_surf_occ.hip).
//
// The rule itself as plain __host__ __device__ code: the parameter check and the defaults, the class of a TSDF voxel, the centre of
// an occupancy voxel and the TSDF voxel it falls into, the class of an occupancy voxel by the plain gather over the cube of
// `reach`, and the write rule of the four modes.  The kernels of lv_surf_occ.hip run these functions (the gather as bitmaps: a
// voxel's class bit, grown axis by axis, is the same OR over the same cube); tests/emu/surf_occ_emu.cpp compiles them with g++
// through tests/emu/hip/hip_runtime.h and tests/test_surf_occ_host.py holds them to tests/surf_occ_ref.py.  One f32 step (the
// centre and its quantisation, lv_grid.hpp's occ_quant), integers after it: the three agree on every bit.
#pragma once

#include <cmath>
#include <cstdio>

#include "lv_occupancy.hpp"

namespace lv {

constexpr int SURF_OCC_MAX_WEIGHT = 1 << 18;   // min_weight's limit: TSDF_MAX_WEIGHT
constexpr int SURF_OCC_MAX_BAND = 4096;        // |band|: 16 voxels, the widest truncation band
constexpr int SURF_OCC_MAX_REACH = 4;
constexpr uint32_t SURF_OCC_NAN_BITS = 0x7FC00000u;

enum : int { SURF_VOX_UNKNOWN = 0, SURF_VOX_OPEN = 1, SURF_VOX_SOLID = 2 };   // a TSDF voxel
enum : int { SURF_OCC_NONE = 0, SURF_OCC_FREE = 1, SURF_OCC_OCCUPIED = 2 };   // an occupancy voxel

inline void default_occ_surface_params(lv_occ_surface_params* p) {
    if (!p) return;
    *p = lv_occ_surface_params{};
    for (int a = 0; a < 3; ++a) p->hi[a] = 1 << 30;   // (clipped to the grid: the whole of it)
    p->min_weight = 1;
    p->band = 0;
    p->reach = 0;
    p->mode = LV_OCC_SURFACE_FILL;
    p->l_solid = 3.5f;
    p->l_open = -2.0f;
}

// The parameters against their limits: true when they hold, otherwise `why` says what is wrong (lv_occ_from_surface: LV_EINVAL,
// before the context).  The box is not judged: it is clipped.
inline bool surf_occ_check_params(const lv_occ_surface_params* p, char* why, size_t n) {
    if (!p) { snprintf(why, n, "null params"); return false; }
    if (p->min_weight < 1 || p->min_weight > SURF_OCC_MAX_WEIGHT) { snprintf(why, n, "min_weight = %d: must be in 1..2^18", p->min_weight); return false; }
    if (p->band < -SURF_OCC_MAX_BAND || p->band > SURF_OCC_MAX_BAND) { snprintf(why, n, "band = %d: must be in -4096..4096", p->band); return false; }
    if (p->reach < 0 || p->reach > SURF_OCC_MAX_REACH) { snprintf(why, n, "reach = %d: must be in 0..4", p->reach); return false; }
    if (p->mode < LV_OCC_SURFACE_FILL || p->mode > LV_OCC_SURFACE_ACCUMULATE) { snprintf(why, n, "mode = %d: must be in 0..3", p->mode); return false; }
    if (!(std::isfinite(p->l_solid) && p->l_solid > 0.f)) { snprintf(why, n, "l_solid = %g: finite and > 0", (double)p->l_solid); return false; }
    if (!(std::isfinite(p->l_open) && p->l_open < 0.f)) { snprintf(why, n, "l_open = %g: finite and < 0", (double)p->l_open); return false; }
    return true;
}

// A TSDF voxel: KNOWN iff W >= min_weight; SOLID iff KNOWN and S <= band * W (its fused distance is at most band / 256 voxel)
LV_OCC_HD int surf_occ_class_of_voxel(int32_t S, int32_t W, int32_t min_weight, int32_t band) {
    if (W < min_weight) return SURF_VOX_UNKNOWN;
    return (int64_t)S <= (int64_t)band * (int64_t)W ? SURF_VOX_SOLID : SURF_VOX_OPEN;
}

// The centre of voxel v of a grid along one axis: f32, unfused, in exactly this order
LV_OCC_HD float surf_occ_centre(float origin, float resolution, int v) { return origin + (((float)v + 0.5f) * resolution); }

// One axis of the way from occupancy voxel v to the TSDF voxel u its centre falls into (n_t voxels along that axis); false: the
// centre does not quantise, or u is not in the volume
LV_OCC_HD bool surf_occ_axis_of(float origin_g, float resolution_g, float origin_t, float resolution_t, int n_t, int v, int& u) {
    int32_t q;
    if (!occ_quant(surf_occ_centre(origin_g, resolution_g, v), origin_t, resolution_t, q)) return false;
    u = q >> 8;
    return (uint32_t)u < (uint32_t)n_t;
}

// The TSDF voxel u that occupancy voxel (i, j, k) falls into; false: OUTSIDE (an axis does not quantise, or u is not in the volume).
// og: the occupancy grid, tg: the TSDF volume's, both at their current origins.
LV_OCC_HD bool surf_occ_voxel_of(const OccGrid& og, const OccGrid& tg, int i, int j, int k, int& ui, int& uj, int& uk) {
    const bool x = surf_occ_axis_of(og.origin[0], og.resolution, tg.origin[0], tg.resolution, tg.nx, i, ui);
    const bool y = surf_occ_axis_of(og.origin[1], og.resolution, tg.origin[1], tg.resolution, tg.ny, j, uj);
    const bool z = surf_occ_axis_of(og.origin[2], og.resolution, tg.origin[2], tg.resolution, tg.nz, k, uk);
    return x && y && z;
}

// The class of an occupancy voxel that falls into TSDF voxel u, by the plain gather: OCCUPIED iff a voxel of the cube of Chebyshev
// radius `reach` round u, inside the volume, is SOLID; else FREE iff u itself is OPEN (free space is never grown); else NONE.
LV_OCC_HD int surf_occ_class_by_gather(const OccGrid& tg, const int32_t* S, const int32_t* W, int32_t min_weight, int32_t band, int reach, int ui, int uj,
                                       int uk) {
    for (int dk = -reach; dk <= reach; ++dk)
        for (int dj = -reach; dj <= reach; ++dj)
            for (int di = -reach; di <= reach; ++di) {
                if (!grid_inside(tg, ui + di, uj + dj, uk + dk)) continue;
                const size_t at = grid_at(tg, ui + di, uj + dj, uk + dk);
                if (surf_occ_class_of_voxel(S[at], W[at], min_weight, band) == SURF_VOX_SOLID) return SURF_OCC_OCCUPIED;
            }
    const size_t at = grid_at(tg, ui, uj, uk);
    return surf_occ_class_of_voxel(S[at], W[at], min_weight, band) == SURF_VOX_OPEN ? SURF_OCC_FREE : SURF_OCC_NONE;
}

LV_OCC_HD uint32_t surf_occ_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return b;
}
LV_OCC_HD float surf_occ_float(uint32_t b) {
    float v;
    __builtin_memcpy(&v, &b, sizeof(v));
    return v;
}

// l_solid and l_open inside the grid's own clamps: what FILL, OVERWRITE and REPLACE write
LV_OCC_HD float surf_occ_clamped(float l, float l_min, float l_max) { return fminf(fmaxf(l, l_min), l_max); }

// The write rule: what a voxel of class `cls` that holds L holds after the call in `mode` (a, b: the clamped l_solid, l_open).
// true: its 32 bits change, and `out` is what to write.
LV_OCC_HD bool surf_occ_write(int mode, int cls, float L, float a, float b, float l_solid, float l_open, float l_min, float l_max, float& out) {
    out = L;
    if (cls == SURF_OCC_NONE) {
        if (mode == LV_OCC_SURFACE_REPLACE) out = surf_occ_float(SURF_OCC_NAN_BITS);
    } else {
        const bool solid = cls == SURF_OCC_OCCUPIED;
        if (mode == LV_OCC_SURFACE_ACCUMULATE) out = occ_update(L, solid ? l_solid : l_open, l_min, l_max);
        else if (mode != LV_OCC_SURFACE_FILL || L != L) out = solid ? a : b;
    }
    return surf_occ_bits(out) != surf_occ_bits(L);
}

// The TSDF voxels the occupancy voxels lo..hi of one axis can fall into, u0..u1 (inclusive, clipped to 0..n - 1; u0 > u1: none
// can).  Every step of surf_occ_centre and occ_quant_f is a correctly rounded f32 operation with a positive factor, so u is a
// monotone function of v and the ends of the box bound it.  A coordinate that is not finite gives the whole axis.
inline void surf_occ_axis_range(float origin_g, float resolution_g, float origin_t, float resolution_t, int lo, int hi, int n, int& u0, int& u1) {
    const float f0 = occ_quant_f(surf_occ_centre(origin_g, resolution_g, lo), origin_t, resolution_t);
    const float f1 = occ_quant_f(surf_occ_centre(origin_g, resolution_g, hi), origin_t, resolution_t);
    u0 = 0;
    u1 = n - 1;
    if (!(std::isfinite(f0) && std::isfinite(f1))) return;
    const float top = (float)n * OCC_SUB;   // (u >= n from here on)
    if (f1 < 0.f || f0 >= top) { u0 = 1; u1 = 0; return; }
    if (f0 > 0.f) u0 = (int32_t)f0 >> 8;
    if (f1 < top) u1 = (int32_t)f1 >> 8;
}

}  // namespace lv
