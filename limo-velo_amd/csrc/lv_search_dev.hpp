// lv_search_dev.hpp — device primitives of the exact voxel-hash k-NN search shared by the measurement pass (lv_match.hip) and
// the map queries (lv_query.hip): candidate keys and their compare-exchange, calc_dist, the query's voxel geometry and the
// guaranteed radii of its blocks (search_radius, block_radius).  Exactness of the ladder: lv_match.hip header.  Moved here
// unchanged from lv_match.hip, whose kernels compile to the same instructions with it.
#pragma once

#include "lv_host.hpp"

namespace lv {

// Candidate keys.  A key packs (f32 distance bits << 32 | position) and is handled as an IEEE f64:
// for non-negative distances the f64 order of the bit pattern equals the unsigned order, so ONE
// v_min_f64 / v_max_f64 pair is a compare-exchange on the (distance, position) pair.  Inside a bucket
// the points are stored in ascending ORIGINAL index, so (distance, position) order == the reference's
// (distance, index) order, ties included; the generic path uses (distance, index) directly.
// NONE = largest finite f64 (its high word 0x7FEFFFFF is an f32 NaN pattern no distance produces;
// no key is ever an f64 NaN/inf because valid distance bits are <= 0x7F800000).
typedef double kkey;
__device__ __forceinline__ kkey make_key(float d, uint32_t low) {
    return __longlong_as_double((long long)(((uint64_t)__float_as_uint(d) << 32) | (uint64_t)low));
}
// the key of a candidate slot that may lie behind the end of its run: selects, not a branch around the distance arithmetic (the
// compiler turns `ok ? make_key(calc_dist(...), j) : none_key()` into an exec-mask region per candidate: save / branch / wait /
// restore around eight instructions).  Level-0 stream: search phase 13.4 -> 13.2 us per launch; level 1: see bucket_attempt
// (the loads have to be pinned in front of the arithmetic there).
__device__ __forceinline__ kkey make_key_if(bool ok, float d, uint32_t low) {
    const uint32_t hi = ok ? __float_as_uint(d) : 0x7FEFFFFFu;
    const uint32_t lo = ok ? low : 0xFFFFFFFFu;
    return __hiloint2double((int)hi, (int)lo);
}
__device__ __forceinline__ uint32_t key_lo(kkey k) { return (uint32_t)(uint64_t)__double_as_longlong(k); }
__device__ __forceinline__ uint32_t key_hi(kkey k) { return (uint32_t)((uint64_t)__double_as_longlong(k) >> 32); }
#define LV_NONE_BITS 0x7FEFFFFFFFFFFFFFll
__device__ __forceinline__ kkey none_key() { return __longlong_as_double(LV_NONE_BITS); }
__device__ __forceinline__ bool is_none(kkey k) { return __double_as_longlong(k) == LV_NONE_BITS; }


__device__ __forceinline__ kkey kmin(kkey a, kkey b) {
    kkey r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ kkey kmax(kkey a, kkey b) {
    kkey r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void cswap(kkey& a, kkey& b) {
    const kkey lo = kmin(a, b), hi = kmax(a, b);
    a = lo;
    b = hi;
}

// [UPSTREAM-RECALL ikd-Tree calc_dist]: (ax-bx)^2 + (ay-by)^2 + (az-bz)^2, f32, left to right, unfused
struct __attribute__((packed, aligned(4))) Xyz {   // one bucket point as streamed: 12 bytes
    float x, y, z;
};
__device__ __forceinline__ float calc_dist(float qx, float qy, float qz, Xyz m) {
    float dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
    float sx = dx * dx, sy = dy * dy, sz = dz * dz;
    float s = sx + sy;
    return s + sz;
}
__device__ __forceinline__ float calc_dist(float qx, float qy, float qz, float4 m) {
    float dx = qx - m.x, dy = qy - m.y, dz = qz - m.z;
    float sx = dx * dx, sy = dy * dy, sz = dz * dz;
    float s = sx + sy;
    return s + sz;
}

// Voxel geometry of one query: continuous and integer level-0 voxel coordinates.
struct QGeom {
    float tx, ty, tz;
    int c0x, c0y, c0z, amax;
};
__device__ __forceinline__ QGeom make_geom(const MapView& map, float qx, float qy, float qz) {
    QGeom g;
    g.tx = (qx - map.origin[0]) * map.inv_cell;
    g.ty = (qy - map.origin[1]) * map.inv_cell;
    g.tz = (qz - map.origin[2]) * map.inv_cell;
    g.c0x = cell_coord(qx, map.origin[0], map.inv_cell);
    g.c0y = cell_coord(qy, map.origin[1], map.inv_cell);
    g.c0z = cell_coord(qz, map.origin[2], map.inv_cell);
    g.amax = max(abs(g.c0x - CELL_OFFSET), max(abs(g.c0y - CELL_OFFSET), abs(g.c0z - CELL_OFFSET)));
    return g;
}
// guaranteed search radius of the 27-voxel block at `lvl` for THIS query: one voxel edge plus the distance to
// the nearest wall of its own voxel, shrunk by 1e-3 relative and by the f32 rounding bound of the voxel
// coordinates (see file header).
__device__ __forceinline__ float search_radius(const MapView& map, const QGeom& g, int lvl) {
    const float scale = (float)(1 << lvl);
    const float bx = (float)((((g.c0x >> lvl) << lvl)) - CELL_OFFSET), by = (float)((((g.c0y >> lvl) << lvl)) - CELL_OFFSET),
                bz = (float)((((g.c0z >> lvl) << lvl)) - CELL_OFFSET);
    const float mx = fminf(g.tx - bx, scale - (g.tx - bx)), my = fminf(g.ty - by, scale - (g.ty - by)),
                mz = fminf(g.tz - bz, scale - (g.tz - bz));
    const float marg = fmaxf(fminf(mx, fminf(my, mz)), 0.f);
    return map.cell * ((scale + marg) * 0.999f - 8.f * 1.1920928955078125e-07f * ((float)g.amax + 2.f * scale));
}

__device__ __forceinline__ kkey shfl_xor_key(kkey v, int mask) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, mask);
    hi = __shfl_xor(hi, mask);
    return __hiloint2double(hi, lo);
}

// a candidate key stands for a real point iff its distance is finite (NONE and the +inf distance of deleted
// entries / ids are not)
__device__ __forceinline__ bool key_real(kkey k) { return key_hi(k) < 0x7F800000u; }

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// guaranteed radius of a block of `side` level-`lvl` voxels per axis whose lower corner is voxel (bx, by, bz) (level-lvl voxel
// coordinates) for THIS query: the distance to the nearest face, shrunk like search_radius
__device__ __forceinline__ float block_radius(const MapView& map, const QGeom& g, int lvl, int bx, int by, int bz, int side) {
    const float lox = (float)((bx << lvl) - CELL_OFFSET), loy = (float)((by << lvl) - CELL_OFFSET), loz = (float)((bz << lvl) - CELL_OFFSET);
    const float ext = (float)(side << lvl);
    const float mx = fminf(g.tx - lox, lox + ext - g.tx), my = fminf(g.ty - loy, loy + ext - g.ty), mz = fminf(g.tz - loz, loz + ext - g.tz);
    const float m = fmaxf(fminf(mx, fminf(my, mz)), 0.f);
    return map.cell * (m * 0.999f - 8.f * 1.1920928955078125e-07f * ((float)g.amax + 2.f * ext));
}

}  // namespace lv
