// lv_elevation.hpp — the elevation map and the traversability class per cell (lv_elev_*, include/limovelo_hip.h "Elevation map";
// kernels and host side in lv_elevation.hip).
//
// The first part is the rule as plain __host__ __device__ code without atomics: the cell and integer height of a point, the body
// band, which cell is known, the terrain of a known cell from its 8-neighbourhood, the class and the height in metres.  The kernels
// of lv_elevation.hip run exactly these functions; tests/emu/elevation_emu.cpp compiles them with g++ through
// tests/emu/hip/hip_runtime.h and tests/test_elevation_host.py holds them to tests/elevation_ref.py.  After occ_quant (lv_grid.hpp's,
// as it is) every step is integer arithmetic, and the layers are integer minima, maxima and sums, which commute: the three agree
// on every cell whatever the order of the points.
//
// The defaults (lv_default_elevation_params) over the occupancy default's footprint, resolution 0.2: min_points 3, head 1920
// (1.5 m), max_span 153 (0.12 m), max_step 128 (0.10 m), each floor(metres / resolution * 256), and max_slope2 34727 =
// floor((512 tan 20 deg)^2).
#pragma once

#include "../../include/limovelo_hip.h"
#include "lv_buffers.hpp"
#include "lv_grid.hpp"

namespace lv {

constexpr int32_t ELEV_NONE = LV_ELEV_NONE;
constexpr int ELEV_MAX_DIM = 4096;
constexpr uint64_t ELEV_MAX_CELLS = (uint64_t)1 << 24;
constexpr int ELEV_MAX_POINTS_MIN = 1 << 20;   // min_points up to this
constexpr int ELEV_MAX_SUB = 1 << 25;          // head, max_span, max_step up to this
constexpr uint64_t ELEV_MAX_N = 0x7FFFFFFFull; // lv_elev_build, lv_elev_query: n below this
constexpr int ELEV_LAYERS = 9;                 // LV_ELEV_LO .. LV_ELEV_HEIGHT

// The grid and the thresholds as the kernels take them (nz = 1: lv_grid.hpp's cell and tile arithmetic applies)
struct ElevGrid {
    float origin[3];
    float resolution;
    int nx, ny, nz;
    int min_points, head, max_span, max_step, max_slope2;
};

// The cell and the integer height of world point p; false: the point is ignored
LV_OCC_HD bool elev_point(const ElevGrid& g, const float p[3], uint32_t& cell, int32_t& z) {
    int32_t qx, qy;
    // (all three are quantised before any is judged, as grid_cell_of does)
    bool ok = occ_quant(p[0], g.origin[0], g.resolution, qx);
    ok = occ_quant(p[1], g.origin[1], g.resolution, qy) && ok;
    ok = occ_quant(p[2], g.origin[2], g.resolution, z) && ok;
    if (!ok) return false;
    const int i = qx >> 8, j = qy >> 8;
    if (!grid_inside(g, i, j, 0)) return false;
    cell = (uint32_t)grid_at(g, i, j, 0);
    return true;
}

// z of a used point of a cell whose lowest point is lo: in the body band, or overhang
LV_OCC_HD bool elev_in_band(int32_t z, int32_t lo, int head) { return z - lo <= head; }   // (0 <= z - lo < 2^25)

LV_OCC_HD bool elev_known(uint32_t nb, int min_points) { return nb >= (uint32_t)min_points; }

// One component of the gradient from lo at -1, 0, +1 along an axis; known_m / known_p: that neighbour is in the grid and known
LV_OCC_HD int64_t elev_gradient(int32_t lo_m, bool known_m, int32_t lo_0, int32_t lo_p, bool known_p) {
    if (known_m && known_p) return (int64_t)lo_p - (int64_t)lo_m;
    if (known_p) return 2 * ((int64_t)lo_p - (int64_t)lo_0);
    if (known_m) return 2 * ((int64_t)lo_0 - (int64_t)lo_m);
    return 0;
}

// step and slope2 of a KNOWN cell whose lowest point is lo0.  nb(di, dj): lo of the neighbour at that offset if it lies in the grid
// and is known, ELEV_NONE otherwise (a known cell's lo is below 2^24, so the two never meet).
template <class Neighbour>
LV_OCC_HD void elev_terrain(int32_t lo0, Neighbour& nb, int32_t& step, int32_t& slope2) {
    int32_t s = 0;
    for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
            if (!di && !dj) continue;
            const int32_t v = nb(di, dj);
            if (v == ELEV_NONE) continue;
            const int32_t d = v > lo0 ? v - lo0 : lo0 - v;   // (below 2^25)
            s = d > s ? d : s;
        }
    step = s;
    const int32_t xm = nb(-1, 0), xp = nb(1, 0), ym = nb(0, -1), yp = nb(0, 1);
    const int64_t gx = elev_gradient(xm, xm != ELEV_NONE, lo0, xp, xp != ELEV_NONE);
    const int64_t gy = elev_gradient(ym, ym != ELEV_NONE, lo0, yp, yp != ELEV_NONE);
    const int64_t s2 = gx * gx + gy * gy;   // (|g| < 2^26: below 2^53)
    slope2 = s2 > (int64_t)0x7FFFFFFF ? (int32_t)0x7FFFFFFF : (int32_t)s2;
}

LV_OCC_HD int elev_class(bool known, int32_t span, int32_t step, int32_t slope2, const ElevGrid& g) {
    if (!known) return -1;
    return (span > g.max_span || step > g.max_step || slope2 > g.max_slope2) ? 100 : 0;
}

// metres: origin_z + resolution * (lo / 256), in that order; NaN for a cell that is not known
LV_OCC_HD float elev_height(bool known, int32_t lo, float origin_z, float resolution) {
    if (!known) return __uint_as_float(0x7FC00000u);
    const float c = (float)lo / OCC_SUB;
    const float m = resolution * c;
    return origin_z + m;
}

// What lv_elev_query answers for world point p: the cell (z is not used), or false
LV_OCC_HD bool elev_query_cell(const ElevGrid& g, const float p[3], uint32_t& cell) {
    int i, j, k;
    if (!grid_cell_of(g, g.origin, g.resolution, true, p, i, j, k)) return false;
    cell = (uint32_t)grid_at(g, i, j, 0);
    return true;
}

inline void default_elevation_params(lv_elevation_params* p) {
    if (!p) return;
    *p = lv_elevation_params{};
    p->origin[0] = -51.2f;
    p->origin[1] = -51.2f;
    p->origin[2] = -3.2f;
    p->resolution = 0.2f;
    p->nx = 512;
    p->ny = 512;
    p->min_points = 3;
    p->head = 1920;        // 1.5 m: floor(m / resolution * 256)
    p->max_span = 153;     // 0.12 m
    p->max_step = 128;     // 0.10 m
    p->max_slope2 = 34727; // floor((512 tan 20 deg)^2)
}

// The parameters against their limits: NULL when they hold, otherwise what is wrong (lv_elev_build: LV_EINVAL)
inline const char* elev_check_params(const lv_elevation_params* p) {
    if (!p) return "null params";
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(p->origin[a]) < __builtin_huge_valf())) return "origin: must be finite";
    if (!(p->resolution > 0.f && p->resolution < __builtin_huge_valf())) return "resolution: finite and > 0";
    if (p->nx < 1 || p->nx > ELEV_MAX_DIM || p->ny < 1 || p->ny > ELEV_MAX_DIM) return "nx, ny: 1..4096 each";
    if ((uint64_t)p->nx * (uint64_t)p->ny > ELEV_MAX_CELLS) return "nx * ny: at most 2^24 cells";
    if (p->min_points < 1 || p->min_points > ELEV_MAX_POINTS_MIN) return "min_points: 1..2^20";
    if (p->head < 0 || p->head > ELEV_MAX_SUB) return "head: 0..2^25 sub-units";
    if (p->max_span < 0 || p->max_span > ELEV_MAX_SUB) return "max_span: 0..2^25 sub-units";
    if (p->max_step < 0 || p->max_step > ELEV_MAX_SUB) return "max_step: 0..2^25 sub-units";
    if (p->max_slope2 < 0) return "max_slope2: 0..2^31 - 1";
    return nullptr;
}

inline ElevGrid elev_grid_of(const lv_elevation_params& p) {
    ElevGrid g{};
    for (int a = 0; a < 3; ++a) g.origin[a] = p.origin[a];
    g.resolution = p.resolution;
    g.nx = p.nx;
    g.ny = p.ny;
    g.nz = 1;
    g.min_points = p.min_points;
    g.head = p.head;
    g.max_span = p.max_span;
    g.max_step = p.max_step;
    g.max_slope2 = p.max_slope2;
    return g;
}

// bytes per element of a layer of lv_elev_fetch; 0: no such layer
inline size_t elev_layer_size(int layer) {
    if (layer < 0 || layer >= ELEV_LAYERS) return 0;
    return layer == LV_ELEV_CLASS ? 1 : 4;
}

// The tile of the terrain kernel: one lane per cell of a 32 x 8 tile, a row of the tile one run of 32 cells
constexpr int ELEV_TX = 32, ELEV_TY = 8;
using ElevTile = HaloTile<ELEV_TX, ELEV_TY, 1>;

// The elevation map of a context and the buffers of its calls.  Nothing is allocated before the first build().
struct ElevStore {
    bool built = false;
    int from_map = 0;
    uint64_t n_points = 0;
    lv_elevation_params prm{};
    ElevGrid grid{};
    size_t n_cells = 0;
    DevBuf<int32_t> d_lo, d_top, d_span, d_step, d_slope2;   // the layers, by cell
    DevBuf<uint32_t> d_n, d_nb;
    DevBuf<int8_t> d_cls;
    DevBuf<float> d_height;
    DevBuf<unsigned long long> d_part;   // one record of 4 per workgroup of the terrain kernel
    Counters4 stats;
    PointStage pts;                      // the caller's points of a build, the points of a query
    DevBuf<float> d_qh;                  // per query point the height ...
    DevBuf<int8_t> d_qc;                 // ... and the class

    // map_orig: the map's points by id (n_ids of them, dead ones included) when pts is NULL
    int build(hipStream_t stream, const lv_elevation_params& p, const float4* map_orig, uint32_t n_ids, uint64_t n_living, const void* pts,
              size_t stride, size_t n, uint64_t out[4]);
    int fetch(hipStream_t stream, int layer, void* out);
    int query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* height, int8_t* cls);
    void release();
};

}  // namespace lv
