// lv_occupancy.hpp — the ray-cast occupancy grid (lv_occ_*, include/limovelo_hip.h "Occupancy grid"; kernels and host side in
// lv_occupancy.hip).
//
// The first part is the rule itself as plain __host__ __device__ code without atomics: the quantisation, the return's range
// rules and world transform, the integer walk and the log-odds update.  The kernels of lv_occupancy.hip run exactly these
// functions; tests/emu/occupancy_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_occupancy_host.py
// holds them to tests/occupancy_ref.py.  After occ_quant every step is integer arithmetic, so the three agree on every voxel.
// The quantisation itself, the cell arithmetic and the projection of a column are lv_grid.hpp's.
#pragma once

#include "../../include/limovelo_hip.h"
#include "lv_buffers.hpp"
#include "lv_grid.hpp"

namespace lv {

struct TsdfStore;   // lv_tsdf.hpp: what from_surface() reads

constexpr int OCC_MAX_VIEWS = 32;
constexpr int OCC_MAX_DIM = 1024;
constexpr uint64_t OCC_MAX_VOXELS = (uint64_t)1 << 28;
constexpr float OCC_T_LIMIT = 8192.0f;       // a sensor origin this many voxels from the grid's origin gives no evidence
constexpr float OCC_RANGE_LIMIT = 4096.0f;   // max_range / resolution

// The grid and the constants of one lv_occ_integrate / lv_occ_query as the kernels take them
struct OccGrid {
    float origin[3];
    float resolution;
    int nx, ny, nz;
    int wx;                       // words per x row of a bitmap: (nx + 31) / 32
    float min_range2, max_range2; // min_range * min_range, max_range * max_range (f32 products)
    float max_range;
    float l_hit, l_miss, l_min, l_max;
};

// The view's sensor origin in sub-units; false: the view gives no evidence (t non-finite or >= 8192 voxels from the origin)
LV_OCC_HD bool occ_view_origin(const OccGrid& g, const float t[3], int32_t qs[3]) {
    for (int a = 0; a < 3; ++a) {
        const float c = (t[a] - g.origin[a]) / g.resolution;
        if (!(fabsf(c) < OCC_T_LIMIT)) return false;   // (NaN and inf fail the comparison too)
        qs[a] = (int32_t)floorf(c * OCC_SUB);
    }
    return true;
}

enum : int { OCC_RAY_IGNORED = 0, OCC_RAY_HIT = 1, OCC_RAY_CUT = 2 };

// One return (x, y, z) of a view at pose (R row-major, t): its quantised end point, and whether it is ignored, a hit or cut
LV_OCC_HD int occ_return(const OccGrid& g, const float R[9], const float t[3], float x, float y, float z, int32_t qe[3]) {
    const float inf = __builtin_huge_valf();
    if (!(fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf)) return OCC_RAY_IGNORED;
    const float r2 = x * x + y * y + z * z;
    if (r2 < g.min_range2) return OCC_RAY_IGNORED;
    int kind = OCC_RAY_HIT;
    if (r2 > g.max_range2) {
        const float c = g.max_range / sqrtf(r2);
        x = x * c;
        y = y * c;
        z = z * c;
        kind = OCC_RAY_CUT;
    }
    for (int a = 0; a < 3; ++a) {
        const float w = ((R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + t[a];
        if (!occ_quant(w, g.origin[a], g.resolution, qe[a])) return OCC_RAY_IGNORED;
    }
    return kind;
}

// The walk from qs to qe.  Named scalars, no indexed arrays: the state lives in registers on the device.
struct OccWalk {
    int32_t vx, vy, vz;   // the cell the walk stands in
    int32_t ex, ey, ez;   // ve, where it ends
    int32_t sx, sy, sz;   // step per axis: sign(d)
    int32_t rx, ry, rz;   // steps left per axis
    int32_t nx, ny, nz;   // numerator of the distance to the next boundary (sub-units); below 2^26
    int32_t ax, ay, az;   // |d| per axis; below 2^25 (the products need int64)
};

LV_OCC_HD void occ_walk_axis(int32_t qs, int32_t qe, int32_t& v, int32_t& e, int32_t& s, int32_t& r, int32_t& n, int32_t& ad) {
    const int32_t d = qe - qs;
    ad = d < 0 ? -d : d;
    s = (d > 0) - (d < 0);
    v = qs >> 8;
    e = qe >> 8;
    r = e > v ? e - v : v - e;
    n = s > 0 ? (v + 1) * 256 - qs : (s < 0 ? qs - v * 256 : 0);   // ((v + 1) << 8, v << 8: a product, v may be negative)
}

LV_OCC_HD void occ_walk_init(OccWalk& w, const int32_t qs[3], const int32_t qe[3]) {
    occ_walk_axis(qs[0], qe[0], w.vx, w.ex, w.sx, w.rx, w.nx, w.ax);
    occ_walk_axis(qs[1], qe[1], w.vy, w.ey, w.sy, w.ry, w.ny, w.ay);
    occ_walk_axis(qs[2], qe[2], w.vz, w.ez, w.sz, w.rz, w.nz, w.az);
}

LV_OCC_HD bool occ_walk_done(const OccWalk& w) { return (w.rx | w.ry | w.rz) == 0; }

// a before b (a the lower axis: it wins the tie): n_a / ad_a <= n_b / ad_b by cross-multiplication
LV_OCC_HD bool occ_first(int32_t na, int32_t ada, int32_t nb, int32_t adb) { return (int64_t)na * (int64_t)adb <= (int64_t)nb * (int64_t)ada; }

// One step: among the axes with steps left the one whose boundary comes first, ties to x, then y, then z.  Returns the axis.
LV_OCC_HD int occ_walk_step(OccWalk& w) {
    int a = -1;
    if (w.rx > 0) a = 0;
    if (w.ry > 0 && !(a == 0 && occ_first(w.nx, w.ax, w.ny, w.ay))) a = 1;
    if (w.rz > 0) {
        if (a < 0) a = 2;
        else if (a == 0) { if (!occ_first(w.nx, w.ax, w.nz, w.az)) a = 2; }
        else if (!occ_first(w.ny, w.ay, w.nz, w.az)) a = 2;
    }
    if (a == 0) { w.vx += w.sx; w.nx += 256; --w.rx; }
    else if (a == 1) { w.vy += w.sy; w.ny += 256; --w.ry; }
    else { w.vz += w.sz; w.nz += 256; --w.rz; }
    return a;
}

LV_OCC_HD bool occ_in_grid(const OccGrid& g, int32_t i, int32_t j, int32_t k) { return grid_inside(g, i, j, k); }

// true: the walk stands outside the grid on an axis it does not move back along, so neither a later cell nor ve is in the grid
LV_OCC_HD bool occ_walk_left(const OccGrid& g, const OccWalk& w) {
    return (w.vx < 0 && w.sx <= 0) || (w.vx >= g.nx && w.sx >= 0) || (w.vy < 0 && w.sy <= 0) || (w.vy >= g.ny && w.sy >= 0) ||
           (w.vz < 0 && w.sz <= 0) || (w.vz >= g.nz && w.sz >= 0);
}

// One update of a voxel: unknown (NaN) starts from 0, the sum is clamped
LV_OCC_HD float occ_update(float L, float delta, float l_min, float l_max) { return fminf(fmaxf((L != L ? 0.0f : L) + delta, l_min), l_max); }

inline void default_occupancy_params(lv_occupancy_params* p) {
    if (!p) return;
    p->origin[0] = -51.2f;
    p->origin[1] = -51.2f;
    p->origin[2] = -3.2f;
    p->resolution = 0.2f;
    p->nx = 512;
    p->ny = 512;
    p->nz = 64;
    p->min_range = 1.f;
    p->max_range = 80.f;
    p->l_hit = 0.85f;
    p->l_miss = -0.4f;
    p->l_min = -2.f;
    p->l_max = 3.5f;
    p->l_occ = 0.4f;
    p->l_free = -0.4f;
}

// (lv_occ_mark judges its parameters in lv_api.hip, before the context)
inline void default_occ_mark_params(lv_occ_mark_params* p) {
    if (!p) return;
    *p = lv_occ_mark_params{};
    for (int a = 0; a < 3; ++a) p->hi[a] = 1 << 30;   // (clipped to the grid: the whole of it)
    p->min_points = 1;
    p->only_unknown = 1;
    p->l_mark = 0.85f;
}

// The parameters against their limits: NULL when they hold, otherwise what is wrong (lv_occ_configure: LV_EINVAL)
inline const char* occ_check_params(const lv_occupancy_params* p) {
    if (!p) return "null params";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(p->origin[a])) return "origin: must be finite";
    if (!(std::isfinite(p->resolution) && p->resolution > 0.f)) return "resolution: must be finite and > 0";
    if (p->nx < 1 || p->nx > OCC_MAX_DIM || p->ny < 1 || p->ny > OCC_MAX_DIM || p->nz < 1 || p->nz > OCC_MAX_DIM)
        return "nx, ny, nz: each must be in 1..1024";
    if ((uint64_t)p->nx * (uint64_t)p->ny * (uint64_t)p->nz > OCC_MAX_VOXELS) return "nx * ny * nz: at most 2^28 voxels";
    if (!(std::isfinite(p->min_range) && std::isfinite(p->max_range) && p->min_range > 0.f && p->min_range < p->max_range))
        return "ranges: finite, 0 < min_range < max_range";
    if (!(p->max_range / p->resolution <= OCC_RANGE_LIMIT)) return "max_range / resolution: at most 4096";
    if (!(std::isfinite(p->l_hit) && std::isfinite(p->l_miss) && p->l_miss < 0.f && p->l_hit > 0.f)) return "l_miss < 0 < l_hit, finite";
    if (!(std::isfinite(p->l_min) && std::isfinite(p->l_max) && p->l_min < 0.f && p->l_max > 0.f)) return "l_min < 0 < l_max, finite";
    if (!(std::isfinite(p->l_occ) && std::isfinite(p->l_free) && p->l_free < p->l_occ)) return "l_free < l_occ, finite";
    return nullptr;
}

inline OccGrid occ_grid_of(const lv_occupancy_params& p) {
    OccGrid g{};
    for (int a = 0; a < 3; ++a) g.origin[a] = p.origin[a];
    g.resolution = p.resolution;
    g.nx = p.nx; g.ny = p.ny; g.nz = p.nz;
    g.wx = (p.nx + 31) / 32;
    g.min_range2 = p.min_range * p.min_range;
    g.max_range2 = p.max_range * p.max_range;
    g.max_range = p.max_range;
    g.l_hit = p.l_hit; g.l_miss = p.l_miss; g.l_min = p.l_min; g.l_max = p.l_max;
    return g;
}

// The grid of a context and the buffers of its calls.  Nothing is allocated before configure().
struct OccStore {
    bool configured = false;
    lv_occupancy_params prm{};
    OccGrid grid{};
    size_t n_vox = 0;
    size_t n_words = 0;            // words of ONE bitmap, padded to a multiple of 4 (the fold reads uint4)
    DevBuf<float> d_L;             // log-odds by grid_at; NaN = never observed
    DevBuf<float> d_L2;            // a recentre gathers into it and the two swap; lv_occ_mark's counts.  Not allocated before the first of either
    float origin0[3] = {0.f, 0.f, 0.f};   // the origin of configure(); prm.origin and grid.origin are grid_shift_origin(origin0, shift)
    int32_t shift[3] = {0, 0, 0};  // the accumulated recentre, in voxels
    DevBuf<uint32_t> d_bits;       // crossed bitmap, then hit bitmap: bit (i & 31) of word (k * ny + j) * wx + (i >> 5); all zero between views
    Counters4 stats;               // the 4 counters of the call in flight
    PointStage pts;                // every view's returns, or the query points
    DevBuf<float> d_out;           // lv_occ_query's results
    DevBuf<int8_t> d_proj;         // lv_occ_project's result (nx * ny)
    DevBuf<uint32_t> d_sbits;      // lv_occ_from_surface's three bitmaps of the TSDF volume (SOLID, OPEN, a spare), in d_bits' layout.  Not allocated before the first call

    int configure(hipStream_t stream, const lv_occupancy_params& p);
    int clear(hipStream_t stream);
    int integrate(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t out[4]);
    int query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* logodds);
    int project(hipStream_t stream, int k_lo, int k_hi, int8_t* grid2d);
    int fetch(hipStream_t stream, float* logodds);
    int load(hipStream_t stream, const float* logodds);
    // d: not all zero; s_new, origin_new: grid_shift_check's.  out: voxels kept, exposed, that held evidence and left, 0
    int recentre(hipStream_t stream, const int32_t d[3], const int32_t s_new[3], const float origin_new[3], uint64_t out[4]);
    // lo..hi: already clipped to the grid, not empty.  The points: map_orig (the map's float4 per id, n_ids of them; the living ones count) or the caller's
    int mark(hipStream_t stream, const lv_occ_mark_params& p, const int lo[3], const int hi[3], const void* map_orig, uint32_t n_ids,
             const void* points, size_t stride, size_t n, uint64_t out[4]);
    // lv_surf_occ.hip ("Occupancy from the surface").  lo..hi: already clipped to the grid, not empty.  out: voxels classed OCCUPIED,
    // classed FREE, voxels whose bits changed, voxels OUTSIDE the volume
    int from_surface(hipStream_t stream, const TsdfStore& tsdf, const lv_occ_surface_params& p, const int lo[3], const int hi[3], uint64_t out[4]);
    void release();
};

}  // namespace lv
