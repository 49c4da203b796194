// lv_distance.hpp — the Euclidean distance field over the occupancy grid (lv_occ_distance_*, include/limovelo_hip.h "Distance
// field"; kernels and host side in lv_distance.hip).
//
// The first part is the rule as plain __host__ __device__ code: which voxel is an obstacle, the three separable passes of the
// exact squared transform, truncation, metres and the gradient.  The kernels of lv_distance.hip run exactly these functions;
// tests/emu/distance_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_distance_host.py holds
// them to tests/distance_ref.py.  Everything up to the metres is integer arithmetic, so the three agree on every voxel.
//
// One signed buffer carries both transforms.  A voxel that is not an obstacle holds its (partial) squared distance to the nearest
// obstacle, > 0; an obstacle holds minus its squared distance to the nearest voxel that is not one, < 0 (0 in an unsigned field).
// The sign therefore tells the class, and a pass reads from a neighbour of the OTHER class 0 and from one of its own class that
// neighbour's partial distance: the outside and the inside transform run in the same three passes.
#pragma once

#include "lv_occupancy.hpp"

namespace lv {

constexpr int32_t DIST_FAR = LV_OCC_FAR;
constexpr int DIST_MAX_CELLS = 1024;

// The field's shape and the constants of its passes as the kernels take them
struct DistGrid {
    int nx, ny, nz;   // of the FIELD: nz = 1 when planar
    int wx;           // words per x row of the obstacle bitmap
    int reach;        // offsets per axis a pass looks at: max_cells, or 1024 without truncation
    int signed_field;
    float resolution;
};

// 3-D field: L >= l_occ (NaN compares false), or unknown when unknown counts
LV_OCC_HD bool dist_obstacle(float L, float l_occ, bool unknown_is_obstacle) { return L >= l_occ || (unknown_is_obstacle && L != L); }

// planar field: column c of lv_occ_project over the clipped layers k0..k1 is 100, or -1 when unknown counts
LV_OCC_HD bool dist_obstacle_planar(const float* L, size_t plane, size_t c, int k0, int k1, float l_occ, float l_free, bool unknown_is_obstacle) {
    const int v = grid_project_column(L, plane, c, k0, k1, l_occ, l_free);
    return v == 100 || (unknown_is_obstacle && v == -1);
}

// planar field over the caller's cells (lv_occ_distance_build_cells): the value is 100, or negative when unknown counts
LV_OCC_HD bool dist_obstacle_cell(int v, bool unknown_is_obstacle) { return v == 100 || (unknown_is_obstacle && v < 0); }

// word w of a bitmap row; inv: the complement, without the bits past nx
LV_OCC_HD uint32_t dist_word(const uint32_t* row, int wx, int nx, int w, bool inv) {
    uint32_t v = row[w];
    if (inv) {
        v = ~v;
        if (w == wx - 1 && (nx & 31)) v &= (1u << (nx & 31)) - 1u;
    }
    return v;
}

// |i - i'| to the nearest set bit i' of the row (of its complement with inv), -1 when there is none
LV_OCC_HD int dist_row_nearest(const uint32_t* row, int wx, int nx, int i, bool inv) {
    const int w0 = i >> 5, b = i & 31;
    int best = -1;
    uint32_t v = dist_word(row, wx, nx, w0, inv) & (b == 31 ? 0xFFFFFFFFu : (2u << b) - 1u);   // bits at or below i
    int w = w0;
    while (!v && w > 0) v = dist_word(row, wx, nx, --w, inv);
    if (v) best = i - (w * 32 + 31 - __builtin_clz(v));
    v = dist_word(row, wx, nx, w0, inv) & (0xFFFFFFFFu << b);   // bits at or above i
    w = w0;
    while (!v && w < wx - 1) v = dist_word(row, wx, nx, ++w, inv);
    if (v) {
        const int d = w * 32 + __builtin_ctz(v) - i;
        if (best < 0 || d < best) best = d;
    }
    return best;
}

// X pass: the signed partial value of voxel i of a row
LV_OCC_HD int32_t dist_pass_x(const DistGrid& g, const uint32_t* row, int i) {
    const bool obstacle = (row[i >> 5] >> (i & 31)) & 1u;
    if (obstacle && !g.signed_field) return 0;
    const int d = dist_row_nearest(row, g.wx, g.nx, i, obstacle);
    if (d < 0 || d > g.reach) return obstacle ? -DIST_FAR : DIST_FAR;
    return obstacle ? -(d * d) : d * d;
}

// Y and Z pass: min over j' of g(j') + (j - j')^2 along a line of n values `stride` apart, for the value at j.  g(j') is 0 where
// j' is of the other class, the magnitude of its value otherwise.  Scans outward from j and stops once (j - j')^2 >= the best
// so far (exact: no farther j' can do better), or after `reach` offsets.
LV_OCC_HD int32_t dist_pass_line(const int32_t* line, size_t stride, int n, int j, int reach) {
    const int32_t own = line[(size_t)j * stride];
    const bool inside = own <= 0;
    int32_t best = inside ? -own : own;
    const int lo = j, hi = n - 1 - j;
    int far = lo > hi ? lo : hi;
    if (far > reach) far = reach;
    for (int d = 1; d <= far; ++d) {
        const int32_t dd = d * d;
        if (dd >= best) break;
        if (d <= lo) {
            const int32_t v = line[(size_t)(j - d) * stride];
            const int32_t t = inside ? -v : v;
            if (t <= 0) best = dd;
            else if (t != DIST_FAR && t + dd < best) best = t + dd;
        }
        if (d <= hi) {
            const int32_t v = line[(size_t)(j + d) * stride];
            const int32_t t = inside ? -v : v;
            if (t <= 0) { if (dd < best) best = dd; }
            else if (t != DIST_FAR && t + dd < best) best = t + dd;
        }
    }
    return inside ? -best : best;
}

// The stored value of a finished transform: beyond max_cells it is FAR
LV_OCC_HD int32_t dist_truncate(int32_t s, int max_cells) {
    if (max_cells == 0 || s == DIST_FAR || s == -DIST_FAR) return s;
    const int32_t lim = max_cells * max_cells;
    if (s > lim) return DIST_FAR;
    if (s < -lim) return -DIST_FAR;
    return s;
}

// resolution * sqrtf(|s2|) with the sign of s2; 0 -> +0, FAR -> inf
LV_OCC_HD float dist_metres(int32_t s2, float resolution) {
    if (s2 == 0) return 0.0f;
    if (s2 == DIST_FAR) return __builtin_huge_valf();
    if (s2 == -DIST_FAR) return -__builtin_huge_valf();
    const float m = resolution * sqrtf((float)(s2 < 0 ? -s2 : s2));
    return s2 < 0 ? -m : m;
}

LV_OCC_HD bool dist_finite(float m) { return fabsf(m) < __builtin_huge_valf(); }   // (NaN fails too)

// One component of the gradient from the metre values at v - e, v, v + e; has_minus / has_plus: that neighbour is in the grid
LV_OCC_HD float dist_gradient(float m_minus, float m0, float m_plus, bool has_minus, bool has_plus, float resolution) {
    if (!dist_finite(m0)) return 0.0f;
    const bool um = has_minus && dist_finite(m_minus), up = has_plus && dist_finite(m_plus);
    if (um && up) return (m_plus - m_minus) / (resolution + resolution);
    if (up) return (m_plus - m0) / resolution;
    if (um) return (m0 - m_minus) / resolution;
    return 0.0f;
}

// One query point against a finished field: dist, and grad[3] when grad is not NULL
LV_OCC_HD void dist_query_point(const DistGrid& g, const float origin[3], bool planar, const int32_t* s2, const float p[3], float* dist, float* grad) {
    int i, j, k;
    if (!grid_cell_of(g, origin, g.resolution, planar, p, i, j, k)) {
        *dist = __uint_as_float(0x7FC00000u);
        if (grad) grad[0] = grad[1] = grad[2] = 0.0f;
        return;
    }
    const size_t step[3] = {1, (size_t)g.nx, (size_t)g.nx * (size_t)g.ny};
    const int v[3] = {i, j, k}, n[3] = {g.nx, g.ny, g.nz};
    const size_t at = grid_at(g, i, j, k);
    const float m0 = dist_metres(s2[at], g.resolution);
    *dist = m0;
    if (!grad) return;
    for (int a = 0; a < 3; ++a) {
        const bool hm = v[a] > 0, hp = v[a] < n[a] - 1;
        const float mm = hm ? dist_metres(s2[at - step[a]], g.resolution) : 0.0f;
        const float mp = hp ? dist_metres(s2[at + step[a]], g.resolution) : 0.0f;
        grad[a] = dist_gradient(mm, m0, mp, hm, hp, g.resolution);
    }
}

inline void default_distance_params(lv_distance_params* p) {
    if (!p) return;
    *p = lv_distance_params{};
}

// The parameters against their limits: NULL when they hold, otherwise what is wrong (lv_occ_distance_build: LV_EINVAL)
inline const char* dist_check_params(const lv_distance_params* p) {
    if (!p) return "null params";
    if (p->max_cells < 0 || p->max_cells > DIST_MAX_CELLS) return "max_cells: 0 (no truncation) or 1..1024";
    if (p->planar && p->k_lo > p->k_hi) return "planar layers: k_lo <= k_hi";
    return nullptr;
}

// The same for lv_occ_distance_build_cells: a planar field, whose layers are not used
inline const char* dist_check_params_cells(const lv_distance_params* p, const int8_t* cells) {
    if (!p) return "null params";
    if (p->max_cells < 0 || p->max_cells > DIST_MAX_CELLS) return "max_cells: 0 (no truncation) or 1..1024";
    if (!p->planar) return "planar: a field over cells is planar (planar != 0)";
    if (!cells) return "null cells";
    return nullptr;
}

inline DistGrid dist_grid_of(const OccGrid& o, const lv_distance_params& p) {
    DistGrid g{};
    g.nx = o.nx;
    g.ny = o.ny;
    g.nz = p.planar ? 1 : o.nz;
    g.wx = o.wx;
    g.reach = p.max_cells ? p.max_cells : DIST_MAX_CELLS;
    g.signed_field = p.signed_field != 0;
    g.resolution = o.resolution;
    return g;
}

// The field of a context and the buffers of its calls.  Nothing is allocated before the first build().
struct DistStore {
    bool built = false;
    int stale = 0;
    int32_t shift[3] = {0, 0, 0};   // the grid's accumulated shift at the build (lv_volume_shift_info)
    lv_distance_params prm{};
    DistGrid grid{};
    float origin[3] = {0.f, 0.f, 0.f};
    size_t n_vox = 0;                // of the field
    DevBuf<int32_t> d_s2;            // the field, by grid_at
    DevBuf<int32_t> d_tmp;           // the Y pass's output; lv_occ_distance_fetch's metres
    DevBuf<uint32_t> d_bits;         // obstacle bitmap, the occupancy bitmaps' layout
    DevBuf<unsigned long long> d_part;   // one record of 4 per workgroup of the Z pass
    Counters4 stats;
    PointStage pts;                  // the query points
    DevBuf<float> d_out;             // per point dist, then grad[3]
    DevBuf<int8_t> d_cells;          // lv_occ_distance_build_cells: the caller's cells (not allocated before the first such build)

    // cells: NULL (the obstacles come from the grid), or nx * ny values of the plane (p.planar != 0)
    int build(hipStream_t stream, const OccStore& occ, const lv_distance_params& p, const int8_t* cells, uint64_t out[4]);
    int fetch(hipStream_t stream, int32_t* s2, float* metres);
    int query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* dist, float* grad);
    void release();
};

}  // namespace lv
