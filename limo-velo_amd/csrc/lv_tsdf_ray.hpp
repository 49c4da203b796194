// lv_tsdf_ray.hpp — ray casting on the TSDF surface (lv_surf_raycast, lv_surf_raycast_views, include/limovelo_hip.h "Surface ray
// casting"; kernels and host side in lv_tsdf_ray.hip, the packed states a member of TsdfStore).
//
// The rule as plain __host__ __device__ code without atomics: the cell states, the walk that reads them, the depth of the stop,
// the normal and the colour.  The walk is lv_occupancy.hpp's (occ_walk_init / occ_walk_step, unchanged), the ends are lv_ray.hpp's
// (ray_ends on TsdfGrid::occ), the packed layout is lv_ray.hpp's (ray_pack / ray_unpack / ray_word_of, read through RayStates), the
// crossing is the mesh's (tsdf_crossing) and the colour the layer's (colour_voxel).  The kernels of lv_tsdf_ray.hip run exactly
// these functions; tests/emu/tsdf_ray_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and
// tests/test_tsdf_ray_host.py holds them to tests/tsdf_ray_ref.py.  After the quantisation of the ends every step but the normal
// is integer arithmetic, and the normal is a fixed sequence of unfused f32 operations, so the three agree on every bit.
#pragma once

#include "lv_colour.hpp"
#include "lv_ray.hpp"

namespace lv {

constexpr uint64_t SURF_MAX_N = 0x7FFFFFFFull;   // lv_surf_raycast: n below this

// The states of a cell, 2 bits in the packed volume
enum : int { SURF_UNKNOWN = 0, SURF_OUT = 1, SURF_IN = 2 };

inline void default_tsdf_ray_params(lv_tsdf_ray_params* p) {
    if (!p) return;
    *p = lv_tsdf_ray_params{};
    p->min_weight = 1;
}

// KNOWN iff W >= min_weight; a KNOWN cell is IN iff S < 0
LV_OCC_HD int surf_state_voxel(int32_t S, int32_t W, int32_t min_weight) { return W < min_weight ? SURF_UNKNOWN : (S < 0 ? SURF_IN : SURF_OUT); }

LV_OCC_HD void surf_ignored(lv_tsdf_ray_result& r) {
    r.status = LV_SURF_IGNORED;
    r.cell = -1;
    r.steps = r.axis = r.depth = r.t = r.n_known = r.n_unknown = 0;
}

// What the depth of a stop needs beside the record: the step that entered c_s*
struct SurfStop {
    int32_t bx, by, bz;   // B = c_s*
    int32_t num, den;     // num_s*, den_s* (0, 1 when s* = 0)
};

// ---- the walk from qs to qe over the cells c_0 .. c_S.  st: the states (state(g, i, j, k) of an in-grid cell, RayStates over the
// packed volume on the device).  Fills every field of r but depth and t.
template <class States>
LV_OCC_HD void surf_walk(const OccGrid& g, const int32_t qs[3], const int32_t qe[3], States& st, lv_tsdf_ray_result& r, SurfStop& h) {
    OccWalk w;
    occ_walk_init(w, qs, qe);
    const int32_t total = w.rx + w.ry + w.rz;
    int32_t steps = 0, axis = -1, num = 0, den = 1, n_known = 0, n_unknown = 0;
    bool prev_out = false;   // c_(s - 1) is inside the grid and OUT
    for (;;) {
        bool out_here = false;
        if (occ_in_grid(g, w.vx, w.vy, w.vz)) {
            const int s = st.state(g, w.vx, w.vy, w.vz);
            if (s == SURF_IN) {
                r.status = prev_out ? LV_SURF_HIT : LV_SURF_BLOCKED;
                r.cell = (int32_t)grid_at(g, w.vx, w.vy, w.vz);
                r.steps = steps; r.axis = axis; r.n_known = n_known; r.n_unknown = n_unknown;
                h.bx = w.vx; h.by = w.vy; h.bz = w.vz; h.num = num; h.den = den;
                return;
            }
            out_here = s == SURF_OUT;
            n_known += out_here;
            n_unknown += s == SURF_UNKNOWN;
        } else if (occ_walk_left(g, w)) {
            break;
        }
        if (occ_walk_done(w)) break;
        prev_out = out_here;
        const int32_t nx = w.nx, ny = w.ny, nz = w.nz;   // n_a as it stands BEFORE the step adds 256
        axis = occ_walk_step(w);
        num = axis == 0 ? nx : axis == 1 ? ny : nz;
        den = axis == 0 ? w.ax : axis == 1 ? w.ay : w.az;
        ++steps;
    }
    r.status = LV_SURF_CLEAR;
    r.cell = occ_in_grid(g, w.ex, w.ey, w.ez) ? (int32_t)grid_at(g, w.ex, w.ey, w.ez) : -1;
    r.steps = total; r.axis = -1; r.n_known = n_known; r.n_unknown = n_unknown;
    h.bx = h.by = h.bz = 0; h.num = 0; h.den = 1;
}

// The linear index of A = c_(s* - 1) of a HIT: B one step back along the axis the ray entered it across
LV_OCC_HD size_t surf_cell_a(const OccGrid& g, const int32_t qs[3], const int32_t qe[3], const lv_tsdf_ray_result& r) {
    const int32_t da = r.axis == 0 ? qe[0] - qs[0] : r.axis == 1 ? qe[1] - qs[1] : qe[2] - qs[2];
    const size_t stride = r.axis == 0 ? (size_t)1 : r.axis == 1 ? (size_t)g.nx : (size_t)g.nx * (size_t)g.ny;
    return da > 0 ? (size_t)r.cell - stride : (size_t)r.cell + stride;
}

// ---- depth and t of a walked ray.  S, W are read here, at the stop, and nowhere before it.
LV_OCC_HD void surf_depth(const OccGrid& g, const int32_t qs[3], const int32_t qe[3], const int32_t* S, const int32_t* W, const SurfStop& h,
                          lv_tsdf_ray_result& r) {
    const int64_t dx = (int64_t)qe[0] - qs[0], dy = (int64_t)qe[1] - qs[1], dz = (int64_t)qe[2] - qs[2];
    const int64_t l2 = dx * dx + dy * dy + dz * dz;
    const int64_t len = tsdf_isqrt(l2);
    r.t = -1;
    if (r.status == LV_SURF_CLEAR) {
        r.depth = (int32_t)len;
    } else if (r.status == LV_SURF_BLOCKED) {
        r.depth = r.steps == 0 ? 0 : (int32_t)(((int64_t)h.num * len) / (int64_t)h.den);
    } else {
        const int64_t da = r.axis == 0 ? dx : r.axis == 1 ? dy : dz;
        const int64_t sg = da > 0 ? 1 : -1;
        const size_t at_b = (size_t)r.cell, at_a = surf_cell_a(g, qs, qe, r);
        const int32_t t = tsdf_crossing(S[at_a], W[at_a], S[at_b], W[at_b]);
        const int64_t ax = h.bx - (r.axis == 0 ? sg : 0), ay = h.by - (r.axis == 1 ? sg : 0), az = h.bz - (r.axis == 2 ? sg : 0);
        int64_t u = (256 * ax + 128 - qs[0]) * dx + (256 * ay + 128 - qs[1]) * dy + (256 * az + 128 - qs[2]) * dz;
        u += (da < 0 ? -da : da) * (int64_t)t;
        u = u < 0 ? 0 : (u > l2 ? l2 : u);
        r.t = t;
        r.depth = (int32_t)(u / len);   // (a step happened: len >= 1)
    }
}

// f32, unfused: the range of a depth in metres
LV_OCC_HD float surf_metres(float resolution, int32_t depth) { return resolution * ((float)depth / 256.0f); }

// ---- the normal at B = (bx, by, bz), a KNOWN cell: the gradient of phi = S / W by central differences over the KNOWN neighbours,
// one-sided (doubled) where only one is KNOWN; zeros when an axis has neither, or the gradient vanishes
LV_OCC_HD void surf_normal(const OccGrid& g, const int32_t* S, const int32_t* W, int32_t min_weight, int32_t bx, int32_t by, int32_t bz, float n[3]) {
    n[0] = n[1] = n[2] = 0.f;
    const size_t at = grid_at(g, bx, by, bz);
    const float phi_b = (float)S[at] / (float)W[at];
    const size_t stride[3] = {(size_t)1, (size_t)g.nx, (size_t)g.nx * (size_t)g.ny};
    const int32_t pos[3] = {bx, by, bz}, dim[3] = {g.nx, g.ny, g.nz};
    float grad[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool lo = pos[a] > 0 && W[at - stride[a]] >= min_weight;
        const bool hi = pos[a] + 1 < dim[a] && W[at + stride[a]] >= min_weight;
        if (!lo && !hi) return;
        const float phi_lo = lo ? (float)S[at - stride[a]] / (float)W[at - stride[a]] : 0.f;
        const float phi_hi = hi ? (float)S[at + stride[a]] / (float)W[at + stride[a]] : 0.f;
        grad[a] = lo && hi ? phi_hi - phi_lo : (hi ? 2.0f * (phi_hi - phi_b) : 2.0f * (phi_b - phi_lo));
    }
    const float norm = sqrtf((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
    if (!(norm > 0.f)) return;
    n[0] = grad[0] / norm;
    n[1] = grad[1] / norm;
    n[2] = grad[2] / norm;
}

// ---- the colour of a HIT: B's voxel colour if it has one, else A's, else 0, 0, 0, 0.  sums: the layer, or NULL without one
LV_OCC_HD uint32_t surf_colour(const uint32_t* sums, size_t at_b, size_t at_a) {
    if (!sums) return 0u;
    if (sums[4 * at_b + 3]) return colour_voxel(sums + 4 * at_b);
    if (sums[4 * at_a + 3]) return colour_voxel(sums + 4 * at_a);
    return 0u;
}

// One ray qs -> qe: the record, and where asked for the normal and the colour (zeros for everything but a HIT)
template <class States>
LV_OCC_HD void surf_cast_q(const OccGrid& g, const int32_t qs[3], const int32_t qe[3], int32_t min_weight, States& st, const int32_t* S,
                           const int32_t* W, const uint32_t* sums, bool want_normal, bool want_colour, lv_tsdf_ray_result& r, float n[3],
                           uint32_t& rgba) {
    SurfStop h;
    surf_walk(g, qs, qe, st, r, h);
    surf_depth(g, qs, qe, S, W, h, r);
    n[0] = n[1] = n[2] = 0.f;
    rgba = 0u;
    if (r.status != LV_SURF_HIT) return;
    if (want_normal) surf_normal(g, S, W, min_weight, h.bx, h.by, h.bz, n);
    if (want_colour) rgba = surf_colour(sums, (size_t)r.cell, surf_cell_a(g, qs, qe, r));
}

// One ray of lv_surf_raycast
template <class States>
LV_OCC_HD void surf_cast(const OccGrid& g, const float from[3], const float to[3], int32_t min_weight, States& st, const int32_t* S,
                         const int32_t* W, const uint32_t* sums, bool want_normal, bool want_colour, lv_tsdf_ray_result& r, float n[3],
                         uint32_t& rgba) {
    int32_t qs[3], qe[3];
    if (!ray_ends(g, from, to, qs, qe)) {
        surf_ignored(r);
        n[0] = n[1] = n[2] = 0.f;
        rgba = 0u;
        return;
    }
    surf_cast_q(g, qs, qe, min_weight, st, S, W, sums, want_normal, want_colour, r, n, rgba);
}

// lv_surf_raycast's and lv_surf_raycast_views' arguments against their limits, before the context: NULL when they hold
inline const char* surf_check_params(const lv_tsdf_ray_params* p) {
    if (!p) return "null params";
    if (p->min_weight < 1) return "min_weight: at least 1";
    return nullptr;
}

}  // namespace lv
