// lv_ray.hpp — ray casting and view gain on the occupancy grid (lv_occ_raycast, lv_occ_view_gain, include/limovelo_hip.h "Ray
// casting"; kernels and host side in lv_ray.hip).
//
// The first part is the rule as plain __host__ __device__ code without atomics: the packed cell states, the two quantisations of a
// ray's ends, and the walk that READS the grid.  The walk itself is lv_occupancy.hpp's (occ_walk_init / occ_walk_step, unchanged);
// the cell states are lv_frontier.hpp's (fr_state_voxel).  The kernels of lv_ray.hip run exactly these functions;
// tests/emu/occ_ray_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_occ_ray_host.py holds them to
// tests/occ_ray_ref.py.  After the quantisation and the states every step is integer arithmetic, so the three agree on every field.
#pragma once

#include "lv_frontier.hpp"
#include "lv_occupancy.hpp"

namespace lv {

constexpr uint64_t RAY_MAX_N = 0x7FFFFFFFull;   // lv_occ_raycast: n below this

inline void default_ray_params(lv_ray_params* p) {
    if (!p) return;
    *p = lv_ray_params{};
}

// ---- the packed states: 2 bits per voxel (FR_OTHER, FR_FREE, FR_OCCUPIED, FR_UNKNOWN = 0..3), 16 consecutive x per word, every
// x row starting a word: voxel (i, j, k) is bits 2 * (i & 15) .. + 1 of word (k * ny + j) * wx16 + (i >> 4)
LV_OCC_HD int ray_wx16(int nx) { return (nx + 15) / 16; }
template <class G>
LV_OCC_HD uint32_t ray_word_of(const G& g, int i, int j, int k) {
    return ((uint32_t)k * (uint32_t)g.ny + (uint32_t)j) * (uint32_t)ray_wx16(g.nx) + ((uint32_t)i >> 4);
}
LV_OCC_HD uint32_t ray_pack(int state, int i) { return (uint32_t)state << (2 * (i & 15)); }
LV_OCC_HD int ray_unpack(uint32_t word, int i) { return (int)((word >> (2 * (i & 15))) & 3u); }

// What a walk reads the states through: the packed volume, with the word it stands in kept (a register on the device; a lane
// loads again only when its walk leaves the word, as occ_march_kernel keeps its bitmap word)
struct RayStates {
    const uint32_t* words;
    uint32_t cur, val;
    LV_OCC_HD explicit RayStates(const uint32_t* w) : words(w), cur(0xFFFFFFFFu), val(0) {}
    // (i, j, k) inside the grid
    LV_OCC_HD int state(const OccGrid& g, int i, int j, int k) {
        const uint32_t word = ray_word_of(g, i, j, k);
        if (word != cur) {
            cur = word;
            val = words[word];
        }
        return ray_unpack(val, i);
    }
};

// ---- the ends of a ray.  `from` as a view's sensor origin (occ_view_origin), `to` as a return's world point (occ_quant):
// the bounds under which every product of the walk fits in int64
LV_OCC_HD bool ray_ends(const OccGrid& g, const float from[3], const float to[3], int32_t qs[3], int32_t qe[3]) {
    if (!occ_view_origin(g, from, qs)) return false;
    for (int a = 0; a < 3; ++a)
        if (!occ_quant(to[a], g.origin[a], g.resolution, qe[a])) return false;
    return true;
}

LV_OCC_HD void ray_ignored(lv_ray_result& r) {
    r.status = LV_RAY_IGNORED;
    r.cell = -1;
    r.steps = r.axis = r.n_free = r.n_unknown = r.num = r.den = 0;
}

// ---- the walk from qs to qe over the cells c_0 = vs .. c_S = ve.  st: the states (state(g, i, j, k) of an in-grid cell);
// seen(i, j, k) is called for every in-grid cell before the stop (all of them when the ray does not stop).  Leaving once
// occ_walk_left holds changes nothing: no later cell, ve included, is in the grid.
template <class States, class Seen>
LV_OCC_HD void ray_walk(const OccGrid& g, const int32_t qs[3], const int32_t qe[3], bool stop_unknown, States& st, Seen& seen, lv_ray_result& r) {
    OccWalk w;
    occ_walk_init(w, qs, qe);
    const int32_t total = w.rx + w.ry + w.rz;
    int32_t steps = 0, axis = -1, num = 0, den = 1, n_free = 0, n_unknown = 0;
    for (;;) {
        if (occ_in_grid(g, w.vx, w.vy, w.vz)) {
            const int s = st.state(g, w.vx, w.vy, w.vz);
            if (s == FR_OCCUPIED || (s == FR_UNKNOWN && stop_unknown)) {
                r.status = LV_RAY_STOPPED;
                r.cell = (int32_t)grid_at(g, w.vx, w.vy, w.vz);
                r.steps = steps; r.axis = axis; r.n_free = n_free; r.n_unknown = n_unknown; r.num = num; r.den = den;
                return;
            }
            n_free += s == FR_FREE;
            n_unknown += s == FR_UNKNOWN;
            seen(w.vx, w.vy, w.vz);
        } else if (occ_walk_left(g, w)) {
            break;
        }
        if (occ_walk_done(w)) break;
        const int32_t nx = w.nx, ny = w.ny, nz = w.nz;   // n_a as it stands BEFORE the step adds 256
        axis = occ_walk_step(w);
        num = axis == 0 ? nx : axis == 1 ? ny : nz;
        den = axis == 0 ? w.ax : axis == 1 ? w.ay : w.az;
        ++steps;
    }
    r.status = LV_RAY_CLEAR;
    r.cell = occ_in_grid(g, w.ex, w.ey, w.ez) ? (int32_t)grid_at(g, w.ex, w.ey, w.ez) : -1;
    r.steps = total; r.axis = -1; r.n_free = n_free; r.n_unknown = n_unknown; r.num = 1; r.den = 1;
}

struct RaySeenNothing {
    LV_OCC_HD void operator()(int, int, int) const {}
};

// One ray of lv_occ_raycast
template <class States>
LV_OCC_HD void ray_cast(const OccGrid& g, const float from[3], const float to[3], bool stop_unknown, States& st, lv_ray_result& r) {
    int32_t qs[3], qe[3];
    if (!ray_ends(g, from, to, qs, qe)) {
        ray_ignored(r);
        return;
    }
    RaySeenNothing seen;
    ray_walk(g, qs, qe, stop_unknown, st, seen, r);
}

// The store of a context.  Nothing is allocated before the first call; the packed states are built by the first call after the
// grid changed (`packed` false).
struct RayStore {
    bool packed = false;
    DevBuf<uint32_t> d_states;             // the packed states
    PointStage pts;                        // lv_occ_raycast: every `from`, then every `to`; lv_occ_view_gain: every view's returns
    DevBuf<lv_ray_result> d_res;
    DevBuf<unsigned long long> d_gain;     // 4 counters per view (Counters4 holds one call's four; a gain call has 32 views' worth)
    PinBuf<unsigned long long> h_gain;

    int raycast(hipStream_t stream, OccStore& occ, const lv_ray_params& p, const void* from, size_t from_stride, const void* to, size_t to_stride,
                size_t n, lv_ray_result* out);
    int view_gain(hipStream_t stream, OccStore& occ, const lv_view* views, size_t n_views, uint64_t* gain);
    void release();

   private:
    int classify(hipStream_t stream, OccStore& occ);
};

}  // namespace lv
