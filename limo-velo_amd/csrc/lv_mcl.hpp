// lv_mcl.hpp — Monte Carlo localisation on the distance field: the likelihood-field weight of K poses under one scan
// (lv_occ_mcl_weigh, include/limovelo_hip.h "Localisation"; kernel and host side in lv_mcl.hip).
//
// The first part is the rule as plain __host__ __device__ code: the limits, a beam's cost, a particle's
// fold over its beams, and the key `best` is chosen by.  The kernel of lv_mcl.hip runs exactly these functions;
// tests/emu/occ_mcl_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_occ_mcl_host.py holds them
// to tests/mcl_ref.py.  Every f32 operation stands alone (-ffp-contract=off) and the sine and cosine are lv_sincos.hpp's one
// polynomial, so the three agree on the cell of every end point; everything after the cell is integer arithmetic.
//
// mcl_particle is written for a GROUP of lanes that serve one particle: every lane computes the sine and cosine itself (the same
// operations give the same bits, nothing is broadcast), lane g takes the beams g, g + stride, ..., and the particle's sum and
// count are folds of the lanes'.  What a group is comes in through the Lanes argument:
//   int first(), int stride()              the beams this lane takes
//   void beam(beams, b, ex, ey, ez)        beam b
//   uint32_t cost(table, idx)              table[idx] (the device: from LDS)
//   uint64_t sum(uint64_t v)               the group's sum; every lane of the group calls it once per particle
//   uint32_t count(uint32_t v)             likewise for the beams that have a cell
// The host emulation is a group of one lane.
#pragma once

#include "lv_rollout.hpp"

namespace lv {

constexpr size_t MCL_MAX_K = (size_t)1 << 20;
constexpr size_t MCL_MAX_B = 65536;
constexpr size_t MCL_MAX_PAIRS = (size_t)1 << 30;   // K * B
constexpr size_t MCL_MAX_TABLE = 4096;              // 16 KiB of LDS
constexpr uint32_t MCL_MAX_COST = 1u << 24;         // of a table entry and of out_cost: a score stays below 2^40
constexpr uint64_t MCL_NO_SCORE = 0xFFFFFFFFFFFFFFFFull;
constexpr int MCL_KEY_SHIFT = 20;                   // key = (score << 20) | index: 60 bits

// What a call reads: the field last built
struct MclView {
    GridDims field;   // nz = 1 when planar
    float origin[3];
    float resolution;
    int planar;
    const int32_t* s2;
};

// the table entry of a field value: FAR goes to the last entry, the inside of a signed field (and an obstacle) to entry 0
LV_OCC_HD uint32_t mcl_index(int32_t s2, uint32_t n_table) { return s2 <= 0 ? 0u : ((uint32_t)s2 < n_table - 1u ? (uint32_t)s2 : n_table - 1u); }

// The cell of beam (ex, ey, ez) seen from the pose (x, y, z) with the heading's (sn, cs); false: the end point has no cell
LV_OCC_HD bool mcl_beam_cell(const MclView& f, float x, float y, float z, float sn, float cs, float ex, float ey, float ez, size_t& at) {
    const float p[3] = {x + (cs * ex - sn * ey), y + (sn * ex + cs * ey), z + ez};
    int i, j, k;
    if (!grid_cell_of(f.field, f.origin, f.resolution, f.planar != 0, p, i, j, k)) return false;
    at = grid_at(f.field, i, j, k);
    return true;
}

// One particle.  live: false for a lane that has no particle and only keeps its group's folds company.  pose: (x, y, z, th).
// In every lane of the group: n_in, and the score (MCL_NO_SCORE: not eligible).
template <class Lanes>
LV_OCC_HD void mcl_particle(const MclView& f, const lv_mcl_params& r, const float* pose, const float* beams, int B, const uint32_t* table,
                            uint32_t n_table, bool live, const Lanes& lanes, uint64_t& score, uint32_t& n_in) {
    uint64_t sum = 0;
    uint32_t cnt = 0;
    bool usable = false;
    if (live) {
        const float x = pose[0], y = pose[1], z = pose[2], th = pose[3];
        usable = rollout_usable(th);   // (fabsf(th) < 2^20: below it sincos_f32's (int)k is defined)
        if (usable) {
            float sn, cs;
            sincos_f32(th, sn, cs);
            for (int b = lanes.first(); b < B; b += lanes.stride()) {
                float ex, ey, ez;
                lanes.beam(beams, b, ex, ey, ez);
                size_t at;
                if (mcl_beam_cell(f, x, y, z, sn, cs, ex, ey, ez, at)) {
                    sum += (uint64_t)lanes.cost(table, mcl_index(f.s2[at], n_table));
                    ++cnt;
                } else {
                    sum += (uint64_t)r.out_cost;
                }
            }
        }
    }
    sum = lanes.sum(sum);
    cnt = lanes.count(cnt);
    n_in = cnt;
    score = (!usable || (int64_t)cnt < (int64_t)r.min_inside) ? MCL_NO_SCORE : sum;
}

// `best` is the least key: (score, index) in one word, MCL_NO_SCORE for a particle that is not eligible
LV_OCC_HD uint64_t mcl_key(uint64_t score, uint32_t index) { return score == MCL_NO_SCORE ? MCL_NO_SCORE : (score << MCL_KEY_SHIFT) | (uint64_t)index; }

LV_OCC_HD void mcl_best_of(uint64_t key, int64_t best[2]) {
    if (key == MCL_NO_SCORE) {
        best[0] = best[1] = -1;
        return;
    }
    best[0] = (int64_t)(key & (((uint64_t)1 << MCL_KEY_SHIFT) - 1u));
    best[1] = (int64_t)(key >> MCL_KEY_SHIFT);
}

// The group of one lane (the host emulation, the timing's CPU baseline)
struct MclOneLane {
    LV_OCC_HD int first() const { return 0; }
    LV_OCC_HD int stride() const { return 1; }
    LV_OCC_HD void beam(const float* beams, int b, float& ex, float& ey, float& ez) const {
        ex = beams[3 * b];
        ey = beams[3 * b + 1];
        ez = beams[3 * b + 2];
    }
    LV_OCC_HD uint32_t cost(const uint32_t* table, uint32_t idx) const { return table[idx]; }
    LV_OCC_HD uint64_t sum(uint64_t v) const { return v; }
    LV_OCC_HD uint32_t count(uint32_t v) const { return v; }
};

inline void default_mcl_params(lv_mcl_params* p) {
    if (!p) return;
    *p = lv_mcl_params{};
    p->out_cost = 0;
    p->min_inside = 1;
}

// Everything that can be judged without a context: NULL when it holds, otherwise what is wrong (lv_occ_mcl_weigh: LV_EINVAL)
inline const char* mcl_check(const lv_mcl_params* p, const float* poses, size_t K, const float* beams, size_t B, const uint32_t* table, size_t n_table,
                             const void* score, const void* n_in, const void* best) {
    if (!p) return "null params";
    if (K > MCL_MAX_K) return "K: 0..2^20";
    if (B < 1 || B > MCL_MAX_B) return "B: 1..65536";
    if (K * B > MCL_MAX_PAIRS) return "K * B: at most 2^30";
    if (n_table < 1 || n_table > MCL_MAX_TABLE) return "n_table: 1..4096";
    if (p->out_cost > MCL_MAX_COST) return "out_cost: 0..2^24";
    if (p->min_inside < 0 || (size_t)p->min_inside > B) return "min_inside: 0..B";
    if (K && !poses) return "null poses with K > 0";
    if (!beams) return "null beams";
    if (!table) return "null table";
    for (size_t t = 0; t < n_table; ++t)
        if (table[t] > MCL_MAX_COST) return "table: every entry 0..2^24";
    if (!score && !n_in && !best) return "score, n_in and best are all null";
    return nullptr;
}

// the lanes that serve one particle: the power of two >= B, at most 64
inline int mcl_group(size_t B) {
    int g = 1;
    while ((size_t)g < B && g < 64) g *= 2;
    return g;
}

// The buffers of a context's calls.  Nothing is allocated before the first call.
struct MclStore {
    PinBuf<uint32_t> h_in;                   // the table (MCL_MAX_TABLE words), then the beams, then the poses, as 32-bit words
    DevBuf<uint32_t> d_in;
    DevBuf<unsigned long long> d_score;      // K scores, then the least key of the call
    DevBuf<uint32_t> d_n_in;
    PinBuf<unsigned long long> h_best;       // the key as it goes up (all ones) and as it comes back

    int run(hipStream_t stream, const DistStore& dist, const lv_mcl_params& p, const float* poses, size_t K, const float* beams, size_t B,
            const uint32_t* table, size_t n_table, uint64_t* score, uint32_t* n_in, int64_t* best);
    void release();
};

}  // namespace lv
