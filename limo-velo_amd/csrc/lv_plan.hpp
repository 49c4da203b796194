// lv_plan.hpp — the cost-to-go planner over the distance field (lv_occ_plan_*, include/limovelo_hip.h "Planner"; kernels and host
// side in lv_plan.hip).
//
// The first part is the rule as plain __host__ __device__ code: the integer square root, the cost byte of a cell, which moves are
// allowed (no corner cutting), the edge cost, one relaxation with its overflow rule and one step of the descent.  The kernels of
// lv_plan.hip run exactly these functions; tests/emu/plan_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and
// tests/test_plan_host.py holds them to tests/plan_ref.py.  No float enters after the quantisation of the goal and start points,
// and the potential is the unique fixpoint of plan_relax over the allowed moves: whatever order relaxations run in, the three agree
// on every cell.
//
// The functions that look at neighbours take the field through an accessor F with
//   uint32_t cost(int i, int j, int k)   the cost byte of a cell, 0 when it is blocked OR outside the field
//   uint32_t pot(int i, int j, int k)    P of a cell inside the field
// so that the same code reads global memory (PlanView), a workgroup's LDS tile (lv_plan.hip) and the emulator's vectors.
#pragma once

#include "lv_distance.hpp"

namespace lv {

constexpr uint32_t PLAN_UNREACHED = LV_PLAN_UNREACHED;
constexpr size_t PLAN_MAX_COST = 1025;                // entries of the cost table
constexpr size_t PLAN_MAX_GOALS = 65536;
constexpr int PLAN_MAX_CLEAR = 3 * 1023 * 1023;       // the largest finite s2 of a field
constexpr int PLAN_ROUNDS_PER_READ = 8;               // relaxation rounds launched between two reads of the round words

// The field's shape and placement as the kernels take them (a copy: the plan outlives the distance field it was built from)
struct PlanGrid {
    int nx, ny, nz;   // nz = 1 when planar
    int planar;
    int max_m;        // non-zero components a move may have: 1, 2 or 3
    float origin[3];
    float resolution;
};

// exact floor(sqrt(s)), s < 2^32
LV_OCC_HD uint32_t plan_isqrt(uint32_t s) {
    uint32_t r = 0;
    for (uint32_t b = 1u << 15; b; b >>= 1) {
        const uint32_t t = r | b;
        if ((uint64_t)t * t <= (uint64_t)s) r = t;
    }
    return r;
}

// c(v) from s2(v): 0 = blocked
LV_OCC_HD uint32_t plan_cell_cost(int32_t s, int min_clear_s2, const uint8_t* cost, int n_cost) {
    if (s < min_clear_s2) return 0;   // (obstacles, negative values and -FAR: min_clear_s2 >= 1)
    uint32_t t = (uint32_t)n_cost - 1u;
    if (s != DIST_FAR) {
        const uint32_t r = plan_isqrt((uint32_t)s);
        if (r < t) t = r;
    }
    return cost[t];
}

// 0 when the connectivity is none of 4, 6, 8, 18, 26
LV_OCC_HD int plan_max_m(int connectivity) {
    return (connectivity == 4 || connectivity == 6) ? 1 : (connectivity == 8 || connectivity == 18) ? 2 : connectivity == 26 ? 3 : 0;
}

LV_OCC_HD uint32_t plan_weight(int m) { return m == 1 ? 10u : m == 2 ? 14u : 17u; }

LV_OCC_HD uint32_t plan_edge(uint32_t cu, uint32_t cv, int m) { return plan_weight(m) * (cu + cv); }

// The offset of move mv = 0..26 in lexicographic order of (dz, dy, dx), each running -1, 0, 1; returns m (0 for mv = 13)
LV_OCC_HD int plan_move(int mv, int& dx, int& dy, int& dz) {
    dz = mv / 9 - 1;
    dy = (mv / 3) % 3 - 1;
    dx = mv % 3 - 1;
    return (dx != 0) + (dy != 0) + (dz != 0);
}

// The move (i, j, k) -> (i + dx, j + dy, k + dz): both ends and every cell reached by a proper non-empty subset of the non-zero
// components traversable.  Symmetric: the cells between are the same from either end.
template <class F>
LV_OCC_HD bool plan_move_allowed(const F& f, int i, int j, int k, int dx, int dy, int dz) {
    if (!f.cost(i, j, k) || !f.cost(i + dx, j + dy, k + dz)) return false;
    const int m = (dx != 0) + (dy != 0) + (dz != 0);
    if (m == 1) return true;
    if (dx && !f.cost(i + dx, j, k)) return false;
    if (dy && !f.cost(i, j + dy, k)) return false;
    if (dz && !f.cost(i, j, k + dz)) return false;
    if (m == 2) return true;
    return f.cost(i + dx, j + dy, k) && f.cost(i + dx, j, k + dz) && f.cost(i, j + dy, k + dz);
}

// What P(v) may be lowered to through u: P(u) + w * (c(u) + c(v)); a 64-bit sum that reaches 0xFFFFFFFF is dropped
LV_OCC_HD uint32_t plan_relax(uint32_t pu, uint32_t cu, uint32_t cv, uint32_t w) {
    if (pu == PLAN_UNREACHED) return PLAN_UNREACHED;
    const uint64_t s = (uint64_t)pu + (uint64_t)w * (uint64_t)(cu + cv);
    return s >= (uint64_t)PLAN_UNREACHED ? PLAN_UNREACHED : (uint32_t)s;
}

// One descent step from u = (i, j, k), P(u) finite and > 0: the first allowed move whose end v has P(v) + edge(u, v) == P(u).
// false: none (cannot happen on a finished potential)
template <class F>
LV_OCC_HD bool plan_next(const F& f, int max_m, bool planar, int& i, int& j, int& k) {
    const uint32_t cu = f.cost(i, j, k), pu = f.pot(i, j, k);
    for (int mv = planar ? 9 : 0; mv < (planar ? 18 : 27); ++mv) {
        int dx, dy, dz;
        const int m = plan_move(mv, dx, dy, dz);
        if (m == 0 || m > max_m || !plan_move_allowed(f, i, j, k, dx, dy, dz)) continue;
        const uint32_t pv = f.pot(i + dx, j + dy, k + dz);
        if (pv < pu && plan_relax(pv, f.cost(i + dx, j + dy, k + dz), cu, plan_weight(m)) == pu) {
            i += dx;
            j += dy;
            k += dz;
            return true;
        }
    }
    return false;
}

// The cell of a world point by the grid's one rule (planar: z is not used)
LV_OCC_HD bool plan_cell_of(const PlanGrid& g, const float p[3], int& i, int& j, int& k) {
    return grid_cell_of(g, g.origin, g.resolution, g.planar != 0, p, i, j, k);
}

// The finished (or growing) field in linear memory
struct PlanView {
    const uint8_t* c;
    const uint32_t* p;
    int nx, ny, nz;
    LV_OCC_HD size_t at(int i, int j, int k) const { return grid_at(*this, i, j, k); }
    LV_OCC_HD bool inside(int i, int j, int k) const { return grid_inside(*this, i, j, k); }
    LV_OCC_HD uint32_t cost(int i, int j, int k) const { return inside(i, j, k) ? c[at(i, j, k)] : 0u; }
    LV_OCC_HD uint32_t pot(int i, int j, int k) const { return p[at(i, j, k)]; }
};

enum : int { PLAN_PATH_OK = 0, PLAN_PATH_UNREACHED = 1, PLAN_PATH_BAD_START = 2 };

// One start point: its status and cost, and the walk to a cell with P = 0.  cells == NULL counts only; returns the path's length
// (0 unless the status is 0).  The walk is capped at the number of cells (P strictly decreases: it cannot get there).
LV_OCC_HD uint64_t plan_walk(const PlanGrid& g, const PlanView& f, const float p[3], int32_t* status, uint32_t* cost, int32_t* cells) {
    int i, j, k;
    *cost = PLAN_UNREACHED;
    if (!plan_cell_of(g, p, i, j, k) || !f.cost(i, j, k)) {
        *status = PLAN_PATH_BAD_START;
        return 0;
    }
    const uint32_t p0 = f.pot(i, j, k);
    if (p0 == PLAN_UNREACHED) {
        *status = PLAN_PATH_UNREACHED;
        return 0;
    }
    *status = PLAN_PATH_OK;
    *cost = p0;
    const uint64_t cap = grid_cells(g);
    uint64_t n = 0;
    for (;;) {
        if (cells) cells[n] = (int32_t)f.at(i, j, k);
        ++n;
        if (f.pot(i, j, k) == 0 || n >= cap) break;
        if (!plan_next(f, g.max_m, g.planar != 0, i, j, k)) break;
    }
    return n;
}

inline void default_plan_params(lv_plan_params* p) {
    if (!p) return;
    *p = lv_plan_params{};
    p->connectivity = 8;
    p->min_clear_s2 = 1;
}

// Everything that can be judged without a context: NULL when it holds, otherwise what is wrong (lv_occ_plan_build: LV_EINVAL)
inline const char* plan_check(const lv_plan_params* p, const uint8_t* cost, size_t n_cost, const void* goals, size_t stride, size_t n_goals) {
    if (!p) return "null params";
    if (!plan_max_m(p->connectivity)) return "connectivity: 4 or 8 (planar field), 6, 18 or 26 (3-D field)";
    if (p->min_clear_s2 < 1 || p->min_clear_s2 > PLAN_MAX_CLEAR) return "min_clear_s2: 1..3 * 1023^2";
    if (!cost) return "null cost table";
    if (n_cost < 1 || n_cost > PLAN_MAX_COST) return "n_cost: 1..1025";
    for (size_t t = 0; t < n_cost; ++t)
        if (cost[t] == 0) return "cost table: every entry 1..255";
    if (n_goals < 1 || n_goals > PLAN_MAX_GOALS) return "n_goals: 1..65536";
    if (!goals || stride < 12) return "bad goal array (null, or a stride below 12)";
    return nullptr;
}

// The connectivity against the field it is to run on: NULL when it suits
inline const char* plan_check_field(int connectivity, bool planar) {
    const bool flat = connectivity == 4 || connectivity == 8;
    if (planar && !flat) return "connectivity: a planar field takes 4 or 8";
    if (!planar && flat) return "connectivity: a 3-D field takes 6, 18 or 26";
    return nullptr;
}

// The plan of a context and the buffers of its calls.  Nothing is allocated before the first build().
struct PlanStore {
    bool built = false;
    int stale = 0;
    int32_t shift[3] = {0, 0, 0};   // the shift of the field it was built from
    int rounds = 0;
    lv_plan_params prm{};
    PlanGrid grid{};
    size_t n_cells = 0, n_tiles = 0;
    DevBuf<uint8_t> d_cost;          // the cost byte per cell, by grid_at
    DevBuf<uint32_t> d_pot;          // P
    DevBuf<uint32_t> d_active;       // 2 * n_tiles flags: the tiles of this round, of the next
    DevBuf<uint8_t> d_table;         // the cost table (PLAN_MAX_COST bytes)
    DevBuf<uint32_t> d_round;        // PLAN_ROUNDS_PER_READ words: round r of a batch lowered something
    PinBuf<uint32_t> h_round;
    Counters4 stats;
    PointStage pts;                  // goal and start points
    DevBuf<int32_t> d_status;        // per start
    DevBuf<uint32_t> d_pcost;
    DevBuf<unsigned long long> d_cnt;   // per start the path's length, one more entry of 0 (the scan's last offset is the total)
    DevBuf<unsigned long long> d_off;
    DevBuf<int32_t> d_cells;
    DevBuf<void> d_tmp;              // the scan's scratch

    int build(hipStream_t stream, const DistStore& dist, const lv_plan_params& p, const uint8_t* cost, size_t n_cost, const void* goals,
              size_t stride, size_t n_goals, uint64_t out[4]);
    int fetch(hipStream_t stream, uint32_t* potential, uint8_t* cell_cost);
    int paths(hipStream_t stream, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets, int32_t* cells,
              size_t capacity, size_t* total);
    void release();

   private:
    int stage(hipStream_t stream, const void* points, size_t stride, size_t n);
};

}  // namespace lv
