// lv_lattice.hpp — the state-lattice planner for car-like robots (lv_occ_lattice_*, include/limovelo_hip.h "Lattice planner";
// kernels and host side in lv_lattice.hip).
//
// The first part is the rule as plain __host__ __device__ code: the check of the caller's table of motion primitives, which
// primitive is allowed from which cell, the edge cost, one relaxation with its overflow rule, one step of the descent and the walk
// of a start.  The kernels of lv_lattice.hip run exactly these functions; tests/emu/lattice_emu.cpp compiles them with g++
// through tests/emu/hip/hip_runtime.h and tests/test_lattice_host.py holds them to tests/lattice_ref.py.  No float enters after
// the quantisation of the goal and start points, and the potential is the unique fixpoint of lat_relax over the allowed
// primitives (every edge costs at least 2): whatever order relaxations run in, all agree on every state.
//
// A state is (i, j, h): a cell of the planar plan and a heading bin.  Edges are DIRECTED: a state lowers itself from its
// successors.  The functions that look at cells take the lattice through an accessor F with
//   uint32_t cost(int i, int j)        the cost byte of a cell, 0 when it is blocked OR outside the grid
//   uint32_t pot(int i, int j, int h)  V of a state whose cell is inside the grid
// so that the same code reads global memory (LatView), a workgroup's LDS box (lv_lattice.hip) and the emulator's vectors.
#pragma once

#include "lv_plan.hpp"

namespace lv {

constexpr uint32_t LAT_UNREACHED = LV_LATTICE_UNREACHED;
constexpr int LAT_MAX_H = 16, LAT_MAX_P = 16;
constexpr int LAT_REACH = LV_LATTICE_REACH;
constexpr int LAT_MAX_SWEEP = LV_LATTICE_MAX_SWEEP;
constexpr uint32_t LAT_MAX_PENALTY = 1u << 24;
constexpr size_t LAT_MAX_STATES = (size_t)1 << 28;
constexpr size_t LAT_MAX_GOALS = 65536;
constexpr size_t LAT_NO_RECORD = ~(size_t)0;
static_assert(sizeof(lv_lattice_prim) == 32, "a primitive is 32 bytes");

// The plan's shape and placement as the kernels take them (a copy: the lattice outlives the plan it was built from).  nz = 1:
// the grid helpers of lv_grid.hpp number its cells.
struct LatGrid {
    int nx, ny, nz;
    int H, P;
    float origin[3];
    float resolution;
};

// the linear index of state (i, j, h)
template <class G>
LV_OCC_HD size_t lat_at(const G& g, int i, int j, int h) {
    return ((size_t)h * (size_t)g.ny + (size_t)j) * (size_t)g.nx + (size_t)i;
}

// One record of the table, as primitive of heading h among H: NULL when it holds, otherwise what is wrong with it
LV_OCC_HD const char* lat_check_prim(const lv_lattice_prim& r, int h, int H) {
    if (r.reserved != 0) return "reserved must be 0";
    if (r.di < -LAT_REACH || r.di > LAT_REACH || r.dj < -LAT_REACH || r.dj > LAT_REACH) return "di, dj: each within +-LV_LATTICE_REACH";
    if ((int)r.h_to >= H) return "h_to: 0..H-1";
    if (r.n_sweep > LAT_MAX_SWEEP) return "n_sweep: 0..LV_LATTICE_MAX_SWEEP";
    if (r.penalty > LAT_MAX_PENALTY) return "penalty: at most 2^24";
    for (int s = 0; s < LAT_MAX_SWEEP; ++s) {
        const int a = r.sweep[s][0], b = r.sweep[s][1];
        if (a < -LAT_REACH || a > LAT_REACH || b < -LAT_REACH || b > LAT_REACH) return "sweep: each offset within +-LV_LATTICE_REACH";
        if (s >= (int)r.n_sweep && (a != 0 || b != 0)) return "sweep: unused entries must be 0";
    }
    if (r.length != 0 && r.di == 0 && r.dj == 0 && (int)r.h_to == h) return "a self loop (di == dj == 0 and h_to == h)";
    return nullptr;
}

// The largest |offset| of the table's non-empty records: how far a primitive's end or sweep cell lies from its start
inline int lat_reach_of(const lv_lattice_prim* prims, size_t n) {
    int reach = 0;
    const auto up = [&](int v) { v = v < 0 ? -v : v; reach = v > reach ? v : reach; };
    for (size_t r = 0; r < n; ++r) {
        if (!prims[r].length) continue;
        up(prims[r].di);
        up(prims[r].dj);
        for (int s = 0; s < (int)prims[r].n_sweep; ++s) { up(prims[r].sweep[s][0]); up(prims[r].sweep[s][1]); }
    }
    return reach;
}

// Primitive r from cell (i, j): the start cell, the end cell and every sweep cell inside the grid and traversable
template <class F>
LV_OCC_HD bool lat_prim_allowed(const F& f, const lv_lattice_prim& r, int i, int j) {
    if (!r.length || !f.cost(i, j) || !f.cost(i + r.di, j + r.dj)) return false;
    for (int s = 0; s < (int)r.n_sweep; ++s)
        if (!f.cost(i + r.sweep[s][0], j + r.sweep[s][1])) return false;
    return true;
}

// length * (c(u) + c(v)) + penalty: at least 2, below 2^26
LV_OCC_HD uint32_t lat_edge(uint32_t cu, uint32_t cv, uint32_t length, uint32_t penalty) { return length * (cu + cv) + penalty; }

// What V(u) may be lowered to through its successor v: V(v) + edge; a 64-bit sum that reaches 0xFFFFFFFF is dropped
LV_OCC_HD uint32_t lat_relax(uint32_t pv, uint32_t edge) {
    if (pv == LAT_UNREACHED) return LAT_UNREACHED;
    const uint64_t s = (uint64_t)pv + (uint64_t)edge;
    return s >= (uint64_t)LAT_UNREACHED ? LAT_UNREACHED : (uint32_t)s;
}

// One descent step from u = (i, j, h), V(u) finite and > 0: the first non-empty allowed primitive whose end v has
// V(v) + edge(u, v) == V(u).  Returns its number, -1: none (cannot happen on a finished potential)
template <class F>
LV_OCC_HD int lat_next(const F& f, const lv_lattice_prim* prims, int P, int& i, int& j, int& h) {
    const uint32_t cu = f.cost(i, j), vu = f.pot(i, j, h);
    for (int p = 0; p < P; ++p) {
        const lv_lattice_prim& r = prims[h * P + p];
        if (!lat_prim_allowed(f, r, i, j)) continue;
        const int vi = i + r.di, vj = j + r.dj;
        const uint32_t vv = f.pot(vi, vj, r.h_to);
        if (vv < vu && lat_relax(vv, lat_edge(cu, f.cost(vi, vj), r.length, r.penalty)) == vu) {
            i = vi;
            j = vj;
            h = r.h_to;
            return p;
        }
    }
    return -1;
}

// The cell of a world point by the grid's one rule (z is not used)
LV_OCC_HD bool lat_cell_of(const LatGrid& g, const float p[3], int& i, int& j) {
    int k;
    return grid_cell_of(g, g.origin, g.resolution, true, p, i, j, k);
}

// The finished (or growing) lattice in linear memory
struct LatView {
    const uint8_t* c;
    const uint32_t* v;
    int nx, ny, nz;
    LV_OCC_HD uint32_t cost(int i, int j) const { return grid_inside(*this, i, j, 0) ? c[grid_at(*this, i, j, 0)] : 0u; }
    LV_OCC_HD uint32_t pot(int i, int j, int h) const { return v[lat_at(*this, i, j, h)]; }
};

enum : int { LAT_PATH_OK = 0, LAT_PATH_UNREACHED = 1, LAT_PATH_BAD_START = 2 };

// One start record (x, y, z, h; h = -1: the heading with the least V at that cell, ties to the smaller h): its status and cost,
// and the walk to a state with V = 0.  states == NULL counts only; returns the path's length (0 unless the status is 0).  taken
// (may be NULL) gets the primitive out of each state, 255 at the last.  The walk is capped at the number of states (V strictly
// decreases: it cannot get there).
LV_OCC_HD uint64_t lat_walk(const LatGrid& g, const LatView& f, const lv_lattice_prim* prims, const float p[3], int32_t h0, int32_t* status,
                            uint32_t* cost, int32_t* states, uint8_t* taken) {
    int i, j;
    *cost = LAT_UNREACHED;
    if (!lat_cell_of(g, p, i, j) || !f.cost(i, j) || h0 < -1 || h0 >= g.H) {
        *status = LAT_PATH_BAD_START;
        return 0;
    }
    int h = h0;
    if (h0 < 0) {
        h = 0;
        for (int t = 1; t < g.H; ++t)
            if (f.pot(i, j, t) < f.pot(i, j, h)) h = t;
    }
    const uint32_t v0 = f.pot(i, j, h);
    if (v0 == LAT_UNREACHED) {
        *status = LAT_PATH_UNREACHED;
        return 0;
    }
    *status = LAT_PATH_OK;
    *cost = v0;
    const uint64_t cap = (uint64_t)g.nx * (uint64_t)g.ny * (uint64_t)g.H;
    uint64_t n = 0;
    for (;;) {
        const size_t at = lat_at(g, i, j, h);
        if (states) states[n] = (int32_t)at;
        const bool last = f.pot(i, j, h) == 0 || n + 1 >= cap;
        const int p_taken = last ? -1 : lat_next(f, prims, g.P, i, j, h);
        if (states && taken) taken[n] = p_taken < 0 ? (uint8_t)255 : (uint8_t)p_taken;
        ++n;
        if (p_taken < 0) break;
    }
    return n;
}

inline void default_lattice_params(lv_lattice_params* p) {
    if (!p) return;
    *p = lv_lattice_params{};
    p->H = 16;
    p->P = 3;
}

// Everything that can be judged without a context: NULL when it holds, otherwise what is wrong (lv_occ_lattice_build:
// LV_EINVAL).  *record: the record the complaint is about, LAT_NO_RECORD when it is about none.
inline const char* lattice_check(const lv_lattice_params* p, const lv_lattice_prim* prims, size_t n_prims, const void* goals, size_t stride,
                                 size_t n_goals, size_t* record) {
    *record = LAT_NO_RECORD;
    if (!p) return "null params";
    if (p->H < 1 || p->H > LAT_MAX_H) return "H: 1..16";
    if (p->P < 1 || p->P > LAT_MAX_P) return "P: 1..16";
    if (!prims) return "null primitive table";
    if (n_prims != (size_t)p->H * (size_t)p->P) return "n_prims: H * P records";
    bool any = false;
    for (size_t r = 0; r < n_prims; ++r) {
        if (const char* why = lat_check_prim(prims[r], (int)(r / (size_t)p->P), p->H)) {
            *record = r;
            return why;
        }
        any = any || prims[r].length != 0;
    }
    if (!any) return "the table has no non-empty record (every length is 0)";
    if (n_goals < 1 || n_goals > LAT_MAX_GOALS) return "n_goals: 1..65536";
    if (!goals || stride < 16) return "bad goal array (null, or a stride below 16)";
    return nullptr;
}

// The lattice of a context and the buffers of its calls.  Nothing is allocated before the first build().
struct LatticeStore {
    bool built = false;
    int stale = 0;
    int32_t shift[3] = {0, 0, 0};   // the shift of the plan it was built from
    int rounds = 0, tile = 0, reach = 0;
    lv_lattice_params prm{};
    LatGrid grid{};
    size_t n_cells = 0, n_states = 0, n_tiles = 0;
    DevBuf<uint8_t> d_cost;             // the plan's cost byte per cell, by grid_at
    DevBuf<uint32_t> d_V;               // V per state, by lat_at
    DevBuf<uint32_t> d_active;          // 2 * n_tiles flags: the tiles of this round, of the next
    DevBuf<lv_lattice_prim> d_prims;    // the table, H * P records
    DevBuf<uint32_t> d_round;           // PLAN_ROUNDS_PER_READ words: round r of a batch lowered something
    PinBuf<uint32_t> h_round;
    Counters4 stats;
    PinBuf<uint32_t> h_rec;             // goal and start records: 4 words each (x, y, z, h)
    DevBuf<uint32_t> d_rec;
    DevBuf<int32_t> d_status;           // per start
    DevBuf<uint32_t> d_pcost;
    DevBuf<unsigned long long> d_cnt;   // per start the path's length, one more entry of 0 (the scan's last offset is the total)
    DevBuf<unsigned long long> d_off;
    DevBuf<int32_t> d_states;
    DevBuf<uint8_t> d_taken;
    DevBuf<void> d_tmp;                 // the scan's scratch

    int build(hipStream_t stream, const PlanStore& plan, const lv_lattice_params& p, const lv_lattice_prim* prims, const void* goals, size_t stride,
              size_t n_goals, uint64_t out[4]);
    int fetch(hipStream_t stream, uint32_t* V);
    int paths(hipStream_t stream, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets, int32_t* states,
              uint8_t* prims_taken, size_t capacity, size_t* total);
    // (inline: lv_occ_configure and lv_destroy call it whether or not a lattice was ever built; a buffer never filled frees nothing)
    void release() {
        d_cost.release(); d_V.release(); d_active.release(); d_prims.release(); d_round.release(); h_round.release(); stats.release();
        h_rec.release(); d_rec.release(); d_status.release(); d_pcost.release(); d_cnt.release(); d_off.release(); d_states.release();
        d_taken.release(); d_tmp.release();
        *this = LatticeStore();
    }
};

}  // namespace lv
