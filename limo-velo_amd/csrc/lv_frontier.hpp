// lv_frontier.hpp — frontier detection and ranking on the occupancy grid (lv_occ_frontier_*, include/limovelo_hip.h "Frontiers";
// kernels and host side in lv_frontier.hip).
//
// The first part is the rule as plain __host__ __device__ code: the state of a voxel or of a projected cell, the frontier
// predicate, the neighbour offsets of a connectivity, the key that orders the clusters, centre and rep, and the window a rank
// looks at.  The kernels of lv_frontier.hip run exactly these functions; tests/emu/frontier_emu.cpp compiles them with g++
// through tests/emu/hip/hip_runtime.h and tests/test_frontier_host.py holds them to tests/frontier_ref.py.  No float enters
// after the states are decided, so the three agree on every cell.
//
// The functions that look at neighbours take the field through an accessor F with
//   int state(int i, int j, int k)   FR_FREE, FR_OCCUPIED, FR_UNKNOWN or FR_OTHER of a cell, FR_OUTSIDE past the field's border
// so that the same code reads a workgroup's LDS tile (lv_frontier.hip) and the emulator's vectors.
// The components are joined by the lock-free union-find of lv_cluster.hpp (cl_find / cl_link / cl_root over cell indices).
#pragma once

#if !defined(__HIPCC__) && !defined(LV_CLUSTER_HOST_ONLY)
#define LV_CLUSTER_HOST_ONLY   // (g++: the sequential stand-ins of tests/emu/hip/hip_runtime.h)
#endif
#include "lv_cluster.hpp"
#include "lv_plan.hpp"

namespace lv {

constexpr int32_t FR_NONE = LV_FRONTIER_NONE;
constexpr int FR_MAX_REACH = 8;
constexpr int FR_MAX_MIN_SIZE = 1 << 28;

enum : int { FR_OTHER = 0, FR_FREE = 1, FR_OCCUPIED = 2, FR_UNKNOWN = 3, FR_OUTSIDE = 4 };

// The result's shape as the kernels take it
struct FrontierGrid {
    int nx, ny, nz;   // nz = 1 when planar
    int planar;
    int max_m;        // non-zero components a neighbour offset may have: 1, 2 or 3
};

// 3-D: FREE iff L <= l_free, OCCUPIED iff L >= l_occ, UNKNOWN iff L is NaN (which compares false twice)
LV_OCC_HD int fr_state_voxel(float L, float l_free, float l_occ) {
    return L != L ? FR_UNKNOWN : L >= l_occ ? FR_OCCUPIED : L <= l_free ? FR_FREE : FR_OTHER;
}

// planar: a value of lv_occ_project (grid_project_column)
LV_OCC_HD int fr_state_projected(int v) { return v == 100 ? FR_OCCUPIED : v == 0 ? FR_FREE : FR_UNKNOWN; }

// planar: column c of lv_occ_project over the clipped layers k0..k1
LV_OCC_HD int fr_state_column(const float* L, size_t plane, size_t c, int k0, int k1, float l_free, float l_occ) {
    return fr_state_projected(grid_project_column(L, plane, c, k0, k1, l_occ, l_free));
}

// A FREE cell with an UNKNOWN face neighbour inside the field (outside cells answer FR_OUTSIDE: the border is not unknown)
template <class F>
LV_OCC_HD bool fr_is_frontier(const F& f, bool planar, int i, int j, int k) {
    if (f.state(i, j, k) != FR_FREE) return false;
    if (f.state(i - 1, j, k) == FR_UNKNOWN || f.state(i + 1, j, k) == FR_UNKNOWN || f.state(i, j - 1, k) == FR_UNKNOWN ||
        f.state(i, j + 1, k) == FR_UNKNOWN)
        return true;
    return !planar && (f.state(i, j, k - 1) == FR_UNKNOWN || f.state(i, j, k + 1) == FR_UNKNOWN);
}

// Neighbour mv = 0..26 (plan_move's order) of a connectivity with max_m: its offset; false when the connectivity has no such
// neighbour.  The offsets with mv < 13 are the ones towards smaller cell indices: every adjacent pair is met once through them.
LV_OCC_HD bool fr_neighbour(int mv, int max_m, bool planar, int& dx, int& dy, int& dz) {
    const int m = plan_move(mv, dx, dy, dz);
    return m != 0 && m <= max_m && !(planar && dz != 0);
}

// Clusters are numbered by ascending key: size descending, then the smaller first member (lv_map_cluster's order)
LV_OCC_HD uint64_t fr_order_key(uint32_t size, uint32_t first) { return cl_order_key(size, first); }

// the centroid rounded half up, from the sum of one coordinate over `size` members
LV_OCC_HD int32_t fr_centre(uint64_t sum, uint32_t size) { return (int32_t)((2ull * sum + (uint64_t)size) / (2ull * (uint64_t)size)); }

// what a member bids to be rep: the least value wins (the squared distance to centre, then the smaller index)
LV_OCC_HD uint64_t fr_rep_key(const int32_t centre[3], int i, int j, int k, uint32_t cell) {
    const int64_t dx = i - centre[0], dy = j - centre[1], dz = k - centre[2];
    return ((uint64_t)(dx * dx + dy * dy + dz * dz) << 32) | (uint64_t)cell;
}

LV_OCC_HD void fr_cell_ijk(const FrontierGrid& g, uint32_t cell, int& i, int& j, int& k) { grid_ijk(g, cell, i, j, k); }

constexpr uint64_t FR_RANK_NONE = ~0ull;   // (LV_PLAN_UNREACHED << 32) | (uint32_t)-1: what rank reports without a reached cell

// What member (i, j, k) bids for its cluster's rank: the least (P << 32) | cell over the plan cells within Chebyshev distance
// `reach`, clipped to the field, unreached cells left out; FR_RANK_NONE when there is none
LV_OCC_HD uint64_t fr_rank_window(const FrontierGrid& g, const uint32_t* pot, int reach, int i, int j, int k) {
    const int i0 = i - reach < 0 ? 0 : i - reach, i1 = i + reach >= g.nx ? g.nx - 1 : i + reach;
    const int j0 = j - reach < 0 ? 0 : j - reach, j1 = j + reach >= g.ny ? g.ny - 1 : j + reach;
    const int k0 = g.planar ? 0 : (k - reach < 0 ? 0 : k - reach), k1 = g.planar ? 0 : (k + reach >= g.nz ? g.nz - 1 : k + reach);
    uint64_t best = FR_RANK_NONE;
    for (int c = k0; c <= k1; ++c)
        for (int b = j0; b <= j1; ++b) {
            const size_t row = grid_at(g, 0, b, c);
            for (int a = i0; a <= i1; ++a) {
                const uint32_t p = pot[row + (size_t)a];
                if (p == PLAN_UNREACHED) continue;
                const uint64_t bid = ((uint64_t)p << 32) | (uint64_t)(row + (size_t)a);
                best = bid < best ? bid : best;
            }
        }
    return best;
}

// The record of a cluster from what was accumulated over its members (rep is found afterwards)
LV_OCC_HD void fr_cluster_record(lv_frontier_cluster& c, uint32_t size, uint32_t first, const uint64_t sum[3], const int32_t lo[3], const int32_t hi[3]) {
    c.size = (int32_t)size;
    c.first = (int32_t)first;
    c.rep = FR_NONE;
    for (int a = 0; a < 3; ++a) {
        c.sum[a] = sum[a];
        c.lo[a] = lo[a];
        c.hi[a] = hi[a];
        c.centre[a] = fr_centre(sum[a], size);
    }
}

inline void default_frontier_params(lv_frontier_params* p) {
    if (!p) return;
    *p = lv_frontier_params{};
    p->connectivity = 26;
    p->min_size = 1;
}

// The parameters against their limits: NULL when they hold, otherwise what is wrong (lv_occ_frontier_build: LV_EINVAL)
inline const char* fr_check_params(const lv_frontier_params* p) {
    if (!p) return "null params";
    const bool flat = p->connectivity == 4 || p->connectivity == 8;
    if (!plan_max_m(p->connectivity)) return "connectivity: 4 or 8 (planar), 6, 18 or 26 (3-D)";
    if (p->planar && !flat) return "connectivity: a planar result takes 4 or 8";
    if (!p->planar && flat) return "connectivity: a 3-D result takes 6, 18 or 26";
    if (p->min_size < 1 || p->min_size > FR_MAX_MIN_SIZE) return "min_size: 1..2^28";
    if (p->planar && p->k_lo > p->k_hi) return "planar layers: k_lo <= k_hi";
    return nullptr;
}

// The frontier of a context and the buffers of its calls.  Nothing is allocated before the first build(); only d_labels and the
// per-cluster records outlive it, the per-cell scratch goes when the build is through.
struct FrontierStore {
    bool built = false;
    int stale = 0;
    int32_t shift[3] = {0, 0, 0};   // the grid's accumulated shift at the build: lv_occ_frontier_rank pairs cells of one shift only
    lv_frontier_params prm{};
    FrontierGrid grid{};
    size_t n_cells = 0, n_clusters = 0;
    DevBuf<int32_t> d_labels;            // the result: one label per cell
    DevBuf<uint32_t> d_parent;           // scratch: the union-find over cell indices (CL_NONE where no frontier); at a root, later, its dense number
    DevBuf<uint32_t> d_root;             // scratch: every frontier cell's root
    DevBuf<uint32_t> d_first;            // per root (dense number): its cell
    DevBuf<uint32_t> d_size;
    DevBuf<unsigned long long> d_sum;    // 3 per root
    DevBuf<int32_t> d_lohi;              // lo[3] of every root, then hi[3] of every root
    DevBuf<uint64_t> d_key, d_key2;      // the roots' order keys and their sorted copy
    DevBuf<uint32_t> d_idx, d_idx2;      // dense numbers, and in cluster order
    DevBuf<int32_t> d_number;            // per root: its cluster's number, or FR_NONE
    DevBuf<void> d_tmp;                  // hipcub scratch
    DevBuf<lv_frontier_cluster> d_clusters;
    DevBuf<unsigned long long> d_best;   // per cluster: the rep bids, then lv_occ_frontier_rank's
    PinBuf<unsigned long long> h_best;
    DevBuf<unsigned long long> d_cnt;    // 4 words: roots, numbers handed out, clusters reported
    PinBuf<unsigned long long> h_cnt;
    Counters4 stats;

    int build(hipStream_t stream, const OccStore& occ, const lv_frontier_params& p, uint64_t out[4]);
    int fetch(hipStream_t stream, int32_t* labels);
    int clusters(hipStream_t stream, lv_frontier_cluster* out);
    int rank(hipStream_t stream, const PlanStore& plan, int reach, uint32_t* best_p, int32_t* best_cell);
    void release();

   private:
    void drop_scratch();
};

}  // namespace lv
