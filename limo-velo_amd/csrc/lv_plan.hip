// lv_plan.hip — the cost-to-go planner over the distance field (include/limovelo_hip.h "Planner"; the rule's code is lv_plan.hpp).
//
// A build is a block-based label-correcting solver (the layout of the fast iterative method) on the context's stream:
//   plan_cost_kernel    one lane per cell: the cost byte from s2 and the table, P = unreached.
//   plan_seed_kernel    one lane per goal: P = 0 in its cell; its tile, and each neighbouring tile that has the cell in its halo,
//                       active for the first round.
//   plan_round_kernel   one workgroup of 256 per tile (32 x 32 cells planar, 8 x 8 x 8 in 3-D), one launch per round over all tiles; a
//                       tile that is not active leaves at once.  An active one loads P and cost of its haloed box (HaloTile, lv_grid.hpp)
//                       into LDS, works out per cell the mask of allowed moves (plan_move_allowed on the LDS tile), and relaxes
//                       (plan_relax) inside LDS until nothing changes, at most as often as the tile has cells.  Lowered values go
//                       back to global memory (only the owner writes a cell), and the neighbouring tiles that see a lowered border
//                       cell in their halo are marked active for the next round.  A halo read while the neighbour writes is safe:
//                       every stored value is the cost of a real path and values only decrease, and the neighbour marks this tile
//                       for the next round whenever it lowers what this tile may have read too early.
//   plan_stats_kernel   traversable cells, reached cells and the largest finite P, folded per wavefront.
// The rounds are driven by the host: PLAN_ROUNDS_PER_READ launches, then one read of that batch's round words ("this round lowered
// something") through pinned memory.  The build is finished after the first round that lowered nothing.  No workgroup ever waits
// for another one.  The fixpoint is unique, so the schedule does not show in the result.
// lv_occ_plan_paths is one lane per start walking plan_next twice: a counting pass, an exclusive scan, a filling pass.
#include "lv_plan.hpp"

#include <hipcub/hipcub.hpp>

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

constexpr int PLAN_PX = 32, PLAN_PY = 32, PLAN_PZ = 1;   // a planar tile
constexpr int PLAN_VX = 8, PLAN_VY = 8, PLAN_VZ = 8;     // a 3-D tile

__global__ __launch_bounds__(256) void plan_cost_kernel(const int32_t* __restrict__ s2, int min_clear_s2, const uint8_t* __restrict__ table,
                                                        int n_cost, uint32_t n, uint8_t* __restrict__ cost, uint32_t* __restrict__ pot) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    cost[v] = (uint8_t)plan_cell_cost(s2[v], min_clear_s2, table, n_cost);
    pot[v] = PLAN_UNREACHED;
}

template <int TX, int TY, int TZ>
__global__ __launch_bounds__(256) void plan_seed_kernel(PlanGrid g, const float* __restrict__ pts, uint32_t n, const uint8_t* __restrict__ cost,
                                                        uint32_t* __restrict__ pot, uint32_t* __restrict__ active,
                                                        unsigned long long* __restrict__ stats) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float p[3] = {pts[3 * (size_t)q], pts[3 * (size_t)q + 1], pts[3 * (size_t)q + 2]};
    int i, j, k;
    if (!plan_cell_of(g, p, i, j, k)) return;
    const size_t at = grid_at(g, i, j, k);
    if (!cost[at]) return;
    pot[at] = 0u;   // (several goals in one cell store the same value)
    // the goal's tile, and every tile that holds the goal cell in its halo: a goal is never "lowered", so no round would wake them
    const GridDims td = HaloTile<TX, TY, TZ>::tile_dims(g);
    const int tx = i / TX, ty = j / TY, tz = k / TZ;
    const int li = i - tx * TX, lj = j - ty * TY, lk = k - tz * TZ;
    for (int mv = 0; mv < 27; ++mv) {
        int dx, dy, dz;
        plan_move(mv, dx, dy, dz);
        if ((dx < 0 && li != 0) || (dx > 0 && li != TX - 1) || (dy < 0 && lj != 0) || (dy > 0 && lj != TY - 1) || (dz < 0 && lk != 0) ||
            (dz > 0 && lk != TZ - 1))
            continue;
        const int ux = tx + dx, uy = ty + dy, uz = tz + dz;
        if (grid_inside(td, ux, uy, uz)) active[grid_at(td, ux, uy, uz)] = 1u;
    }
    atomicAdd(&stats[0], 1ull);
}

// The accessor of lv_plan.hpp over a workgroup's HaloTile in LDS
template <class T>
struct PlanTile {
    const uint8_t* c;
    const uint32_t* p;
    __device__ __forceinline__ uint32_t cost(int i, int j, int k) const { return c[T::at(i, j, k)]; }
    __device__ __forceinline__ uint32_t pot(int i, int j, int k) const { return p[T::at(i, j, k)]; }
};

enum : uint32_t { PLAN_F_AGAIN = 1u << 6, PLAN_F_LOWERED = 1u << 7 };   // above the six face bits

template <int TX, int TY, int TZ>
__global__ __launch_bounds__(256) void plan_round_kernel(PlanGrid g, const uint8_t* __restrict__ cost, uint32_t* pot, uint32_t* cur, uint32_t* nxt,
                                                         uint32_t* round_word) {
    using T = HaloTile<TX, TY, TZ>;
    constexpr int NPT = T::CELLS / 256;   // cells per lane
    static_assert(T::CELLS % 256 == 0, "a tile is a whole number of cells per lane");
    __shared__ uint32_t sp[T::LCELLS];
    __shared__ uint8_t sc[T::LCELLS];
    __shared__ uint32_t s_flag, s_faces;
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_flag = cur[t];
        cur[t] = 0u;   // (this buffer is `nxt` in the next round: clean by then)
        s_faces = 0u;
    }
    __syncthreads();
    if (!s_flag) return;   // (the whole workgroup)
    const GridDims td = T::tile_dims(g);
    int tx, ty, tz;
    T::origin_of(g, t, tx, ty, tz);
    const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
    for (int l = (int)tid; l < T::LCELLS; l += 256) {
        int di, dj, dk;
        T::halo_of(l, di, dj, dk);
        const bool in = grid_inside(g, x0 + di, y0 + dj, z0 + dk);
        const size_t at = grid_at(g, x0 + di, y0 + dj, z0 + dk);
        sc[l] = in ? cost[at] : (uint8_t)0;
        sp[l] = in ? pot[at] : PLAN_UNREACHED;
    }
    __syncthreads();
    const PlanTile<T> tile{sc, sp};
    const int mv0 = TZ > 1 ? 0 : 9, mv1 = TZ > 1 ? 27 : 18;
    uint32_t mask[NPT], first[NPT];
    int at[NPT];
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        int i, j, k;
        T::local_of((int)tid + q * 256, i, j, k);
        at[q] = T::at(i, j, k);
        first[q] = sp[at[q]];
        uint32_t m = 0;
        for (int mv = mv0; mv < mv1; ++mv) {
            int dx, dy, dz;
            const int nz = plan_move(mv, dx, dy, dz);
            if (nz != 0 && nz <= g.max_m && plan_move_allowed(tile, i, j, k, dx, dy, dz)) m |= 1u << mv;
        }
        mask[q] = m;   // (0 for a blocked cell and for one past the field's edge: its cost is 0)
    }
    int it = 0;
    bool more = true;
    for (; it < T::CELLS && more; ++it) {
        bool changed = false;
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const uint32_t cv = sc[at[q]];
            uint32_t best = sp[at[q]];
            const uint32_t had = best;
            for (uint32_t mm = mask[q]; mm; mm &= mm - 1u) {
                int dx, dy, dz;
                const int nz = plan_move(__builtin_ctz(mm), dx, dy, dz);
                const int u = at[q] + (dz * T::LY + dy) * T::LX + dx;
                const uint32_t cand = plan_relax(sp[u], sc[u], cv, plan_weight(nz));
                best = cand < best ? cand : best;
            }
            if (best < had) {
                sp[at[q]] = best;   // (a neighbour's lane may read the old or the new value: both are costs of real paths)
                changed = true;
            }
        }
        more = __syncthreads_or(changed) != 0;
    }
    uint32_t faces = more ? (uint32_t)PLAN_F_AGAIN : 0u;   // (the cap: not reachable; the tile would go on next round)
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        const uint32_t now = sp[at[q]];
        if (now < first[q]) {
            int i, j, k;
            T::local_of((int)tid + q * 256, i, j, k);
            pot[grid_at(g, x0 + i, y0 + j, z0 + k)] = now;
            faces |= PLAN_F_LOWERED | (i == 0 ? 1u : 0u) | (i == TX - 1 ? 2u : 0u) | (j == 0 ? 4u : 0u) | (j == TY - 1 ? 8u : 0u);
            if (TZ > 1) faces |= (k == 0 ? 16u : 0u) | (k == TZ - 1 ? 32u : 0u);
        }
    }
    if (faces) atomicOr(&s_faces, faces);
    __syncthreads();
    const uint32_t f = s_faces;
    if (!f) return;
    if (tid == 0 && (f & PLAN_F_LOWERED)) *round_word = 1u;
    if (tid < 27) {
        int dx, dy, dz;
        const int nz = plan_move((int)tid, dx, dy, dz);
        if (nz == 0) {
            if (f & PLAN_F_AGAIN) nxt[t] = 1u;
        } else {
            const uint32_t need = (dx < 0 ? 1u : 0u) | (dx > 0 ? 2u : 0u) | (dy < 0 ? 4u : 0u) | (dy > 0 ? 8u : 0u) | (dz < 0 ? 16u : 0u) | (dz > 0 ? 32u : 0u);
            const int ux = tx + dx, uy = ty + dy, uz = tz + dz;
            if ((f & need) == need && grid_inside(td, ux, uy, uz)) nxt[grid_at(td, ux, uy, uz)] = 1u;
        }
    }
}

// stats[1..3]: traversable cells, reached cells, the largest finite P (grid-stride: one atomic per counter and wavefront)
__global__ __launch_bounds__(256) void plan_stats_kernel(const uint8_t* __restrict__ cost, const uint32_t* __restrict__ pot, uint32_t n,
                                                         unsigned long long* __restrict__ stats) {
    unsigned long long trav = 0, reached = 0, top = 0;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
        trav += cost[v] != 0;
        const uint32_t p = pot[v];
        if (p != PLAN_UNREACHED) {
            ++reached;
            top = p > top ? p : top;
        }
    }
    wave_add_to(&stats[1], trav);
    wave_add_to(&stats[2], reached);
    top = wave_max(top);
    if ((threadIdx.x & 63u) == 0 && top) atomicMax(&stats[3], top);
}

// cnt[n] = 0 makes the exclusive scan's entry n the total
template <bool FILL>
__global__ __launch_bounds__(256) void plan_paths_kernel(PlanGrid g, const uint8_t* __restrict__ cost, const uint32_t* __restrict__ pot,
                                                         const float* __restrict__ pts, uint32_t n, int32_t* __restrict__ status,
                                                         uint32_t* __restrict__ pcost, unsigned long long* __restrict__ cnt,
                                                         const unsigned long long* __restrict__ off, int32_t* __restrict__ cells) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n) return;
    if (q == n) {
        if (!FILL) cnt[n] = 0ull;
        return;
    }
    const float p[3] = {pts[3 * (size_t)q], pts[3 * (size_t)q + 1], pts[3 * (size_t)q + 2]};
    const PlanView f{cost, pot, g.nx, g.ny, g.nz};
    int32_t st;
    uint32_t pc;
    const uint64_t len = plan_walk(g, f, p, &st, &pc, FILL ? cells + off[q] : nullptr);
    if (!FILL) {
        status[q] = st;
        pcost[q] = pc;
        cnt[q] = len;
    }
}

}  // namespace

void PlanStore::release() {
    d_cost.release(); d_pot.release(); d_active.release(); d_table.release(); d_round.release(); h_round.release(); stats.release();
    pts.release(); d_status.release(); d_pcost.release(); d_cnt.release(); d_off.release(); d_cells.release(); d_tmp.release();
    *this = PlanStore();
}

// n points (goals or starts) into pts.d
int PlanStore::stage(hipStream_t stream, const void* points, size_t stride, size_t n) {
    const int rc = pts.reserve(stream, n);
    if (rc) return rc;
    pts.append(points, stride, n);
    return pts.upload(stream);
}

int PlanStore::build(hipStream_t stream, const DistStore& dist, const lv_plan_params& p, const uint8_t* cost, size_t n_cost, const void* goals,
                     size_t stride, size_t n_goals, uint64_t out[4]) {
    PlanGrid g{};
    g.nx = dist.grid.nx;
    g.ny = dist.grid.ny;
    g.nz = dist.grid.nz;
    g.planar = dist.prm.planar != 0;
    g.max_m = plan_max_m(p.connectivity);
    for (int a = 0; a < 3; ++a) g.origin[a] = dist.origin[a];
    g.resolution = dist.grid.resolution;
    const size_t nc = dist.n_vox;
    const size_t nt = g.planar ? HaloTile<PLAN_PX, PLAN_PY, PLAN_PZ>::tiles(g) : HaloTile<PLAN_VX, PLAN_VY, PLAN_VZ>::tiles(g);
    int rc = stage(stream, goals, stride, n_goals);
    if (rc) return rc;
    built = false;   // (before a buffer goes: the old plan's are overwritten from here on; the new one stands when the rounds are through)
    rc = d_cost.need(nc);
    if (!rc) rc = d_pot.need(nc);
    if (!rc) rc = d_active.need(2 * nt);
    if (!rc) rc = d_table.need(PLAN_MAX_COST);
    if (!rc) rc = d_round.need(PLAN_ROUNDS_PER_READ);
    if (!rc) rc = h_round.need(PLAN_ROUNDS_PER_READ);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_table, cost, n_cost, hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetAsync(d_active, 0, 2 * nt * sizeof(uint32_t), stream));
    rc = stats.zero(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(plan_cost_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, dist.d_s2, p.min_clear_s2, d_table, (int)n_cost, (uint32_t)nc,
                       d_cost, d_pot);
    const auto seed_kernel = g.planar ? plan_seed_kernel<PLAN_PX, PLAN_PY, PLAN_PZ> : plan_seed_kernel<PLAN_VX, PLAN_VY, PLAN_VZ>;
    const auto round_kernel = g.planar ? plan_round_kernel<PLAN_PX, PLAN_PY, PLAN_PZ> : plan_round_kernel<PLAN_VX, PLAN_VY, PLAN_VZ>;
    hipLaunchKernelGGL(seed_kernel, dim3(blocks_of(n_goals)), dim3(256), 0, stream, g, pts.d, (uint32_t)n_goals, d_cost, d_pot, d_active, stats.d);
    LV_HIP(hipGetLastError());
    // the rounds: a batch of launches, then one look at the batch's words.  Once a round lowers nothing no later one does.
    size_t done = 0;   // rounds launched so far
    bool finished = false;
    while (!finished) {
        if (done > nc) { set_error("lv_occ_plan_build: no fixpoint after %zu rounds", done); return LV_ESTATE; }   // (not reachable)
        LV_HIP(hipMemsetAsync(d_round, 0, PLAN_ROUNDS_PER_READ * sizeof(uint32_t), stream));
        for (int r = 0; r < PLAN_ROUNDS_PER_READ; ++r) {
            uint32_t* cur = d_active + ((done + (size_t)r) & 1) * nt;
            uint32_t* nxt = d_active + ((done + (size_t)r + 1) & 1) * nt;
            hipLaunchKernelGGL(round_kernel, dim3((uint32_t)nt), dim3(256), 0, stream, g, d_cost, d_pot, cur, nxt, d_round + r);
        }
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(h_round, d_round, PLAN_ROUNDS_PER_READ * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        for (int r = 0; r < PLAN_ROUNDS_PER_READ && !finished; ++r) {
            ++done;
            finished = h_round[r] == 0;
        }
    }
    hipLaunchKernelGGL(plan_stats_kernel, dim3(blocks_of(nc) < 1024u ? blocks_of(nc) : 1024u), dim3(256), 0, stream, d_cost, d_pot, (uint32_t)nc, stats.d);
    LV_HIP(hipGetLastError());
    rc = stats.read(stream, out);
    if (rc) return rc;
    prm = p;
    grid = g;
    n_cells = nc;
    n_tiles = nt;
    rounds = (int)done;
    stale = 0;
    built = true;
    return LV_OK;
}

int PlanStore::fetch(hipStream_t stream, uint32_t* potential, uint8_t* cell_cost) {
    if (potential) LV_HIP(hipMemcpyAsync(potential, d_pot, n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (cell_cost) LV_HIP(hipMemcpyAsync(cell_cost, d_cost, n_cells * sizeof(uint8_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int PlanStore::paths(hipStream_t stream, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets,
                     int32_t* cells, size_t capacity, size_t* total) {
    *total = 0;
    offsets[0] = 0;
    if (n == 0) return LV_OK;
    int rc = stage(stream, starts, stride, n);
    if (!rc) rc = d_status.need(n);
    if (!rc) rc = d_pcost.need(n);
    if (!rc) rc = d_cnt.need(n + 1);
    if (!rc) rc = d_off.need(n + 1);
    if (rc) return rc;
    hipLaunchKernelGGL(plan_paths_kernel<false>, dim3(blocks_of(n + 1)), dim3(256), 0, stream, grid, d_cost, d_pot, pts.d, (uint32_t)n, d_status, d_pcost,
                       d_cnt, (const unsigned long long*)nullptr, (int32_t*)nullptr);
    LV_HIP(hipGetLastError());
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_cnt.p, d_off.p, (int)(n + 1), stream));
    rc = d_tmp.need(bytes);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(d_tmp.p, bytes, d_cnt.p, d_off.p, (int)(n + 1), stream));
    static_assert(sizeof(size_t) == sizeof(unsigned long long), "offsets are copied out as size_t");
    LV_HIP(hipMemcpyAsync(offsets, d_off, (n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipMemcpyAsync(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipMemcpyAsync(cost, d_pcost, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    const size_t tot = offsets[n];
    *total = tot;
    if (!cells) return LV_OK;   // count only: any total
    if (capacity < tot) { set_error("capacity %zu < %zu path cells", capacity, tot); return LV_EINVAL; }
    if (tot > (size_t)0x7FFFFFFF) {
        set_error("%zu path cells: one call returns at most 2^31 - 1 (split the starts; the count-only call has no limit)", tot);
        return LV_EINVAL;
    }
    if (tot == 0) return LV_OK;
    rc = d_cells.need(tot);
    if (rc) return rc;
    hipLaunchKernelGGL(plan_paths_kernel<true>, dim3(blocks_of(n + 1)), dim3(256), 0, stream, grid, d_cost, d_pot, pts.d, (uint32_t)n, d_status, d_pcost,
                       d_cnt, (const unsigned long long*)d_off.p, d_cells);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(cells, d_cells, tot * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
