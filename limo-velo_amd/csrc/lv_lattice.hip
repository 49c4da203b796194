// lv_lattice.hip — the state-lattice planner (include/limovelo_hip.h "Lattice planner"; the rule's code is lv_lattice.hpp).
//
// A build is a block-based label-correcting solver on the context's stream, in the shape of lv_plan.hip:
//   (copy)               the plan's cost bytes, device to device; V = unreached (a fill).
//   lat_seed_kernel      one lane per goal record: V = 0 on its state (h = -1: on all H of the cell); every tile whose haloed box
//                        holds the goal cell active for the first round (a goal is never "lowered", so no round would wake them).
//   lat_round_kernel<T>  one workgroup of 256 per tile of T x T cells FOR ALL H HEADINGS, one launch per round over all tiles; a
//                        tile that is not active leaves at once.  An active one loads V of its box, haloed by `reach` cells, for
//                        every heading, and the box's cost bytes, into LDS; works out once per state the mask of allowed
//                        primitives (lat_prim_allowed on the LDS box: the sweep test is not redone in the inner iteration); and
//                        PULLS inside LDS until nothing changes: a state lowers itself from its successors (lat_relax), at most as
//                        often as the tile has states.  Lowered values go back to global memory (only the owner writes a state),
//                        and every tile whose haloed box holds a lowered cell is marked active for the next round.  A halo read
//                        while the neighbour writes is safe: every stored value is the cost of a real sequence and values only
//                        fall, and the neighbour marks this tile whenever it lowers what this tile may have read too early.
//                        The 64 lanes of a wavefront share one heading (T = 16: a lane per cell, the headings in turn; T = 8: a
//                        wavefront per heading, four at a time), so the primitive's record is wave-uniform: scalar loads.
//   lat_stats_kernel     traversable states, reached states and the largest finite V, folded per wavefront.
// The rounds are driven by the host as the plan's are: PLAN_ROUNDS_PER_READ launches, then one read of that batch's round words
// through pinned memory.  No workgroup ever waits for another one.  The fixpoint is unique, so the schedule does not show.
// lv_occ_lattice_paths is one lane per start walking lat_walk twice: a counting pass, an exclusive scan, a filling pass.
#include "lv_lattice.hpp"

#include <hipcub/hipcub.hpp>

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

constexpr int LAT_LDS_BUDGET = 65536 - 1024;   // dynamic LDS of a workgroup: the 64 KB a kernel gets without asking, less its static words and their padding
static_assert(offsetof(lv_lattice_prim, length) == 4 && offsetof(lv_lattice_prim, penalty) == 8, "the round kernel reads a record's first three words");
static_assert(LAT_REACH <= 8, "a tile of edge 8 sees a lowered cell at most one tile away");

// bytes of LDS a tile of edge T takes: V of the box per heading, the masks of the tile's states, the cost bytes of the box
__host__ __device__ inline size_t lat_lds_bytes(int T, int reach, int H) {
    const size_t B = (size_t)(T + 2 * reach);
    return B * B * 4 * (size_t)H + (size_t)T * T * 2 * (size_t)H + ((B * B + 3) & ~(size_t)3);
}

// the strips of a tile of edge T whose cells lie in a neighbouring tile's haloed box: bit 0: the tile at -x, 1: +x, 2: -y, 3: +y
__host__ __device__ inline uint32_t lat_strips(int T, int reach, int li, int lj) {
    return (li < reach ? 1u : 0u) | (li >= T - reach ? 2u : 0u) | (lj < reach ? 4u : 0u) | (lj >= T - reach ? 8u : 0u);
}
// what neighbour (dx, dy), each -1, 0, 1, needs of those bits
__host__ __device__ inline uint32_t lat_need(int dx, int dy) {
    return (dx < 0 ? 1u : 0u) | (dx > 0 ? 2u : 0u) | (dy < 0 ? 4u : 0u) | (dy > 0 ? 8u : 0u);
}

__global__ __launch_bounds__(256) void lat_seed_kernel(LatGrid g, int T, int reach, const uint32_t* __restrict__ rec, uint32_t n,
                                                       const uint8_t* __restrict__ cost, uint32_t* __restrict__ V, uint32_t* __restrict__ active,
                                                       unsigned long long* __restrict__ stats) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float p[3] = {__uint_as_float(rec[4 * (size_t)q]), __uint_as_float(rec[4 * (size_t)q + 1]), __uint_as_float(rec[4 * (size_t)q + 2])};
    const int32_t h = (int32_t)rec[4 * (size_t)q + 3];
    int i, j;
    if (h < -1 || h >= g.H || !lat_cell_of(g, p, i, j)) return;
    if (!cost[grid_at(g, i, j, 0)]) return;
    for (int t = (h < 0 ? 0 : h); t < (h < 0 ? g.H : h + 1); ++t) V[lat_at(g, i, j, t)] = 0u;   // (several goals on one state store the same value)
    const GridDims td{(g.nx + T - 1) / T, (g.ny + T - 1) / T, 1};
    const int tx = i / T, ty = j / T;
    const uint32_t strips = lat_strips(T, reach, i - tx * T, j - ty * T);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t need = lat_need(dx, dy);
            if ((strips & need) == need && grid_inside(td, tx + dx, ty + dy, 0)) active[grid_at(td, tx + dx, ty + dy, 0)] = 1u;
        }
    atomicAdd(&stats[0], 1ull);
}

// The accessor of lv_lattice.hpp over a workgroup's box in LDS: (i, j) are box coordinates
struct LatBox {
    const uint8_t* c;
    const uint32_t* v;
    int B, BB;
    __device__ __forceinline__ uint32_t cost(int i, int j) const { return c[j * B + i]; }
    __device__ __forceinline__ uint32_t pot(int i, int j, int h) const { return v[h * BB + j * B + i]; }
};

enum : uint32_t { LAT_F_AGAIN = 1u << 4, LAT_F_LOWERED = 1u << 5 };   // above the four strip bits

template <int T>
__global__ __launch_bounds__(256) void lat_round_kernel(LatGrid g, int reach, const lv_lattice_prim* __restrict__ prims, const uint8_t* __restrict__ cost,
                                                        uint32_t* V, uint32_t* cur, uint32_t* nxt, uint32_t* round_word) {
    constexpr int C = T * T;        // cells of the tile: 256 or 64
    constexpr int G = 256 / C;      // headings in flight: 1 or 4
    static_assert(C == 256 || C == 64, "a wavefront's 64 lanes share one heading");
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t s_flag, s_strips;
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_flag = cur[t];
        cur[t] = 0u;   // (this buffer is `nxt` in the next round: clean by then)
        s_strips = 0u;
    }
    __syncthreads();
    if (!s_flag) return;   // (the whole workgroup)
    const int H = g.H, P = g.P;
    const int B = T + 2 * reach, BB = B * B;
    uint32_t* sV = lds;                                        // [H][BB]
    uint16_t* sm = reinterpret_cast<uint16_t*>(sV + H * BB);   // [H][C]
    uint8_t* sc = reinterpret_cast<uint8_t*>(sm + H * C);      // [BB]
    const GridDims td{(g.nx + T - 1) / T, (g.ny + T - 1) / T, 1};
    const int ty = (int)(t / (uint32_t)td.nx), tx = (int)(t - (uint32_t)ty * (uint32_t)td.nx);
    const int x0 = tx * T - reach, y0 = ty * T - reach;   // the box's origin
    const size_t plane = (size_t)g.nx * (size_t)g.ny;
    for (int l = (int)tid; l < BB; l += 256) {
        const int bj = l / B, bi = l - bj * B;
        const bool in = grid_inside(g, x0 + bi, y0 + bj, 0);
        const size_t at = in ? grid_at(g, x0 + bi, y0 + bj, 0) : 0;
        sc[l] = in ? cost[at] : (uint8_t)0;
        for (int h = 0; h < H; ++h) sV[h * BB + l] = in ? V[(size_t)h * plane + at] : LAT_UNREACHED;
    }
    __syncthreads();
    // this lane's cell, and the first of its headings: uniform over the wavefront
    const int c = (int)tid % C, lj = c / T, li = c - lj * T;
    const int hg = G == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)tid / C);
    const int at = (lj + reach) * B + li + reach;
    const LatBox box{sc, sV, B, BB};
    for (int h = hg; h < H; h += G) {
        uint32_t m = 0;
        for (int p = 0; p < P; ++p)
            if (lat_prim_allowed(box, prims[h * P + p], li + reach, lj + reach)) m |= 1u << p;
        sm[h * C + c] = (uint16_t)m;   // (0 for a blocked cell and for one past the grid's edge: its cost is 0)
    }
    const uint32_t cu = sc[at];
    const int cap = C * H;
    int it = 0;
    bool more = true;
    for (; it < cap && more; ++it) {
        bool changed = false;
        for (int h = hg; h < H; h += G) {
            const uint32_t m = sm[h * C + c];
            const uint32_t had = sV[h * BB + at];
            uint32_t best = had;
            for (int p = 0; p < P; ++p) {
                // the record's first 12 bytes as three words: wave-uniform (h and p are), so three scalar loads; there is no scalar
                // load of a byte or a half-word, and the fields read one by one would come through the vector memory path
                uint32_t w[3];
                __builtin_memcpy(w, &prims[h * P + p], sizeof(w));
                const int di = (int8_t)(w[0] & 0xFFu), dj = (int8_t)((w[0] >> 8) & 0xFFu), h_to = (int)((w[0] >> 16) & 0xFFu);
                if ((m >> p) & 1u) {
                    const int u = at + dj * B + di;
                    const uint32_t cand = lat_relax(sV[h_to * BB + u], lat_edge(cu, sc[u], w[1] & 0xFFFFu, w[2]));
                    best = cand < best ? cand : best;
                }
            }
            if (best < had) {
                sV[h * BB + at] = best;   // (another lane may read the old or the new value: both are costs of real sequences)
                changed = true;
            }
        }
        more = __syncthreads_or(changed) != 0;
    }
    uint32_t flags = more ? (uint32_t)LAT_F_AGAIN : 0u;   // (the cap: not reachable; the tile would go on next round)
    const int gi = x0 + reach + li, gj = y0 + reach + lj;
    if (grid_inside(g, gi, gj, 0)) {
        const size_t gat = grid_at(g, gi, gj, 0);
        for (int h = hg; h < H; h += G) {
            const uint32_t now = sV[h * BB + at];
            if (now < V[(size_t)h * plane + gat]) {   // (only this workgroup writes the state: what it reads here is what it loaded)
                V[(size_t)h * plane + gat] = now;
                flags |= LAT_F_LOWERED | lat_strips(T, reach, li, lj);
            }
        }
    }
    if (flags) atomicOr(&s_strips, flags);
    __syncthreads();
    const uint32_t f = s_strips;
    if (!f) return;
    if (tid == 0 && (f & LAT_F_LOWERED)) *round_word = 1u;
    if (tid < 9) {
        const int dx = (int)tid % 3 - 1, dy = (int)tid / 3 - 1;
        if (dx == 0 && dy == 0) {
            if (f & LAT_F_AGAIN) nxt[t] = 1u;
        } else if (f & LAT_F_LOWERED) {
            const uint32_t need = lat_need(dx, dy);
            if ((f & need) == need && grid_inside(td, tx + dx, ty + dy, 0)) nxt[grid_at(td, tx + dx, ty + dy, 0)] = 1u;
        }
    }
}

// stats[1..3]: traversable states, reached states, the largest finite V (grid-stride: one atomic per counter and wavefront)
__global__ __launch_bounds__(256) void lat_stats_kernel(const uint8_t* __restrict__ cost, const uint32_t* __restrict__ V, uint32_t n_cells, uint32_t n_states,
                                                        unsigned long long* __restrict__ stats) {
    unsigned long long trav = 0, reached = 0, top = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_states; s += gridDim.x * blockDim.x) {
        trav += cost[s % n_cells] != 0;
        const uint32_t v = V[s];
        if (v != LAT_UNREACHED) {
            ++reached;
            top = v > top ? v : top;
        }
    }
    wave_add_to(&stats[1], trav);
    wave_add_to(&stats[2], reached);
    top = wave_max(top);
    if ((threadIdx.x & 63u) == 0 && top) atomicMax(&stats[3], top);
}

// cnt[n] = 0 makes the exclusive scan's entry n the total
template <bool FILL>
__global__ __launch_bounds__(256) void lat_paths_kernel(LatGrid g, const lv_lattice_prim* __restrict__ prims, const uint8_t* __restrict__ cost,
                                                        const uint32_t* __restrict__ V, const uint32_t* __restrict__ rec, uint32_t n,
                                                        int32_t* __restrict__ status, uint32_t* __restrict__ pcost, unsigned long long* __restrict__ cnt,
                                                        const unsigned long long* __restrict__ off, int32_t* __restrict__ states,
                                                        uint8_t* __restrict__ taken) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n) return;
    if (q == n) {
        if (!FILL) cnt[n] = 0ull;
        return;
    }
    const float p[3] = {__uint_as_float(rec[4 * (size_t)q]), __uint_as_float(rec[4 * (size_t)q + 1]), __uint_as_float(rec[4 * (size_t)q + 2])};
    const LatView f{cost, V, g.nx, g.ny, 1};
    int32_t st;
    uint32_t pc;
    const uint64_t len = lat_walk(g, f, prims, p, (int32_t)rec[4 * (size_t)q + 3], &st, &pc, FILL ? states + off[q] : nullptr, FILL ? taken + off[q] : nullptr);
    if (!FILL) {
        status[q] = st;
        pcost[q] = pc;
        cnt[q] = len;
    }
}

// n records of 16 bytes (goals or starts) into d_rec.  The stream is synchronised first: the previous upload has left the pinned
// buffer before it is overwritten or freed (PointStage's rule)
int stage_records(hipStream_t stream, PinBuf<uint32_t>& h, DevBuf<uint32_t>& d, const void* recs, size_t stride, size_t n) {
    LV_HIP(hipStreamSynchronize(stream));
    int rc = h.need(4 * n);
    if (!rc) rc = d.need(4 * n);
    if (rc) return rc;
    const char* b = static_cast<const char*>(recs);
    for (size_t i = 0; i < n; ++i) std::memcpy(h.p + 4 * i, b + i * stride, 16);
    LV_HIP(hipMemcpyAsync(d.p, h.p, 16 * n, hipMemcpyHostToDevice, stream));
    return LV_OK;
}

}  // namespace

int LatticeStore::build(hipStream_t stream, const PlanStore& plan, const lv_lattice_params& p, const lv_lattice_prim* prims, const void* goals,
                        size_t stride, size_t n_goals, uint64_t out[4]) {
    LatGrid g{};
    g.nx = plan.grid.nx;
    g.ny = plan.grid.ny;
    g.nz = 1;
    g.H = p.H;
    g.P = p.P;
    for (int a = 0; a < 3; ++a) g.origin[a] = plan.grid.origin[a];
    g.resolution = plan.grid.resolution;
    const size_t n_prims = (size_t)p.H * (size_t)p.P;
    const int R = lat_reach_of(prims, n_prims);
    const int T = lat_lds_bytes(16, R, p.H) <= (size_t)LAT_LDS_BUDGET ? 16 : 8;   // (edge 8 always fits: 24 * 24 * 65 + 2048 bytes at most)
    const size_t lds = lat_lds_bytes(T, R, p.H);
    const size_t nc = (size_t)g.nx * (size_t)g.ny, ns = nc * (size_t)p.H;
    const size_t nt = (size_t)((g.nx + T - 1) / T) * (size_t)((g.ny + T - 1) / T);
    int rc = stage_records(stream, h_rec, d_rec, goals, stride, n_goals);
    if (rc) return rc;
    built = false;   // (before a buffer goes: the old lattice's are overwritten from here on; the new one stands when the rounds are through)
    rc = d_cost.need(nc);
    if (!rc) rc = d_V.need(ns);
    if (!rc) rc = d_active.need(2 * nt);
    if (!rc) rc = d_prims.need((size_t)LAT_MAX_H * LAT_MAX_P);
    if (!rc) rc = d_round.need(PLAN_ROUNDS_PER_READ);
    if (!rc) rc = h_round.need(PLAN_ROUNDS_PER_READ);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_prims, prims, n_prims * sizeof(lv_lattice_prim), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_cost, plan.d_cost, nc, hipMemcpyDeviceToDevice, stream));
    LV_HIP(hipMemsetAsync(d_V, 0xFF, ns * sizeof(uint32_t), stream));
    LV_HIP(hipMemsetAsync(d_active, 0, 2 * nt * sizeof(uint32_t), stream));
    rc = stats.zero(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(lat_seed_kernel, dim3(blocks_of(n_goals)), dim3(256), 0, stream, g, T, R, d_rec, (uint32_t)n_goals, d_cost, d_V, d_active, stats.d);
    LV_HIP(hipGetLastError());
    LV_HIP(hipStreamSynchronize(stream));   // (the caller's table has left the host: prims need not be pinned memory)
    const auto round_kernel = T == 16 ? lat_round_kernel<16> : lat_round_kernel<8>;
    // the rounds: a batch of launches, then one look at the batch's words.  Once a round lowers nothing no later one does.
    size_t done = 0;   // rounds launched so far
    bool finished = false;
    while (!finished) {
        if (done > ns) { set_error("lv_occ_lattice_build: no fixpoint after %zu rounds", done); return LV_ESTATE; }   // (not reachable)
        LV_HIP(hipMemsetAsync(d_round, 0, PLAN_ROUNDS_PER_READ * sizeof(uint32_t), stream));
        for (int r = 0; r < PLAN_ROUNDS_PER_READ; ++r) {
            uint32_t* cur = d_active + ((done + (size_t)r) & 1) * nt;
            uint32_t* nxt = d_active + ((done + (size_t)r + 1) & 1) * nt;
            hipLaunchKernelGGL(round_kernel, dim3((uint32_t)nt), dim3(256), lds, stream, g, R, d_prims, d_cost, d_V, cur, nxt, d_round + r);
        }
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(h_round, d_round, PLAN_ROUNDS_PER_READ * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        for (int r = 0; r < PLAN_ROUNDS_PER_READ && !finished; ++r) {
            ++done;
            finished = h_round[r] == 0;
        }
    }
    hipLaunchKernelGGL(lat_stats_kernel, dim3(blocks_of(ns) < 1024u ? blocks_of(ns) : 1024u), dim3(256), 0, stream, d_cost, d_V, (uint32_t)nc, (uint32_t)ns,
                       stats.d);
    LV_HIP(hipGetLastError());
    rc = stats.read(stream, out);
    if (rc) return rc;
    prm = p;
    grid = g;
    n_cells = nc;
    n_states = ns;
    n_tiles = nt;
    rounds = (int)done;
    tile = T;
    reach = R;
    stale = 0;
    built = true;
    return LV_OK;
}

int LatticeStore::fetch(hipStream_t stream, uint32_t* V) {
    LV_HIP(hipMemcpyAsync(V, d_V, n_states * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int LatticeStore::paths(hipStream_t stream, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets,
                        int32_t* states, uint8_t* prims_taken, size_t capacity, size_t* total) {
    *total = 0;
    offsets[0] = 0;
    if (n == 0) return LV_OK;
    int rc = stage_records(stream, h_rec, d_rec, starts, stride, n);
    if (!rc) rc = d_status.need(n);
    if (!rc) rc = d_pcost.need(n);
    if (!rc) rc = d_cnt.need(n + 1);
    if (!rc) rc = d_off.need(n + 1);
    if (rc) return rc;
    hipLaunchKernelGGL(lat_paths_kernel<false>, dim3(blocks_of(n + 1)), dim3(256), 0, stream, grid, d_prims, d_cost, d_V, d_rec, (uint32_t)n, d_status, d_pcost,
                       d_cnt, (const unsigned long long*)nullptr, (int32_t*)nullptr, (uint8_t*)nullptr);
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
    if (!states) return LV_OK;   // count only: any total
    if (capacity < tot) { set_error("lv_occ_lattice_paths: capacity %zu < %zu path states", capacity, tot); return LV_EINVAL; }
    if (tot > (size_t)0x7FFFFFFF) {
        set_error("lv_occ_lattice_paths: %zu path states: one call returns at most 2^31 - 1 (split the starts; the count-only call has no limit)", tot);
        return LV_EINVAL;
    }
    if (tot == 0) return LV_OK;
    rc = d_states.need(tot);
    if (!rc) rc = d_taken.need(tot);
    if (rc) return rc;
    hipLaunchKernelGGL(lat_paths_kernel<true>, dim3(blocks_of(n + 1)), dim3(256), 0, stream, grid, d_prims, d_cost, d_V, d_rec, (uint32_t)n, d_status, d_pcost,
                       d_cnt, (const unsigned long long*)d_off.p, d_states.p, d_taken.p);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(states, d_states, tot * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (prims_taken) LV_HIP(hipMemcpyAsync(prims_taken, d_taken, tot * sizeof(uint8_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
