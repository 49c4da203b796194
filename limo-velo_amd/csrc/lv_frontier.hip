// lv_frontier.hip — frontier detection and ranking on the occupancy grid (include/limovelo_hip.h "Frontiers"; the rule's code is
// lv_frontier.hpp).
//
// A build is connected-component labelling in tiles on the context's stream:
//   fr_tile_kernel      one workgroup of 256 per tile (32 x 32 cells planar, 32 x 8 x 4 in 3-D; 4 cells per lane).  The states of the
//                       tile's haloed box (HaloTile, lv_grid.hpp) go into LDS (3-D: one read of L per cell instead of seven; planar: the column's
//                       projection), the frontier predicate runs on the LDS tile, and the tile's frontier cells are labelled in LDS
//                       to the tile's fixpoint: every cell takes the least label among its neighbours (fr_neighbour), then the
//                       label of its label, until nothing changes.  Only a cell's owner writes its label and labels only fall, so
//                       a read beside a write sees an older label of the same component.  The labels leave as global cell indices
//                       in parent[]: within a tile every frontier cell points at the smallest cell of its piece, which points at
//                       itself: a union-find forest as lv_cluster.hpp wants it.
//   fr_seam_kernel      one lane per cell: a frontier cell links (cl_link) with each frontier neighbour in ANOTHER tile, through the
//                       offsets towards smaller indices (each pair once).  A serpentine through every tile is one chain of such
//                       links; with global propagation rounds it would take as many launches as the chain has tiles.
//   fr_flatten_kernel   every frontier cell's root (cl_root) into root[]; the roots are counted.
//   fr_assign_kernel    the roots get dense numbers (an atomic counter: which root gets which number is the schedule's business and
//                       shows nowhere, the order below is by key), so that everything 64-bit is sized by roots.
//   fr_accumulate_kernel  size, sum, lo, hi per root by integer atomics, one set per wavefront where the wavefront is of one root.
//   fr_key_kernel, hipcub radix sort, fr_number_kernel   the roots by (size descending, first ascending); the cluster records.
//   fr_label_kernel     the labels, and every member's bid for rep (64-bit atomicMin on (d2 << 32) | cell); fr_rep_kernel stores it.
// Integer atomics only: the result is the same bits whatever the schedule.  No lane waits for a value another lane has yet to
// write; the host reads two counters (roots, clusters) to size the next buffers.
// lv_occ_frontier_rank is one kernel: a lane per labelled cell scans its window of P (fr_rank_window) and bids with a 64-bit
// atomicMin on (P << 32) | cell.
#include "lv_frontier.hpp"

#include <hipcub/hipcub.hpp>

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

constexpr int FR_PX = 32, FR_PY = 32, FR_PZ = 1;   // a planar tile
constexpr int FR_VX = 32, FR_VY = 8, FR_VZ = 4;    // a 3-D tile

// The accessor of lv_frontier.hpp over a workgroup's HaloTile in LDS
template <class T>
struct FrTile {
    const uint8_t* s;
    __device__ __forceinline__ int state(int i, int j, int k) const { return s[T::at(i, j, k)]; }
};

// the neighbour offsets of the connectivity as a mask over plan_move's 27 (uniform: scalar work)
__device__ __forceinline__ uint32_t fr_neighbour_mask(const FrontierGrid& g) {
    uint32_t m = 0;
    for (int mv = 0; mv < 27; ++mv) {
        int dx, dy, dz;
        if (fr_neighbour(mv, g.max_m, g.planar != 0, dx, dy, dz)) m |= 1u << mv;
    }
    return m;
}

// L: the whole grid; planar: k0..k1 the clipped band and plane = nx * ny.  stats[0..2]: FREE, UNKNOWN, frontier cells.
template <int TX, int TY, int TZ>
__global__ __launch_bounds__(256) void fr_tile_kernel(const float* __restrict__ L, FrontierGrid g, int k0, int k1, float l_free, float l_occ,
                                                      uint32_t* __restrict__ parent, unsigned long long* __restrict__ stats) {
    using T = HaloTile<TX, TY, TZ>;
    constexpr int NPT = T::CELLS / 256;   // cells per lane
    static_assert(T::CELLS % 256 == 0, "a tile is a whole number of cells per lane");
    __shared__ uint8_t ss[T::LCELLS];
    __shared__ uint32_t sl[T::LCELLS];
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    int tx, ty, tz;
    T::origin_of(g, t, tx, ty, tz);
    const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
    const size_t plane = (size_t)g.nx * (size_t)g.ny;
    for (int l = (int)tid; l < T::LCELLS; l += 256) {
        int di, dj, dk;
        T::halo_of(l, di, dj, dk);
        int st = FR_OUTSIDE;
        if (grid_inside(g, x0 + di, y0 + dj, z0 + dk)) {
            const size_t cell = grid_at(g, x0 + di, y0 + dj, z0 + dk);   // (planar: z0 + dk = 0, the cell is the column)
            st = g.planar ? fr_state_column(L, plane, cell, k0, k1, l_free, l_occ) : fr_state_voxel(L[cell], l_free, l_occ);
        }
        ss[l] = (uint8_t)st;
        sl[l] = CL_NONE;
    }
    __syncthreads();
    const FrTile<T> tile{ss};
    int at[NPT];
    bool mine[NPT];
    unsigned long long n_free = 0, n_unknown = 0, n_frontier = 0;
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        int i, j, k;
        T::local_of((int)tid + q * 256, i, j, k);
        at[q] = T::at(i, j, k);
        const int st = ss[at[q]];   // (FR_OUTSIDE past the field's edge: neither counted nor a frontier)
        n_free += st == FR_FREE;
        n_unknown += st == FR_UNKNOWN;
        mine[q] = fr_is_frontier(tile, g.planar != 0, i, j, k);
        n_frontier += mine[q];
    }
#pragma unroll
    for (int q = 0; q < NPT; ++q)
        if (mine[q]) sl[at[q]] = (uint32_t)at[q];   // (the halo keeps CL_NONE: this tile's labelling stays inside it)
    __syncthreads();
    const uint32_t nb = fr_neighbour_mask(g);
    bool more = true;
    while (more) {   // (every change lowers a label: it ends)
        bool changed = false;
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            if (!mine[q]) continue;
            const uint32_t own = sl[at[q]];
            uint32_t m = own;
            for (uint32_t mm = nb; mm; mm &= mm - 1u) {
                int dx, dy, dz;
                plan_move(__builtin_ctz(mm), dx, dy, dz);
                const uint32_t v = sl[at[q] + (dz * T::LY + dy) * T::LX + dx];
                m = v < m ? v : m;
            }
            if (m < own) {
                sl[at[q]] = m;
                changed = true;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            if (!mine[q]) continue;
            const uint32_t a = sl[at[q]], b = sl[a];   // (a is a frontier cell of this tile: its label is one too)
            if (b < a) {
                sl[at[q]] = b;
                changed = true;
            }
        }
        more = __syncthreads_or(changed) != 0;
    }
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        int i, j, k;
        T::local_of((int)tid + q * 256, i, j, k);
        if (x0 + i >= g.nx || y0 + j >= g.ny || z0 + k >= g.nz) continue;
        uint32_t p = CL_NONE;
        if (mine[q]) {   // the LDS label back to the global cell it stands for
            int li, lj, lk;
            T::halo_of((int)sl[at[q]], li, lj, lk);
            p = (uint32_t)grid_at(g, x0 + li, y0 + lj, z0 + lk);
        }
        parent[grid_at(g, x0 + i, y0 + j, z0 + k)] = p;
    }
    wave_add_to(&stats[0], n_free);
    wave_add_to(&stats[1], n_unknown);
    wave_add_to(&stats[2], n_frontier);
}

// (tx, ty, tz: the tile edges of fr_tile_kernel)
__global__ __launch_bounds__(256) void fr_seam_kernel(FrontierGrid g, int tx, int ty, int tz, uint32_t n, uint32_t* parent) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || cl_load(parent + c) == CL_NONE) return;
    int i, j, k;
    fr_cell_ijk(g, c, i, j, k);
    for (int mv = 0; mv < 13; ++mv) {
        int dx, dy, dz;
        if (!fr_neighbour(mv, g.max_m, g.planar != 0, dx, dy, dz)) continue;
        const int ni = i + dx, nj = j + dy, nk = k + dz;
        if (!grid_inside(g, ni, nj, nk)) continue;
        if (ni / tx == i / tx && nj / ty == j / ty && nk / tz == k / tz) continue;   // (the tile has joined them)
        const uint32_t v = (uint32_t)grid_at(g, ni, nj, nk);
        if (cl_load(parent + v) != CL_NONE) cl_link(parent, c, v);
    }
}

// cnt[0]: the roots
__global__ __launch_bounds__(256) void fr_flatten_kernel(uint32_t n, const uint32_t* parent, uint32_t* __restrict__ root, unsigned long long* __restrict__ cnt) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    bool is_root = false;
    if (c < n) {
        uint32_t r = CL_NONE;
        if (cl_load(parent + c) != CL_NONE) r = cl_root(parent, c);
        root[c] = r;
        is_root = r == c;
    }
    const unsigned long long m = __ballot(is_root);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(&cnt[0], (unsigned long long)__popcll(m));
}

// cnt[1]: the numbers handed out.  A root's number replaces its parent entry (the union-find has served).
__global__ __launch_bounds__(256) void fr_assign_kernel(uint32_t n, const uint32_t* __restrict__ root, uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ first, unsigned long long* __restrict__ cnt) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || root[c] != c) return;
    const uint32_t d = (uint32_t)atomicAdd(&cnt[1], 1ull);
    parent[c] = d;
    first[d] = c;
}

// lo, hi: 3 per root
__global__ __launch_bounds__(256) void fr_accumulate_kernel(FrontierGrid g, uint32_t n, const uint32_t* __restrict__ root, const uint32_t* __restrict__ parent,
                                                            uint32_t* __restrict__ size, unsigned long long* __restrict__ sum, int32_t* __restrict__ blo,
                                                            int32_t* __restrict__ bhi) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = c < n ? root[c] : CL_NONE;
    const bool valid = r != CL_NONE;
    const unsigned long long vm = __ballot(valid);
    if (!vm) return;   // (the whole wavefront)
    const uint32_t d = valid ? parent[r] : 0u;
    int v[3] = {0, 0, 0};
    if (valid) fr_cell_ijk(g, c, v[0], v[1], v[2]);
    const int src = __ffsll((long long)vm) - 1;
    const uint32_t d0 = __shfl(d, src);
    if (__ballot(valid && d != d0) == 0) {   // one root: one set of atomics
        const unsigned long long members = (unsigned long long)__popcll(vm);
        unsigned long long s[3];
        int lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            s[a] = wave_sum(valid ? (unsigned long long)v[a] : 0ull);
            lo[a] = wave_min(valid ? v[a] : 0x7FFFFFFF);
            hi[a] = wave_max(valid ? v[a] : -1);
        }
        if ((int)(threadIdx.x & 63u) == src) {
            atomicAdd(&size[d0], (uint32_t)members);
            for (int a = 0; a < 3; ++a) {
                atomicAdd(&sum[3 * (size_t)d0 + a], s[a]);
                atomicMin(&blo[3 * (size_t)d0 + a], lo[a]);
                atomicMax(&bhi[3 * (size_t)d0 + a], hi[a]);
            }
        }
    } else if (valid) {
        atomicAdd(&size[d], 1u);
        for (int a = 0; a < 3; ++a) {
            atomicAdd(&sum[3 * (size_t)d + a], (unsigned long long)v[a]);
            atomicMin(&blo[3 * (size_t)d + a], v[a]);
            atomicMax(&bhi[3 * (size_t)d + a], v[a]);
        }
    }
}

// cnt[2]: the clusters reported.  A dropped component sorts behind every reported one.
__global__ __launch_bounds__(256) void fr_key_kernel(uint32_t n_roots, uint32_t min_size, const uint32_t* __restrict__ size, const uint32_t* __restrict__ first,
                                                     uint64_t* __restrict__ key, uint32_t* __restrict__ idx, unsigned long long* __restrict__ cnt) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    bool reported = false;
    if (d < n_roots) {
        reported = size[d] >= min_size;
        key[d] = reported ? fr_order_key(size[d], first[d]) : ~0ull;
        idx[d] = d;
    }
    const unsigned long long m = __ballot(reported);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(&cnt[2], (unsigned long long)__popcll(m));
}

// idx: the dense numbers in key order; the first n_clusters of them are the clusters
__global__ __launch_bounds__(256) void fr_number_kernel(uint32_t n_roots, uint32_t n_clusters, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ size,
                                                        const uint32_t* __restrict__ first, const unsigned long long* __restrict__ sum,
                                                        const int32_t* __restrict__ blo, const int32_t* __restrict__ bhi, int32_t* __restrict__ number,
                                                        lv_frontier_cluster* __restrict__ clusters, unsigned long long* __restrict__ best) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_roots) return;
    const uint32_t d = idx[r];
    number[d] = r < n_clusters ? (int32_t)r : FR_NONE;
    if (r >= n_clusters) return;
    const uint64_t s[3] = {sum[3 * (size_t)d], sum[3 * (size_t)d + 1], sum[3 * (size_t)d + 2]};
    lv_frontier_cluster c;
    fr_cluster_record(c, size[d], first[d], s, blo + 3 * (size_t)d, bhi + 3 * (size_t)d);
    clusters[r] = c;
    best[r] = ~0ull;
}

// One 64-bit atomicMin per wavefront where the wavefront bids for one cluster, otherwise one per lane.  Every lane of the
// wavefront calls it; a lane without a bid passes valid = false.
__device__ __forceinline__ void fr_bid(unsigned long long* best, bool valid, int32_t lab, unsigned long long bid) {
    const unsigned long long vm = __ballot(valid);
    if (!vm) return;
    const int src = __ffsll((long long)vm) - 1;
    const int32_t lab0 = __shfl(lab, src);
    if (__ballot(valid && lab != lab0) == 0) {
        const unsigned long long b = wave_min(valid ? bid : ~0ull);
        if ((int)(threadIdx.x & 63u) == src && b != ~0ull) atomicMin(&best[lab0], b);
    } else if (valid && bid != ~0ull) {
        atomicMin(&best[lab], bid);
    }
}

__global__ __launch_bounds__(256) void fr_label_kernel(FrontierGrid g, uint32_t n, const uint32_t* __restrict__ root, const uint32_t* __restrict__ parent,
                                                       const int32_t* __restrict__ number, const lv_frontier_cluster* __restrict__ clusters,
                                                       int32_t* __restrict__ labels, unsigned long long* __restrict__ best) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t lab = FR_NONE;
    unsigned long long bid = ~0ull;
    if (c < n) {
        const uint32_t r = root[c];
        if (r != CL_NONE) lab = number[parent[r]];
        labels[c] = lab;
        if (lab >= 0) {
            int i, j, k;
            fr_cell_ijk(g, c, i, j, k);
            bid = fr_rep_key(clusters[lab].centre, i, j, k, c);
        }
    }
    fr_bid(best, lab >= 0, lab, bid);
}

__global__ __launch_bounds__(256) void fr_rep_kernel(uint32_t n_clusters, const unsigned long long* __restrict__ best, lv_frontier_cluster* __restrict__ clusters) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_clusters) clusters[r].rep = (int32_t)(uint32_t)best[r];
}

__global__ __launch_bounds__(256) void fr_rank_kernel(FrontierGrid g, uint32_t n, const int32_t* __restrict__ labels, const uint32_t* __restrict__ pot, int reach,
                                                      unsigned long long* __restrict__ best) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lab = c < n ? labels[c] : FR_NONE;
    unsigned long long bid = ~0ull;
    if (lab >= 0) {
        int i, j, k;
        fr_cell_ijk(g, c, i, j, k);
        bid = fr_rank_window(g, pot, reach, i, j, k);
    }
    fr_bid(best, lab >= 0, lab, bid);
}

}  // namespace

void FrontierStore::drop_scratch() {
    d_parent.release();
    d_root.release();
}

void FrontierStore::release() {
    drop_scratch();
    d_labels.release(); d_first.release(); d_size.release(); d_sum.release(); d_lohi.release(); d_key.release(); d_key2.release();
    d_idx.release(); d_idx2.release(); d_number.release(); d_tmp.release(); d_clusters.release(); d_best.release(); h_best.release();
    d_cnt.release(); h_cnt.release(); stats.release();
    *this = FrontierStore();
}

int FrontierStore::build(hipStream_t stream, const OccStore& occ, const lv_frontier_params& p, uint64_t out[4]) {
    FrontierGrid g{};
    g.nx = occ.grid.nx;
    g.ny = occ.grid.ny;
    g.nz = p.planar ? 1 : occ.grid.nz;
    g.planar = p.planar != 0;
    g.max_m = plan_max_m(p.connectivity);
    const size_t nc = grid_cells(g);
    const uint32_t n = (uint32_t)nc;
    int k0, k1;
    grid_clip_band(p.k_lo, p.k_hi, occ.grid.nz, k0, k1);
    const int tx = g.planar ? FR_PX : FR_VX, ty = g.planar ? FR_PY : FR_VY, tz = g.planar ? FR_PZ : FR_VZ;
    const size_t nt = g.planar ? HaloTile<FR_PX, FR_PY, FR_PZ>::tiles(g) : HaloTile<FR_VX, FR_VY, FR_VZ>::tiles(g);
    LV_HIP(hipStreamSynchronize(stream));   // (the pinned words below are free)
    built = false;   // (before a buffer goes: the old result's are overwritten from here on)
    n_clusters = 0;
    int rc = d_labels.need(nc);
    if (!rc) rc = d_parent.need(nc);
    if (!rc) rc = d_root.need(nc);
    if (!rc) rc = d_cnt.need(4);
    if (!rc) rc = h_cnt.need(4);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(d_cnt, 0, 4 * sizeof(unsigned long long), stream));
    const auto tile_kernel = g.planar ? fr_tile_kernel<FR_PX, FR_PY, FR_PZ> : fr_tile_kernel<FR_VX, FR_VY, FR_VZ>;
    hipLaunchKernelGGL(tile_kernel, dim3((uint32_t)nt), dim3(256), 0, stream, occ.d_L, g, k0, k1, occ.prm.l_free, occ.prm.l_occ, d_parent, stats.d);
    hipLaunchKernelGGL(fr_seam_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, g, tx, ty, tz, n, d_parent);
    hipLaunchKernelGGL(fr_flatten_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, n, d_parent, d_root, d_cnt);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(h_cnt, d_cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    const size_t nr = (size_t)h_cnt[0];
    size_t C = 0;
    if (nr == 0) {
        LV_HIP(hipMemsetAsync(d_labels, 0xFF, nc * sizeof(int32_t), stream));
    } else {
        rc = d_first.need(nr);
        if (!rc) rc = d_size.need(nr);
        if (!rc) rc = d_sum.need(3 * nr);
        if (!rc) rc = d_lohi.need(6 * nr);
        if (!rc) rc = d_key.need(nr);
        if (!rc) rc = d_key2.need(nr);
        if (!rc) rc = d_idx.need(nr);
        if (!rc) rc = d_idx2.need(nr);
        if (!rc) rc = d_number.need(nr);
        if (rc) return rc;
        size_t bytes = 0;
        LV_HIP((hipError_t)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, d_key.p, d_key2.p, d_idx.p, d_idx2.p, (int)nr, 0, 64, stream));
        rc = d_tmp.need(bytes);
        if (rc) return rc;
        LV_HIP(hipMemsetAsync(d_size, 0, nr * sizeof(uint32_t), stream));
        LV_HIP(hipMemsetAsync(d_sum, 0, 3 * nr * sizeof(unsigned long long), stream));
        // lo starts above every coordinate (0x7F7F7F7F), hi at 0: coordinates are 0..1023
        LV_HIP(hipMemsetAsync(d_lohi, 0x7F, 3 * nr * sizeof(int32_t), stream));
        LV_HIP(hipMemsetAsync(d_lohi + 3 * nr, 0, 3 * nr * sizeof(int32_t), stream));
        hipLaunchKernelGGL(fr_assign_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, n, d_root, d_parent, d_first, d_cnt);
        hipLaunchKernelGGL(fr_accumulate_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, g, n, d_root, d_parent, d_size, d_sum, d_lohi, d_lohi + 3 * nr);
        hipLaunchKernelGGL(fr_key_kernel, dim3(blocks_of(nr)), dim3(256), 0, stream, (uint32_t)nr, (uint32_t)p.min_size, d_size, d_first, d_key, d_idx, d_cnt);
        LV_HIP(hipGetLastError());
        LV_HIP((hipError_t)hipcub::DeviceRadixSort::SortPairs(d_tmp.p, bytes, d_key.p, d_key2.p, d_idx.p, d_idx2.p, (int)nr, 0, 64, stream));
        LV_HIP(hipMemcpyAsync(h_cnt, d_cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        C = (size_t)h_cnt[2];
        rc = d_clusters.need(C);
        if (!rc) rc = d_best.need(C);
        if (rc) return rc;
        hipLaunchKernelGGL(fr_number_kernel, dim3(blocks_of(nr)), dim3(256), 0, stream, (uint32_t)nr, (uint32_t)C, d_idx2, d_size, d_first, d_sum, d_lohi, d_lohi + 3 * nr,
                           d_number, d_clusters, d_best);
        hipLaunchKernelGGL(fr_label_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, g, n, d_root, d_parent, d_number, d_clusters, d_labels, d_best);
        if (C) hipLaunchKernelGGL(fr_rep_kernel, dim3(blocks_of(C)), dim3(256), 0, stream, (uint32_t)C, d_best, d_clusters);
        LV_HIP(hipGetLastError());
    }
    uint64_t st[4];
    rc = stats.read(stream, st);   // (waits for the stream)
    if (rc) return rc;
    drop_scratch();
    st[3] = (uint64_t)C;
    if (out) std::memcpy(out, st, sizeof st);
    prm = p;
    grid = g;
    n_cells = nc;
    n_clusters = C;
    stale = 0;
    built = true;
    return LV_OK;
}

int FrontierStore::fetch(hipStream_t stream, int32_t* labels) {
    LV_HIP(hipMemcpyAsync(labels, d_labels, n_cells * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int FrontierStore::clusters(hipStream_t stream, lv_frontier_cluster* out) {
    if (n_clusters) LV_HIP(hipMemcpyAsync(out, d_clusters, n_clusters * sizeof(lv_frontier_cluster), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int FrontierStore::rank(hipStream_t stream, const PlanStore& plan, int reach, uint32_t* best_p, int32_t* best_cell) {
    const size_t C = n_clusters;
    if (C == 0) return LV_OK;
    LV_HIP(hipStreamSynchronize(stream));   // (h_best is free)
    int rc = h_best.need(C);
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(d_best, 0xFF, C * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(fr_rank_kernel, dim3(blocks_of(n_cells)), dim3(256), 0, stream, grid, (uint32_t)n_cells, d_labels, plan.d_pot, reach, d_best);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(h_best, d_best, C * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    for (size_t c = 0; c < C; ++c) {   // FR_RANK_NONE unpacks to LV_PLAN_UNREACHED and -1
        if (best_p) best_p[c] = (uint32_t)(h_best[c] >> 32);
        if (best_cell) best_cell[c] = (int32_t)(uint32_t)h_best[c];
    }
    return LV_OK;
}

}  // namespace lv
