// lv_elevation.hip — the elevation map and the traversability class per cell (include/limovelo_hip.h "Elevation map"; the rule's
// code is lv_elevation.hpp).
//
// One build is three kernels (and the fold of their partials) on the context's stream:
//   elev_low_kernel      one lane per source point (a map id tested with pt_alive as lv_paint.hip does, or a staged caller
//                        point): elev_point, then an integer atomicMin into lo and an atomicAdd into n of its cell.
//   elev_band_kernel     the same sweep again, against the now final lo: elev_in_band, then atomicMax into top and atomicAdd into
//                        nb.  The used and overhang counts are folded per wavefront (wave_add_to).
//   elev_terrain_kernel  one workgroup per 32 x 8 tile, one lane per cell: lo of the tile and of its one-cell halo goes to LDS
//                        (34 consecutive words per row: a wavefront's two rows read and write without a bank conflict), with
//                        ELEV_NONE standing for "outside the grid or not known" (a known cell's lo is below 2^24, so one word
//                        carries both lo and known); then elev_terrain, elev_class, elev_height and five coalesced stores per
//                        cell.  The known and lethal counts go through block_fold4 into one partial record per workgroup.
//   elev_stats_kernel    one workgroup folds the partial records (lv_distance.hip measured why: atomics on a few addresses from
//                        every workgroup cost more than the passes).
// Integer min, max and add commute: the result does not depend on the order of the points or of the lanes.  No float atomics.
// lv_elev_query is one lane per point; lv_elev_fetch copies a layer.
#include "lv_elevation.hpp"

#include <cstring>

#include "lv_host.hpp"

namespace lv {

namespace {

// source point i: a living map point (MAP) or packed caller point; false: nothing there
template <bool MAP>
__device__ __forceinline__ bool elev_source(const void* __restrict__ src, uint32_t i, float p[3]) {
    if (MAP) {
        const float4 q = static_cast<const float4*>(src)[i];
        if (!pt_alive(q)) return false;
        p[0] = q.x;
        p[1] = q.y;
        p[2] = q.z;
    } else {
        const float* q = static_cast<const float*>(src) + 3 * (size_t)i;
        p[0] = q[0];
        p[1] = q[1];
        p[2] = q[2];
    }
    return true;
}

template <bool MAP>
__global__ __launch_bounds__(256) void elev_low_kernel(const void* __restrict__ src, uint32_t n, ElevGrid g, int32_t* __restrict__ lo,
                                                       uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float p[3];
    uint32_t cell;
    int32_t z;
    if (!elev_source<MAP>(src, i, p) || !elev_point(g, p, cell, z)) return;
    atomicMin(lo + cell, z);
    atomicAdd(cnt + cell, 1u);
}

// stats[0] += used points, stats[1] += overhang points
template <bool MAP>
__global__ __launch_bounds__(256) void elev_band_kernel(const void* __restrict__ src, uint32_t n, ElevGrid g, const int32_t* __restrict__ lo,
                                                        int32_t* __restrict__ top, uint32_t* __restrict__ nb, unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t used = 0, over = 0;
    float p[3];
    uint32_t cell;
    int32_t z;
    if (i < n && elev_source<MAP>(src, i, p) && elev_point(g, p, cell, z)) {
        used = 1;
        if (elev_in_band(z, lo[cell], g.head)) {
            atomicMax(top + cell, z);
            atomicAdd(nb + cell, 1u);
        } else {
            over = 1;
        }
    }
    wave_add_to(stats + 0, used);
    wave_add_to(stats + 1, over);
}

// what elev_terrain reads its neighbours through: the tile in LDS
struct ElevTileView {
    const int32_t* sh;
    int at;
    __device__ int32_t operator()(int di, int dj) const { return sh[at + dj * ElevTile::LX + di]; }
};

// part: per workgroup known cells, lethal cells, 0, 0
__global__ __launch_bounds__(256) void elev_terrain_kernel(ElevGrid g, const int32_t* __restrict__ lo, const int32_t* __restrict__ top,
                                                           const uint32_t* __restrict__ nb, int32_t* __restrict__ span, int32_t* __restrict__ step,
                                                           int32_t* __restrict__ slope2, int8_t* __restrict__ cls, float* __restrict__ height,
                                                           unsigned long long* __restrict__ part) {
    using T = ElevTile;
    __shared__ int32_t sh_lo[T::LCELLS];
    __shared__ unsigned long long sh[4][4];
    int tx, ty, tz;
    T::origin_of(g, blockIdx.x, tx, ty, tz);
    const int i0 = tx * ELEV_TX, j0 = ty * ELEV_TY;
    for (int l = threadIdx.x; l < T::LCELLS; l += 256) {
        int di, dj, dk;
        T::halo_of(l, di, dj, dk);
        const int i = i0 + di, j = j0 + dj;
        int32_t v = ELEV_NONE;
        if (grid_inside(g, i, j, 0)) {
            const size_t c = grid_at(g, i, j, 0);
            if (elev_known(nb[c], g.min_points)) v = lo[c];
        }
        sh_lo[l] = v;
    }
    __syncthreads();
    int li, lj, lk;
    T::local_of((int)threadIdx.x, li, lj, lk);
    const int i = i0 + li, j = j0 + lj;
    unsigned long long kn = 0, le = 0;
    if (grid_inside(g, i, j, 0)) {
        const size_t c = grid_at(g, i, j, 0);
        const ElevTileView view{sh_lo, T::at(li, lj, 0)};
        const int32_t lo0 = view(0, 0);
        const bool known = lo0 != ELEV_NONE;
        int32_t sp = 0, st = 0, s2 = 0;
        if (known) {
            sp = top[c] - lo0;
            elev_terrain(lo0, view, st, s2);
        }
        const int k = elev_class(known, sp, st, s2, g);
        span[c] = sp;
        step[c] = st;
        slope2[c] = s2;
        cls[c] = (int8_t)k;
        height[c] = elev_height(known, lo0, g.origin[2], g.resolution);
        kn = known;
        le = k == 100;
    }
    unsigned long long a;
    if (block_fold4(sh, kn, le, 0ull, 0ull, a)) part[(size_t)blockIdx.x * 4 + threadIdx.x] = a;
}

// one workgroup of 1024: the n_blocks partial records of elev_terrain_kernel into stats[2], stats[3]
__global__ __launch_bounds__(1024) void elev_stats_kernel(const unsigned long long* __restrict__ part, uint32_t n_blocks, unsigned long long* stats) {
    __shared__ unsigned long long sh[16][4];
    unsigned long long kn = 0, le = 0;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += 1024u) {
        kn += part[(size_t)b * 4];
        le += part[(size_t)b * 4 + 1];
    }
    unsigned long long a;
    if (block_fold4(sh, kn, le, 0ull, 0ull, a) && threadIdx.x < 2) stats[2 + threadIdx.x] = a;
}

// out_h / out_c: NULL or n entries
__global__ __launch_bounds__(256) void elev_query_kernel(const float* __restrict__ pts, uint32_t n, ElevGrid g, const float* __restrict__ height,
                                                         const int8_t* __restrict__ cls, float* __restrict__ out_h, int8_t* __restrict__ out_c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    uint32_t cell;
    const bool in = elev_query_cell(g, p, cell);
    if (out_h) out_h[i] = in ? height[cell] : __uint_as_float(0x7FC00000u);
    if (out_c) out_c[i] = in ? cls[cell] : (int8_t)-1;
}

}  // namespace

void ElevStore::release() {
    d_lo.release(); d_top.release(); d_span.release(); d_step.release(); d_slope2.release(); d_n.release(); d_nb.release(); d_cls.release();
    d_height.release(); d_part.release(); stats.release(); pts.release(); d_qh.release(); d_qc.release();
    *this = ElevStore();
}

int ElevStore::build(hipStream_t stream, const lv_elevation_params& p, const float4* map_orig, uint32_t n_ids, uint64_t n_living, const void* points,
                     size_t stride, size_t n, uint64_t out[4]) {
    const ElevGrid g = elev_grid_of(p);
    const size_t nc = grid_cells(g);
    const uint32_t tiles = (uint32_t)ElevTile::tiles(g);
    const bool from = points == nullptr;
    int rc = pts.reserve(stream, from ? 0 : n);   // (synchronises the stream)
    built = false;   // (before a buffer goes, and until the kernels are through)
    if (!rc) rc = d_lo.need(nc);
    if (!rc) rc = d_top.need(nc);
    if (!rc) rc = d_span.need(nc);
    if (!rc) rc = d_step.need(nc);
    if (!rc) rc = d_slope2.need(nc);
    if (!rc) rc = d_n.need(nc);
    if (!rc) rc = d_nb.need(nc);
    if (!rc) rc = d_cls.need(nc);
    if (!rc) rc = d_height.need(nc);
    if (!rc) rc = d_part.need((size_t)tiles * 4);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    if (!from) {
        pts.append(points, stride, n);
        rc = pts.upload(stream);
        if (rc) return rc;
    }
    // every layer of the cells in use starts from "no point": the buffers may be a larger build's
    LV_HIP(hipMemsetD32Async((hipDeviceptr_t)d_lo.p, ELEV_NONE, nc, stream));
    LV_HIP(hipMemsetD32Async((hipDeviceptr_t)d_top.p, -ELEV_NONE, nc, stream));
    LV_HIP(hipMemsetAsync(d_n.p, 0, nc * sizeof(uint32_t), stream));
    LV_HIP(hipMemsetAsync(d_nb.p, 0, nc * sizeof(uint32_t), stream));
    const uint32_t ns = from ? n_ids : (uint32_t)n;
    if (ns) {
        if (from) {
            hipLaunchKernelGGL(elev_low_kernel<true>, dim3(blocks_of(ns)), dim3(256), 0, stream, map_orig, ns, g, d_lo.p, d_n.p);
            hipLaunchKernelGGL(elev_band_kernel<true>, dim3(blocks_of(ns)), dim3(256), 0, stream, map_orig, ns, g, d_lo.p, d_top.p, d_nb.p, stats.d.p);
        } else {
            hipLaunchKernelGGL(elev_low_kernel<false>, dim3(blocks_of(ns)), dim3(256), 0, stream, pts.d.p, ns, g, d_lo.p, d_n.p);
            hipLaunchKernelGGL(elev_band_kernel<false>, dim3(blocks_of(ns)), dim3(256), 0, stream, pts.d.p, ns, g, d_lo.p, d_top.p, d_nb.p, stats.d.p);
        }
    }
    hipLaunchKernelGGL(elev_terrain_kernel, dim3(tiles), dim3(256), 0, stream, g, d_lo.p, d_top.p, d_nb.p, d_span.p, d_step.p, d_slope2.p, d_cls.p,
                       d_height.p, d_part.p);
    hipLaunchKernelGGL(elev_stats_kernel, dim3(1), dim3(1024), 0, stream, d_part.p, tiles, stats.d.p);
    LV_HIP(hipGetLastError());
    rc = stats.read(stream, out);
    if (rc) return rc;
    prm = p;
    grid = g;
    n_cells = nc;
    from_map = from ? 1 : 0;
    n_points = from ? n_living : (uint64_t)n;
    built = true;
    return LV_OK;
}

int ElevStore::fetch(hipStream_t stream, int layer, void* out) {
    const void* src = nullptr;
    switch (layer) {
        case LV_ELEV_LO: src = d_lo.p; break;
        case LV_ELEV_TOP: src = d_top.p; break;
        case LV_ELEV_SPAN: src = d_span.p; break;
        case LV_ELEV_STEP: src = d_step.p; break;
        case LV_ELEV_SLOPE2: src = d_slope2.p; break;
        case LV_ELEV_COUNT: src = d_n.p; break;
        case LV_ELEV_BAND_COUNT: src = d_nb.p; break;
        case LV_ELEV_CLASS: src = d_cls.p; break;
        default: src = d_height.p; break;
    }
    LV_HIP(hipMemcpyAsync(out, src, n_cells * elev_layer_size(layer), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int ElevStore::query(hipStream_t stream, const void* points, size_t stride, size_t n, float* height, int8_t* cls) {
    if (n == 0) return LV_OK;
    int rc = pts.reserve(stream, n);
    if (!rc && height) rc = d_qh.need(n);
    if (!rc && cls) rc = d_qc.need(n);
    if (rc) return rc;
    pts.append(points, stride, n);
    rc = pts.upload(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(elev_query_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, pts.d.p, (uint32_t)n, grid, d_height.p, d_cls.p,
                       height ? d_qh.p : nullptr, cls ? d_qc.p : nullptr);
    LV_HIP(hipGetLastError());
    if (height) LV_HIP(hipMemcpyAsync(height, d_qh.p, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (cls) LV_HIP(hipMemcpyAsync(cls, d_qc.p, n, hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
