// lv_distance.hip — the Euclidean distance field over the occupancy grid (include/limovelo_hip.h "Distance field"; the rule's code
// is lv_distance.hpp).
//
// One build is five kernels on the context's stream, every one with its lanes along x so that each load and store of a wavefront is
// one contiguous run of a row:
//   dist_classify_kernel  one wavefront per 64 consecutive x of a row: the obstacle test per lane (the planar field projects its
//                         band of layers: grid_project_column), one __ballot, two words of the one-bit-per-voxel bitmap (the occupancy bitmaps' layout).
//                         dist_classify_cells_kernel is the same over the caller's plane of cells (lv_occ_distance_build_cells): it
//                         writes the same bitmap, and everything after it is shared.
//   dist_x_kernel         one lane per voxel: the nearest set bit of its row (the nearest clear one for an obstacle of a signed
//                         field) by clz / ctz over the row's at most 32 words, which sit in L2.  Writes +-dx^2, +-FAR or 0.
//   dist_y_kernel         one lane per voxel: dist_pass_line along y (stride nx).  The wavefront's neighbours in x read the
//                         neighbouring words, so every step of the outward scan is a coalesced load.
//   dist_z_kernel         the same along z (stride nx * ny), then truncation and the stats: sums and maxima folded per workgroup
//                         (block_fold4), one partial record per workgroup.
//   dist_stats_kernel     one workgroup folds the partial records (integer sums and maxima: the order does not matter).  One
//                         atomic per wavefront on the four counters instead was measured: the atomics on four addresses took
//                         6.3 of the 9.7 ms of a build of the default grid.
// The inside transform of a signed field rides in the same passes (lv_distance.hpp), so signed costs what unsigned costs.
// lv_occ_distance_query is a one-lane-per-point kernel; the metres of lv_occ_distance_fetch one lane per voxel into the Y pass's buffer.
#include "lv_distance.hpp"

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

struct DistOrigin {
    float o[3];
};

// n_waves = rows * ceil(nx / 64); planar: L is the whole grid, k0..k1 the clipped band; otherwise the row is the voxel row
__global__ __launch_bounds__(256) void dist_classify_kernel(const float* __restrict__ L, DistGrid g, int planar, int k0, int k1, float l_occ,
                                                            float l_free, int unknown, uint32_t n_waves, uint32_t* __restrict__ bits) {
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wave >= n_waves) return;   // (whole wavefronts leave together)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t per_row = ((uint32_t)g.nx + 63u) / 64u;
    const uint32_t row = wave / per_row, seg = wave - row * per_row;
    const uint32_t i = seg * 64u + lane;
    bool ob = false;
    if (i < (uint32_t)g.nx) {
        if (planar) ob = dist_obstacle_planar(L, (size_t)g.nx * (size_t)g.ny, (size_t)row * (size_t)g.nx + i, k0, k1, l_occ, l_free, unknown != 0);
        else ob = dist_obstacle(L[(size_t)row * (size_t)g.nx + i], l_occ, unknown != 0);
    }
    const unsigned long long m = __ballot(ob);
    const uint32_t word = seg * 2u + (lane >> 5);
    if ((lane & 31u) == 0 && word < (uint32_t)g.wx) bits[(size_t)row * (size_t)g.wx + word] = (uint32_t)(m >> (lane & 32u));
}

// the wavefront's ballot into its two words of the bitmap
__device__ __forceinline__ void dist_store_ballot(bool ob, const DistGrid& g, uint32_t row, uint32_t seg, uint32_t lane, uint32_t* __restrict__ bits) {
    const unsigned long long m = __ballot(ob);
    const uint32_t word = seg * 2u + (lane >> 5);
    if ((lane & 31u) == 0 && word < (uint32_t)g.wx) bits[(size_t)row * (size_t)g.wx + word] = (uint32_t)(m >> (lane & 32u));
}

// n_waves = ny * ceil(nx / 64); cells: the caller's plane, index j * nx + i
__global__ __launch_bounds__(256) void dist_classify_cells_kernel(const int8_t* __restrict__ cells, DistGrid g, int unknown, uint32_t n_waves,
                                                                  uint32_t* __restrict__ bits) {
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wave >= n_waves) return;   // (whole wavefronts leave together)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t per_row = ((uint32_t)g.nx + 63u) / 64u;
    const uint32_t row = wave / per_row, seg = wave - row * per_row;
    const uint32_t i = seg * 64u + lane;
    const bool ob = i < (uint32_t)g.nx && dist_obstacle_cell(cells[(size_t)row * (size_t)g.nx + i], unknown != 0);
    dist_store_ballot(ob, g, row, seg, lane, bits);
}

__global__ __launch_bounds__(256) void dist_x_kernel(const uint32_t* __restrict__ bits, DistGrid g, uint32_t n, int32_t* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t row = v / (uint32_t)g.nx;
    out[v] = dist_pass_x(g, bits + (size_t)row * (size_t)g.wx, (int)(v - row * (uint32_t)g.nx));
}

__global__ __launch_bounds__(256) void dist_y_kernel(const int32_t* __restrict__ in, DistGrid g, uint32_t n, int32_t* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int i, j, k;
    grid_ijk(g, v, i, j, k);
    out[v] = dist_pass_line(in + grid_at(g, i, 0, k), (size_t)g.nx, g.ny, j, g.reach);
}

// part: per workgroup obstacles, finite values, largest finite d2_out, largest finite d2_in
__global__ __launch_bounds__(256) void dist_z_kernel(const int32_t* __restrict__ in, DistGrid g, int max_cells, uint32_t n, int32_t* __restrict__ out,
                                                     unsigned long long* __restrict__ part) {
    __shared__ unsigned long long sh[4][4];
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long ob = 0, fin = 0, mo = 0, mi = 0;
    if (v < n) {
        const uint32_t plane = (uint32_t)g.nx * (uint32_t)g.ny;
        const uint32_t k = v / plane, r = v - k * plane;
        const int32_t s = dist_truncate(dist_pass_line(in + r, (size_t)plane, g.nz, (int)k, g.reach), max_cells);
        out[v] = s;
        ob = s <= 0;
        if (s != DIST_FAR && s != -DIST_FAR) {
            fin = 1;
            if (s > 0) mo = (unsigned long long)s;
            else mi = (unsigned long long)(-s);
        }
    }
    unsigned long long a;
    if (block_fold4(sh, ob, fin, mo, mi, a)) part[(size_t)blockIdx.x * 4 + threadIdx.x] = a;
}

// one workgroup of 1024: the n_blocks partial records of dist_z_kernel into stats[4]
__global__ __launch_bounds__(1024) void dist_stats_kernel(const unsigned long long* __restrict__ part, uint32_t n_blocks, unsigned long long* stats) {
    __shared__ unsigned long long sh[16][4];
    unsigned long long ob = 0, fin = 0, mo = 0, mi = 0;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += 1024u) {
        ob += part[(size_t)b * 4];
        fin += part[(size_t)b * 4 + 1];
        const unsigned long long o = part[(size_t)b * 4 + 2], i = part[(size_t)b * 4 + 3];
        mo = o > mo ? o : mo;
        mi = i > mi ? i : mi;
    }
    unsigned long long a;
    if (block_fold4(sh, ob, fin, mo, mi, a)) stats[threadIdx.x] = a;
}

__global__ __launch_bounds__(256) void dist_metres_kernel(const int32_t* __restrict__ s2, float resolution, uint32_t n, float* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) out[v] = dist_metres(s2[v], resolution);
}

// out: n dist values, then (with_grad) 3 * n gradient components
__global__ __launch_bounds__(256) void dist_query_kernel(const int32_t* __restrict__ s2, DistGrid g, DistOrigin origin, int planar,
                                                         const float* __restrict__ pts, uint32_t n, int with_grad, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    float d, gr[3];
    dist_query_point(g, origin.o, planar != 0, s2, p, &d, with_grad ? gr : nullptr);
    out[i] = d;
    if (with_grad) {
        float* dst = out + (size_t)n + 3 * (size_t)i;
        dst[0] = gr[0];
        dst[1] = gr[1];
        dst[2] = gr[2];
    }
}

}  // namespace

void DistStore::release() {
    d_s2.release(); d_tmp.release(); d_bits.release(); d_part.release(); stats.release(); pts.release(); d_out.release(); d_cells.release();
    *this = DistStore();
}

int DistStore::build(hipStream_t stream, const OccStore& occ, const lv_distance_params& p, const int8_t* cells, uint64_t out[4]) {
    const DistGrid g = dist_grid_of(occ.grid, p);
    const size_t nv = grid_cells(g);
    const size_t nw = (size_t)g.wx * (size_t)g.ny * (size_t)g.nz;
    LV_HIP(hipStreamSynchronize(stream));
    built = false;   // (before a buffer goes, and until the passes are through)
    int rc = d_s2.need(nv);
    if (!rc) rc = d_tmp.need(nv);
    if (!rc) rc = d_bits.need(nw);
    if (!rc) rc = d_part.need((size_t)blocks_of(nv) * 4);
    if (!rc) rc = stats.need();
    if (!rc && cells) rc = d_cells.need(nv);
    if (rc) return rc;
    int k0, k1;
    grid_clip_band(p.k_lo, p.k_hi, occ.grid.nz, k0, k1);
    const size_t rows = (size_t)g.ny * (size_t)g.nz;
    const uint32_t n_waves = (uint32_t)(rows * (((size_t)g.nx + 63) / 64));
    if (cells) {
        // (from the caller's pageable memory: the copy has left it when the call returns, which the read of the stats waits for)
        LV_HIP(hipMemcpyAsync(d_cells.p, cells, nv, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(dist_classify_cells_kernel, dim3((n_waves + 3) / 4), dim3(256), 0, stream, d_cells.p, g, p.unknown_is_obstacle != 0,
                           n_waves, d_bits);
    } else {
        hipLaunchKernelGGL(dist_classify_kernel, dim3((n_waves + 3) / 4), dim3(256), 0, stream, occ.d_L, g, p.planar != 0, k0, k1, occ.prm.l_occ,
                           occ.prm.l_free, p.unknown_is_obstacle != 0, n_waves, d_bits);
    }
    hipLaunchKernelGGL(dist_x_kernel, dim3(blocks_of(nv)), dim3(256), 0, stream, d_bits, g, (uint32_t)nv, d_s2);
    hipLaunchKernelGGL(dist_y_kernel, dim3(blocks_of(nv)), dim3(256), 0, stream, d_s2, g, (uint32_t)nv, d_tmp);
    hipLaunchKernelGGL(dist_z_kernel, dim3(blocks_of(nv)), dim3(256), 0, stream, d_tmp, g, p.max_cells, (uint32_t)nv, d_s2, d_part);
    hipLaunchKernelGGL(dist_stats_kernel, dim3(1), dim3(1024), 0, stream, d_part, blocks_of(nv), stats.d);
    LV_HIP(hipGetLastError());
    rc = stats.read(stream, out);
    if (rc) return rc;
    prm = p;
    grid = g;
    for (int a = 0; a < 3; ++a) origin[a] = occ.grid.origin[a];
    n_vox = nv;
    stale = 0;
    built = true;
    return LV_OK;
}

int DistStore::fetch(hipStream_t stream, int32_t* s2, float* metres) {
    if (metres) {
        hipLaunchKernelGGL(dist_metres_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, d_s2, grid.resolution, (uint32_t)n_vox,
                           reinterpret_cast<float*>(d_tmp.p));
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(metres, d_tmp, n_vox * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    if (s2) LV_HIP(hipMemcpyAsync(s2, d_s2, n_vox * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int DistStore::query(hipStream_t stream, const void* points, size_t stride, size_t n, float* dist, float* grad) {
    if (n == 0) return LV_OK;
    int rc = pts.reserve(stream, n);
    if (!rc) rc = d_out.need(4 * n);
    if (rc) return rc;
    pts.append(points, stride, n);
    rc = pts.upload(stream);
    if (rc) return rc;
    DistOrigin o;
    std::memcpy(o.o, origin, sizeof(o.o));
    hipLaunchKernelGGL(dist_query_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_s2, grid, o, prm.planar != 0, pts.d, (uint32_t)n,
                       grad != nullptr, d_out);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(dist, d_out, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (grad) LV_HIP(hipMemcpyAsync(grad, d_out + n, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
