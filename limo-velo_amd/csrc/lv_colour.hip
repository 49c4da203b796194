// lv_colour.hip — the colour layer of the TSDF volume (include/limovelo_hip.h "Colour layer"; the rule's code is lv_colour.hpp,
// the projection and the sample lv_paint_dev.hpp's, shared with lv_map_paint).
//
// One lv_colour_integrate, on the context's stream:
//   colour_count_kernel   one lane per voxel, S and W read coalesced along x: a wave ballot of the candidate test, the workgroup's
//                         count to bcnt; then the exclusive sum mesh_build uses (tsdf_scan) over the workgroups;
//   colour_list_kernel    the same test again, every candidate's voxel index to its place: the list is in linear order whatever
//                         the schedule.  A call without candidates ends here;
//   paint_unpack_kernel   the staged image bytes to packed texels;
//   colour_zbuf_kernel    one lane per candidate: its centre, a loop over the views, atomicMin of the z bits into the centre's
//                         cell (an integer atomic, independent of order);
//   paint_min_x / _y      the window-min;
//   colour_fold_kernel    one lane per candidate: the loop over the views again through the same paint_project, n and dC kept in
//                         registers, then its voxel's entry read and written once as one 16-byte access.  No atomics but the
//                         stats': a wave sum, then one 64-bit add per workgroup and counter.
// The vertex colours (colour_vertex_kernel, inside lv_tsdf_mesh_build) run one lane per cell over the build's flags and vertex
// ids, as tsdf_vertex_kernel does, with eight 16-byte loads.  lv_volume_recentre gathers the layer into a second buffer
// (colour_shift_kernel), which then takes the first one's place.  Nothing here depends on the launch geometry.
#include "lv_colour.hpp"

#include <cstring>

#include "lv_paint_dev.hpp"

namespace lv {

namespace {

// the workgroup's sum of a per-lane flag, by ballot: in every lane after the barrier.  rank: the lane's place among the set lanes
__device__ __forceinline__ uint32_t block_ballot(bool pred, uint32_t (&sh)[4], uint32_t& rank) {
    const unsigned long long m = __ballot(pred ? 1 : 0);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    uint32_t total = 0;
    for (uint32_t w = 0; w < 4; ++w) {
        if (w < wave) rank += sh[w];
        total += sh[w];
    }
    return total;
}

// bcnt[workgroup] = its candidates; bcnt[gridDim.x] = 0 (the scan's total lands there)
__global__ __launch_bounds__(256) void colour_count_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, uint32_t n_vox,
                                                           int32_t min_weight, int32_t band, uint32_t* __restrict__ bcnt) {
    __shared__ uint32_t sh[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool cand = i < n_vox && colour_candidate(S[i], W[i], min_weight, band);
    uint32_t rank;
    const uint32_t total = block_ballot(cand, sh, rank);
    if (threadIdx.x == 0) {
        bcnt[blockIdx.x] = total;
        if (blockIdx.x == 0) bcnt[gridDim.x] = 0;
    }
}

// list[boff[workgroup] + rank] = voxel index of every candidate
__global__ __launch_bounds__(256) void colour_list_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, uint32_t n_vox,
                                                          int32_t min_weight, int32_t band, const uint32_t* __restrict__ boff, uint32_t n_cand,
                                                          uint32_t* __restrict__ list) {
    __shared__ uint32_t sh[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool cand = i < n_vox && colour_candidate(S[i], W[i], min_weight, band);
    uint32_t rank;
    block_ballot(cand, sh, rank);
    const uint32_t at = boff[blockIdx.x] + rank;
    if (cand && at < n_cand) list[at] = i;
}

__device__ __forceinline__ float4 colour_centre_of(const TsdfGrid& g, uint32_t vox) {
    int i, j, k;
    grid_ijk(g.occ, vox, i, j, k);
    return make_float4(colour_centre(g.occ.origin[0], g.occ.resolution, i), colour_centre(g.occ.origin[1], g.occ.resolution, j),
                       colour_centre(g.occ.origin[2], g.occ.resolution, k), 0.f);
}

// one lane per candidate; cell: every view's cells, initialised to +inf
__global__ __launch_bounds__(256) void colour_zbuf_kernel(const uint32_t* __restrict__ list, uint32_t n_cand, TsdfGrid g,
                                                          const PaintCam* __restrict__ cams, PaintRule q, uint32_t* __restrict__ cell) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cand) return;
    const float4 p = colour_centre_of(g, list[t]);
    for (int w = 0; w < q.n_views; ++w) {
        const PaintCam& c = cams[w];
        float z, u, v;
        if (!paint_project(c, q, p, z, u, v)) continue;
        atomicMin(&cell[paint_cell(c, q, u, v)], __float_as_uint(z));
    }
}

// One lane per candidate.  cell: the window-min occlusion buffers; layer: one uint4 (C[0], C[1], C[2], Wc) per voxel.
// stats[1] += pairs that pass steps 1 to 3, stats[2] += pairs seen, stats[3] += voxels with n > 0
__global__ __launch_bounds__(256) void colour_fold_kernel(const uint32_t* __restrict__ list, uint32_t n_cand, TsdfGrid g,
                                                          const PaintCam* __restrict__ cams, PaintRule q, const uint32_t* __restrict__ cell,
                                                          const uint32_t* __restrict__ tex, uint32_t max_weight, uint4* __restrict__ layer,
                                                          unsigned long long* stats) {
    __shared__ unsigned long long sh[4][3];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t pairs = 0, n = 0;
    if (t < n_cand) {
        const uint32_t vox = list[t];
        const float4 p = colour_centre_of(g, vox);
        uint32_t dC[3] = {0u, 0u, 0u};
        for (int w = 0; w < q.n_views; ++w) {
            const PaintCam& c = cams[w];
            float z, u, v;
            if (!paint_project(c, q, p, z, u, v)) continue;
            ++pairs;
            const float zw = __uint_as_float(cell[paint_cell(c, q, u, v)]);
            if (!(z - zw <= fmaxf(q.margin_abs, q.margin_rel * z))) continue;
            ++n;
            const float3 s = paint_sample(c, tex, u, v);
            dC[0] += colour_quant(s.x);
            dC[1] += colour_quant(s.y);
            dC[2] += colour_quant(s.z);
        }
        if (n > 0) {
            const uint4 a = layer[vox];
            uint32_t e[4] = {a.x, a.y, a.z, a.w};
            colour_fold(max_weight, n, dC, e);
            layer[vox] = make_uint4(e[0], e[1], e[2], e[3]);
        }
    }
    const unsigned long long v[3] = {wave_sum((unsigned long long)pairs), wave_sum((unsigned long long)n), wave_sum((unsigned long long)(n > 0 ? 1u : 0u))};
    if ((threadIdx.x & 63u) == 0)
        for (int c = 0; c < 3; ++c) sh[threadIdx.x >> 6][c] = v[c];
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long a = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (a) atomicAdd(stats + 1 + threadIdx.x, a);
    }
}

// one lane per cell, as tsdf_vertex_kernel: rgba[vertex of the cell] from its 8 corner voxels' entries
__global__ __launch_bounds__(256) void colour_vertex_kernel(const uint4* __restrict__ layer, GridDims g, uint32_t n_vox, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ vid, uint32_t n_vert, uint32_t* __restrict__ rgba) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_vox || !flag[cell]) return;
    int i, j, k;
    grid_ijk(g, cell, i, j, k);
    if (i > g.nx - 2 || j > g.ny - 2 || k > g.nz - 2) return;   // (an active cell never is: the corners stay inside the layer)
    uint32_t e[8][4];
    for (int n = 0; n < 8; ++n) {
        const uint4 a = layer[grid_at(g, i + (n & 1), j + ((n >> 1) & 1), k + (n >> 2))];
        e[n][0] = a.x; e[n][1] = a.y; e[n][2] = a.z; e[n][3] = a.w;
    }
    const uint32_t o = vid[cell];
    if (o < n_vert) rgba[o] = colour_vertex(e);
}

// dst[new voxel] = src[the voxel it takes after a recentre by (dx, dy, dz)], or four zeros
__global__ __launch_bounds__(256) void colour_shift_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, GridDims g, int32_t dx, int32_t dy,
                                                           int32_t dz, uint32_t n_vox) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_vox) return;
    int i, j, k, si, sj, sk;
    grid_ijk(g, c, i, j, k);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (grid_shift_source(g, dx, dy, dz, i, j, k, si, sj, sk)) v = src[grid_at(g, si, sj, sk)];
    dst[c] = v;
}

__global__ __launch_bounds__(256) void colour_rgba_kernel(const uint4* __restrict__ layer, uint32_t n_vox, uint32_t* __restrict__ rgba) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_vox) return;
    const uint4 a = layer[i];
    const uint32_t e[4] = {a.x, a.y, a.z, a.w};
    rgba[i] = colour_voxel(e);
}

__global__ __launch_bounds__(256) void colour_query_kernel(const uint4* __restrict__ layer, TsdfGrid g, const float* __restrict__ pts, uint32_t n,
                                                           uint32_t* __restrict__ rgba) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int ci, cj, ck;
    uint32_t out = 0u;
    if (grid_cell_of(g.occ, g.occ.origin, g.occ.resolution, false, pts + 3 * (size_t)i, ci, cj, ck)) {
        const uint4 a = layer[grid_at(g.occ, ci, cj, ck)];
        const uint32_t e[4] = {a.x, a.y, a.z, a.w};
        out = colour_voxel(e);
    }
    rgba[i] = out;
}

// stats[0] += the voxels with Wc > 0
__global__ __launch_bounds__(256) void colour_coloured_kernel(const uint4* __restrict__ layer, uint32_t n_vox, unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    wave_add_to(stats, i < n_vox && layer[i].w > 0u ? 1u : 0u);
}

inline uint4* layer_of(const ColourLayer& c) { return reinterpret_cast<uint4*>(c.d_sums.p); }

}  // namespace

int TsdfStore::colour_ensure(hipStream_t stream) {
    if (colour.present) return LV_OK;
    const int rc = colour.d_sums.need(4 * n_vox);
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(colour.d_sums, 0, 4 * n_vox * sizeof(uint32_t), stream));
    LV_HIP(hipStreamSynchronize(stream));
    colour.present = true;
    return LV_OK;
}

int TsdfStore::colour_clear(hipStream_t stream) {
    LV_HIP(hipMemsetAsync(colour.d_sums, 0, 4 * n_vox * sizeof(uint32_t), stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::colour_integrate(hipStream_t stream, const lv_camera_view* views, const PaintCam* cams, const PaintRule& q, int band, int min_weight,
                                int max_weight, uint64_t out[4]) {
    ColourLayer& c = colour;
    int rc = colour_ensure(stream);
    const uint32_t nb = blocks_of(n_vox);
    if (!rc) rc = c.d_bcnt.need((size_t)nb + 1);
    if (!rc) rc = c.d_boff.need((size_t)nb + 1);
    if (rc) return rc;
    const uint32_t nv = (uint32_t)n_vox;
    uint32_t n_cand = 0;
    hipLaunchKernelGGL(colour_count_kernel, dim3(nb), dim3(256), 0, stream, d_S.p, d_W.p, nv, min_weight, band, c.d_bcnt.p);
    LV_HIP(hipGetLastError());
    rc = tsdf_scan(stream, d_tmp, c.d_bcnt.p, c.d_boff.p, nb, &n_cand);   // (waits for the stream)
    if (rc) return rc;
    if (out) out[0] = out[1] = out[2] = out[3] = 0;
    if (n_cand == 0) return LV_OK;
    rc = c.d_list.need(n_cand);
    if (!rc) rc = c.d_raw.need(q.raw_bytes);
    if (!rc) rc = c.d_tex.need(q.total_pixels);
    if (!rc) rc = c.d_cell.need(q.total_cells);
    if (!rc && q.window > 0) rc = c.d_tmp.need(q.total_cells);
    if (!rc) rc = c.d_cams.need(PAINT_MAX_VIEWS);
    if (!rc) rc = c.h_cams.need(PAINT_MAX_VIEWS);   // (the stream is idle: the previous call's copies have left the pinned buffers)
    if (!rc) rc = c.h_raw.need(q.raw_bytes);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    paint_stage_images(views, cams, q, c.h_raw);
    std::memcpy(c.h_cams, cams, (size_t)q.n_views * sizeof(PaintCam));
    LV_HIP(hipMemcpyAsync(c.d_cams, c.h_cams, (size_t)q.n_views * sizeof(PaintCam), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(c.d_raw, c.h_raw, q.raw_bytes, hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetD32Async((hipDeviceptr_t)c.d_cell.p, 0x7F800000, q.total_cells, stream));
    hipLaunchKernelGGL(colour_list_kernel, dim3(nb), dim3(256), 0, stream, d_S.p, d_W.p, nv, min_weight, band, c.d_boff.p, n_cand, c.d_list.p);
    hipLaunchKernelGGL(paint_unpack_kernel, dim3(blocks_of(q.max_pixels), q.n_views), dim3(256), 0, stream, c.d_raw.p, c.d_cams.p, c.d_tex.p);
    hipLaunchKernelGGL(colour_zbuf_kernel, dim3(blocks_of(n_cand)), dim3(256), 0, stream, c.d_list.p, n_cand, grid, c.d_cams.p, q, c.d_cell.p);
    if (q.window > 0) {
        hipLaunchKernelGGL(paint_min_x_kernel, dim3(blocks_of(q.max_cells), q.n_views), dim3(256), 0, stream, c.d_cell.p, c.d_tmp.p, c.d_cams.p, q.window);
        hipLaunchKernelGGL(paint_min_y_kernel, dim3(blocks_of(q.max_cells), q.n_views), dim3(256), 0, stream, c.d_tmp.p, c.d_cell.p, c.d_cams.p, q.window);
    }
    hipLaunchKernelGGL(colour_fold_kernel, dim3(blocks_of(n_cand)), dim3(256), 0, stream, c.d_list.p, n_cand, grid, c.d_cams.p, q, c.d_cell.p, c.d_tex.p,
                       (uint32_t)max_weight, layer_of(c), stats.d.p);
    LV_HIP(hipGetLastError());
    uint64_t st[4];
    rc = stats.read(stream, st);   // (waits for the stream)
    if (rc) return rc;
    if (out) {
        out[0] = n_cand;
        out[1] = st[1];
        out[2] = st[2];
        out[3] = st[3];
    }
    return LV_OK;
}

int TsdfStore::colour_fetch(hipStream_t stream, uint32_t* sums, uint8_t* rgba) {
    if (rgba) {
        const int rc = colour.d_rgba.need(n_vox);
        if (rc) return rc;
        hipLaunchKernelGGL(colour_rgba_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, layer_of(colour), (uint32_t)n_vox, colour.d_rgba.p);
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(rgba, colour.d_rgba, n_vox * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    if (sums) LV_HIP(hipMemcpyAsync(sums, colour.d_sums, 4 * n_vox * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::colour_load(hipStream_t stream, const uint32_t* sums) {
    const int rc = colour_ensure(stream);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(colour.d_sums, sums, 4 * n_vox * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::colour_query(hipStream_t stream, const void* points, size_t stride, size_t n, uint8_t* rgba) {
    if (n == 0) return LV_OK;
    int rc = pts.reserve(stream, n);
    if (!rc) rc = colour.d_rgba.need(n);
    if (rc) return rc;
    pts.append(points, stride, n);
    rc = pts.upload(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(colour_query_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, layer_of(colour), grid, pts.d.p, (uint32_t)n, colour.d_rgba.p);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(rgba, colour.d_rgba, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::colour_count(hipStream_t stream, uint64_t* coloured) {
    int rc = stats.zero(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(colour_coloured_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, layer_of(colour), (uint32_t)n_vox, stats.d.p);
    LV_HIP(hipGetLastError());
    uint64_t st[4];
    rc = stats.read(stream, st);
    if (rc) return rc;
    *coloured = st[0];
    return LV_OK;
}

int TsdfStore::colour_shift(hipStream_t stream, const int32_t d[3]) {
    const GridDims g{grid.occ.nx, grid.occ.ny, grid.occ.nz};
    hipLaunchKernelGGL(colour_shift_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, layer_of(colour), reinterpret_cast<uint4*>(colour.d_next.p), g,
                       d[0], d[1], d[2], (uint32_t)n_vox);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int TsdfStore::colour_vertices(hipStream_t stream, const uint32_t* flag, const uint32_t* vid, uint32_t n_vert) {
    const int rc = mesh.d_rgba.need(n_vert);
    if (rc) return rc;
    const GridDims g{grid.occ.nx, grid.occ.ny, grid.occ.nz};
    hipLaunchKernelGGL(colour_vertex_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, layer_of(colour), g, (uint32_t)n_vox, flag, vid, n_vert,
                       mesh.d_rgba.p);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int TsdfStore::mesh_colours(hipStream_t stream, uint8_t* rgba) {
    const size_t nv = (size_t)mesh.counts[0];
    if (nv) LV_HIP(hipMemcpyAsync(rgba, mesh.d_rgba, nv * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
