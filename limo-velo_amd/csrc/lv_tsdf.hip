// lv_tsdf.hip — TSDF fusion and the surface mesh (include/limovelo_hip.h "TSDF and mesh"; the rule's code is lv_tsdf.hpp).
//
// One lv_tsdf_integrate, on the context's stream:
//   tsdf_march_kernel  per view, one lane per return: range rules, world transform, quantisation (lv_occupancy.hpp's), the ray,
//                      then the integer walk.  Every cell inside the truncation band takes ONE no-return 64-bit atomicAdd of
//                      the packed word (dW above a signed 39-bit dS) into the call's scratch.  Integer adds commute, so the
//                      scratch does not depend on the schedule.
//   tsdf_fold_kernel   once per call, one lane per voxel: a non-zero scratch word is unpacked, folded into (S, W) with the
//                      max_weight rescale, and cleared for the next call; the contributions and touched voxels go to the stats.
// One lv_tsdf_mesh_build: classify the cells (tsdf_classify_kernel), hipcub exclusive sum -> vertex ids, the vertices
// (tsdf_vertex_kernel), faces per voxel 0..3 (tsdf_face_count_kernel), exclusive sum, the faces (tsdf_face_emit_kernel).  All of
// them read S and W from global memory: the 8 corners of a cell are shared with its neighbours through L2, nothing is staged.
// lv_tsdf_query / the metres of lv_tsdf_fetch are one-lane-per-item streaming kernels; load / clear are copies and fills.
// lv_volume_recentre (DESIGN.md "Rolling volumes") stages the moved volume in the call's scratch, which is all zero between
// calls and holds 8 bytes per voxel, so nothing is allocated: tsdf_shift_gather_kernel writes (S, W) of every voxel's source
// cell into its scratch word, two voxels and one 16-byte store per lane (an exposed voxel's word is 0, which is S = 0, W = 0),
// and tsdf_shift_unpack_kernel moves the words into S and W, four voxels per lane, and zeroes them again.
// The rays' packed states (lv_tsdf_ray.hip) are a member of the store too: integrate(), load(), clear() and recentre() mark them
// not packed, release() frees them.
// The colour layer (lv_colour.hip) is a member of the store: clear() and load() zero it, recentre() moves it through a second buffer
// of its own, mesh_build() takes the vertex colours from it, release() frees it.  A store without one does none of that.
// Depth fusion (lv_depth.hip) is a member as well: integrate_depth() folds into S and W directly, one owner per voxel, without
// the scratch words; release() frees its staging.
#include <utility>

#include "lv_tsdf.hpp"

#include <hipcub/hipcub.hpp>

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

constexpr uint32_t TSDF_NAN_BITS = 0x7FC00000u;

struct TsdfPose {
    float R[9];
    float t[3];
};

// pts: n returns (packed x, y, z) of one view; qs: its quantised sensor origin
__global__ __launch_bounds__(256) void tsdf_march_kernel(const float* __restrict__ pts, uint32_t n, TsdfGrid g, TsdfPose pose, int32_t qsx,
                                                         int32_t qsy, int32_t qsz, unsigned long long* scratch, unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int kind = OCC_RAY_IGNORED;
    int32_t qe[3] = {0, 0, 0};
    if (i < n) kind = occ_return(g.occ, pose.R, pose.t, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], qe);
    bool used = false;
    if (kind != OCC_RAY_IGNORED) {
        const int32_t qs[3] = {qsx, qsy, qsz};
        TsdfRay ray;
        used = tsdf_ray_init(g, qs, qe, kind, ray);
        if (used) {
            OccWalk w;
            occ_walk_init(w, ray.start, ray.qb);
            for (;;) {
                if (occ_in_grid(g.occ, w.vx, w.vy, w.vz)) {
                    int32_t s;
                    if (tsdf_cell_s(g, ray, w.vx, w.vy, w.vz, s)) atomicAdd(scratch + grid_at(g.occ, w.vx, w.vy, w.vz), tsdf_pack(s));
                } else if (occ_walk_left(g.occ, w)) {
                    break;
                }
                if (occ_walk_done(w)) break;
                occ_walk_step(w);
            }
        }
    }
    wave_add_to(stats + 0, used ? 1u : 0u);
    wave_add_to(stats + 1, used && kind == OCC_RAY_CUT ? 1u : 0u);
}

__global__ __launch_bounds__(256) void tsdf_fold_kernel(int32_t* __restrict__ S, int32_t* __restrict__ W, unsigned long long* __restrict__ scratch,
                                                        uint32_t n_vox, int32_t max_weight, unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long contributions = 0;
    uint32_t touched = 0;
    if (i < n_vox) {
        const unsigned long long word = scratch[i];
        if (word) {
            int64_t dS, dW;
            tsdf_unpack(word, dS, dW);
            int32_t s = S[i], w = W[i];
            tsdf_fold(max_weight, dS, dW, s, w);
            S[i] = s;
            W[i] = w;
            scratch[i] = 0;
            contributions = (unsigned long long)dW;
            touched = 1;
        }
    }
    wave_add_to(stats + 2, contributions);
    wave_add_to(stats + 3, touched);
}

// scratch word c = S of the source cell in the low half, W in the high half.  A workgroup strides over the pairs and adds its
// two counts once, as occ_shift_kernel does: stats[1] += exposed voxels, stats[2] += voxels that left (W > 0, see grid_shift_mirror)
__global__ __launch_bounds__(256) void tsdf_shift_gather_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W,
                                                                unsigned long long* __restrict__ scratch, GridDims g, int32_t dx, int32_t dy,
                                                                int32_t dz, uint32_t n_vox, unsigned long long* stats) {
    __shared__ unsigned long long sh[4][4];
    const uint32_t pairs = (n_vox + 1u) / 2u;
    unsigned long long exposed = 0, left = 0;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < pairs; t += gridDim.x * 256u) {
        const uint32_t c0 = 2u * t;
        int i, j, k, si, sj, sk;
        grid_ijk(g, c0, i, j, k);
        const uint32_t n = n_vox - c0 < 2u ? n_vox - c0 : 2u;
        uint32_t e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            if (q < n) {
                if (grid_shift_source(g, dx, dy, dz, i, j, k, si, sj, sk)) {
                    const size_t at = grid_at(g, si, sj, sk);
                    e[2 * q] = (uint32_t)S[at];
                    e[2 * q + 1] = (uint32_t)W[at];
                } else {
                    grid_shift_mirror(g, i, j, k, si, sj, sk);
                    left += W[grid_at(g, si, sj, sk)] > 0 ? 1u : 0u;
                    ++exposed;
                }
                if (++i == g.nx) {   // the next voxel of the pair
                    i = 0;
                    if (++j == g.ny) {
                        j = 0;
                        ++k;
                    }
                }
            }
        }
        if (n == 2u)
            *reinterpret_cast<uint4*>(scratch + c0) = make_uint4(e[0], e[1], e[2], e[3]);
        else
            scratch[c0] = ((unsigned long long)e[1] << 32) | (unsigned long long)e[0];
    }
    unsigned long long a;
    if (block_fold4(sh, exposed, left, 0ull, 0ull, a) && threadIdx.x < 2 && a) atomicAdd(stats + 1 + threadIdx.x, a);
}

// S, W of four voxels from their scratch words, which go back to zero
__global__ __launch_bounds__(256) void tsdf_shift_unpack_kernel(int32_t* __restrict__ S, int32_t* __restrict__ W, unsigned long long* __restrict__ scratch,
                                                                uint32_t n_vox) {
    const uint32_t c0 = 4u * (blockIdx.x * blockDim.x + threadIdx.x);
    if (c0 >= n_vox) return;
    if (n_vox - c0 >= 4u) {
        uint4* w = reinterpret_cast<uint4*>(scratch + c0);
        const uint4 a = w[0], b = w[1];
        *reinterpret_cast<uint4*>(S + c0) = make_uint4(a.x, a.z, b.x, b.z);
        *reinterpret_cast<uint4*>(W + c0) = make_uint4(a.y, a.w, b.y, b.w);
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        w[0] = zero;
        w[1] = zero;
    } else {   // the volume's last one to three voxels
        for (uint32_t c = c0; c < n_vox; ++c) {
            const unsigned long long word = scratch[c];
            S[c] = (int32_t)(uint32_t)word;
            W[c] = (int32_t)(uint32_t)(word >> 32);
            scratch[c] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void tsdf_metres_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, uint32_t n_vox,
                                                          float resolution, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_vox) out[i] = tsdf_metres(resolution, S[i], W[i]);
}

__global__ __launch_bounds__(256) void tsdf_query_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, TsdfGrid g,
                                                         const float* __restrict__ pts, uint32_t n, float* __restrict__ metres,
                                                         int32_t* __restrict__ weight) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int ci, cj, ck;
    float m = __uint_as_float(TSDF_NAN_BITS);
    int32_t w = 0;
    if (grid_cell_of(g.occ, g.occ.origin, g.occ.resolution, false, pts + 3 * (size_t)i, ci, cj, ck)) {
        const size_t at = grid_at(g.occ, ci, cj, ck);
        w = W[at];
        m = tsdf_metres(g.occ.resolution, S[at], w);
    }
    metres[i] = m;
    weight[i] = w;
}

// flag[cell] = 1 where the cell with that low corner is active; flag[n_vox] = 0 (the scan's total lands there)
__global__ __launch_bounds__(256) void tsdf_classify_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, GridDims g, uint32_t n_vox,
                                                            int32_t min_weight, uint32_t* __restrict__ flag) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell > n_vox) return;
    uint32_t f = 0;
    if (cell < n_vox) {
        int i, j, k;
        grid_ijk(g, cell, i, j, k);
        TsdfCorners c;
        f = tsdf_cell_active(g, S, W, min_weight, i, j, k, c) ? 1u : 0u;
    }
    flag[cell] = f;
}

__global__ __launch_bounds__(256) void tsdf_vertex_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, GridDims g, uint32_t n_vox,
                                                          int32_t min_weight, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ vid,
                                                          float ox, float oy, float oz, float resolution, int32_t* __restrict__ sub,
                                                          float* __restrict__ xyz) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_vox || !flag[cell]) return;
    int i, j, k;
    grid_ijk(g, cell, i, j, k);
    TsdfCorners c;
    tsdf_cell_active(g, S, W, min_weight, i, j, k, c);
    int32_t v[3];
    tsdf_vertex(c, i, j, k, v);
    const size_t o = 3 * (size_t)vid[cell];
    sub[o] = v[0];
    sub[o + 1] = v[1];
    sub[o + 2] = v[2];
    xyz[o] = tsdf_vertex_metres(ox, resolution, v[0]);
    xyz[o + 1] = tsdf_vertex_metres(oy, resolution, v[1]);
    xyz[o + 2] = tsdf_vertex_metres(oz, resolution, v[2]);
}

// fcnt[p] = the quads of the three edges that start at voxel p; fcnt[n_vox] = 0.  The refused edges go to *refused.
__global__ __launch_bounds__(256) void tsdf_face_count_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, GridDims g, uint32_t n_vox,
                                                              int32_t min_weight, const uint32_t* __restrict__ flag, uint32_t* __restrict__ fcnt,
                                                              unsigned long long* refused) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t quads = 0, bad = 0;
    if (p < n_vox) {
        int i, j, k;
        grid_ijk(g, p, i, j, k);
        uint32_t cells[4];
        for (int a = 0; a < 3; ++a) {
            const int r = tsdf_edge_face(g, S, W, min_weight, i, j, k, a, [flag](uint32_t c) { return flag[c] != 0; }, cells);
            quads += r == 1;
            bad += r == 2;
        }
    }
    if (p <= n_vox) fcnt[p] = quads;
    wave_add_to(refused, bad);
}

__global__ __launch_bounds__(256) void tsdf_face_emit_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, GridDims g, uint32_t n_vox,
                                                             int32_t min_weight, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ vid,
                                                             const uint32_t* __restrict__ fcnt, const uint32_t* __restrict__ foff,
                                                             uint32_t* __restrict__ tri) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_vox || !fcnt[p]) return;
    int i, j, k;
    grid_ijk(g, p, i, j, k);
    size_t o = 6 * (size_t)foff[p];   // two triangles of three indices per quad
    uint32_t cells[4];
    for (int a = 0; a < 3; ++a) {
        if (tsdf_edge_face(g, S, W, min_weight, i, j, k, a, [flag](uint32_t c) { return flag[c] != 0; }, cells) != 1) continue;
        const uint32_t q0 = vid[cells[0]], q1 = vid[cells[1]], q2 = vid[cells[2]], q3 = vid[cells[3]];
        tri[o] = q0; tri[o + 1] = q1; tri[o + 2] = q2;
        tri[o + 3] = q0; tri[o + 4] = q2; tri[o + 5] = q3;
        o += 6;
    }
}

}  // namespace

void TsdfStore::mesh_release() {
    mesh.d_xyz.release(); mesh.d_sub.release(); mesh.d_tri.release(); mesh.d_rgba.release();
    mesh = TsdfMesh();
}

void TsdfStore::release() {
    mesh_release();
    d_S.release(); d_W.release(); d_scratch.release(); stats.release(); pts.release(); d_out.release(); d_wout.release();
    d_flag.release(); d_vid.release(); d_fcnt.release(); d_foff.release(); d_tmp.release();
    colour.release();
    rays.release();
    depth.release();
    align.release();
    merged.release();
    *this = TsdfStore();
}

int TsdfStore::configure(hipStream_t stream, const lv_tsdf_params& p) {
    LV_HIP(hipStreamSynchronize(stream));
    release();
    const TsdfGrid g = tsdf_grid_of(p);
    const size_t nv = grid_cells(g.occ);
    int rc = d_S.need(nv);
    if (!rc) rc = d_W.need(nv);
    if (!rc) rc = d_scratch.need(nv);
    if (!rc) rc = stats.need();
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(d_scratch, 0, nv * sizeof(unsigned long long), stream));
    prm = p;
    grid = g;
    for (int a = 0; a < 3; ++a) origin0[a] = p.origin[a];
    n_vox = nv;
    rc = clear(stream);
    if (rc) return rc;
    configured = true;
    return LV_OK;
}

int TsdfStore::clear(hipStream_t stream) {
    rays.packed = false;
    LV_HIP(hipMemsetAsync(d_S, 0, n_vox * sizeof(int32_t), stream));
    LV_HIP(hipMemsetAsync(d_W, 0, n_vox * sizeof(int32_t), stream));
    if (colour.present) return colour_clear(stream);   // (waits for the stream)
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::integrate(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t out[4]) {
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) total += views[v].n;
    rays.packed = false;
    int rc = LV_OK;
    if (total) {   // every view's returns in one upload
        rc = pts.reserve(stream, total);
        if (rc) return rc;
        for (size_t v = 0; v < n_views; ++v) pts.append(views[v].points, views[v].stride, views[v].n);
        rc = pts.upload(stream);
        if (rc) return rc;
    }
    rc = stats.zero(stream);
    if (rc) return rc;
    size_t o = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const size_t n = views[v].n;
        int32_t qs[3];
        if (n && occ_view_origin(grid.occ, views[v].t, qs)) {
            TsdfPose pose;
            std::memcpy(pose.R, views[v].R, sizeof(pose.R));
            std::memcpy(pose.t, views[v].t, sizeof(pose.t));
            hipLaunchKernelGGL(tsdf_march_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, pts.d + 3 * o, (uint32_t)n, grid, pose, qs[0], qs[1],
                               qs[2], d_scratch.p, stats.d.p);
        }
        o += n;
    }
    hipLaunchKernelGGL(tsdf_fold_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, d_S.p, d_W.p, d_scratch.p, (uint32_t)n_vox, grid.max_weight,
                       stats.d.p);
    LV_HIP(hipGetLastError());
    return stats.read(stream, out);
}

int TsdfStore::query(hipStream_t stream, const void* points, size_t stride, size_t n, float* metres, int32_t* weight) {
    if (n == 0) return LV_OK;
    int rc = pts.reserve(stream, n);
    if (!rc) rc = d_out.need(n);
    if (!rc) rc = d_wout.need(n);
    if (rc) return rc;
    pts.append(points, stride, n);
    rc = pts.upload(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tsdf_query_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_S.p, d_W.p, grid, pts.d.p, (uint32_t)n, d_out.p, d_wout.p);
    LV_HIP(hipGetLastError());
    if (metres) LV_HIP(hipMemcpyAsync(metres, d_out, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (weight) LV_HIP(hipMemcpyAsync(weight, d_wout, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::fetch(hipStream_t stream, int32_t* S, int32_t* W, float* metres) {
    if (metres) {
        const int rc = d_out.need(n_vox);
        if (rc) return rc;
        hipLaunchKernelGGL(tsdf_metres_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, d_S.p, d_W.p, (uint32_t)n_vox, grid.occ.resolution,
                           d_out.p);
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(metres, d_out, n_vox * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    if (S) LV_HIP(hipMemcpyAsync(S, d_S, n_vox * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (W) LV_HIP(hipMemcpyAsync(W, d_W, n_vox * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::load(hipStream_t stream, const int32_t* S, const int32_t* W) {
    rays.packed = false;
    LV_HIP(hipMemcpyAsync(d_S, S, n_vox * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_W, W, n_vox * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (colour.present) return colour_clear(stream);   // (colours of another volume mean nothing; waits for the stream)
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::recentre(hipStream_t stream, const int32_t d[3], const int32_t s_new[3], const float origin_new[3], uint64_t out[4]) {
    rays.packed = false;
    int rc = stats.zero(stream);
    if (!rc && colour.present) rc = colour.d_next.need(4 * n_vox);   // (before anything moves: a call that fails has changed nothing)
    if (rc) return rc;
    const GridDims g{grid.occ.nx, grid.occ.ny, grid.occ.nz};
    hipLaunchKernelGGL(tsdf_shift_gather_kernel, dim3(grid_stride_blocks((n_vox + 1) / 2)), dim3(256), 0, stream, d_S.p, d_W.p, d_scratch.p, g, d[0], d[1], d[2],
                       (uint32_t)n_vox, stats.d.p);
    hipLaunchKernelGGL(tsdf_shift_unpack_kernel, dim3(blocks_of((n_vox + 3) / 4)), dim3(256), 0, stream, d_S.p, d_W.p, d_scratch.p, (uint32_t)n_vox);
    LV_HIP(hipGetLastError());
    if (colour.present) rc = colour_shift(stream, d);
    if (rc) return rc;
    uint64_t st[4];
    rc = stats.read(stream, st);   // (waits for the stream)
    if (rc) return rc;
    if (colour.present) {   // the moved layer takes the old one's place
        std::swap(colour.d_sums, colour.d_next);
        colour.d_next.release();
    }
    if (out) {
        out[0] = (uint64_t)n_vox - st[1];   // a voxel is kept or exposed
        out[1] = st[1];
        out[2] = st[2];
        out[3] = 0;
    }
    for (int a = 0; a < 3; ++a) {
        shift[a] = s_new[a];
        prm.origin[a] = origin_new[a];
        grid.occ.origin[a] = origin_new[a];
    }
    return LV_OK;
}

// exclusive sum of in[0 .. n] into out[0 .. n] (n + 1 items: out[n] is the total), then the total to the host
int tsdf_scan(hipStream_t stream, DevBuf<void>& tmp, const uint32_t* in, uint32_t* out, size_t n, uint32_t* total) {
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)(n + 1), stream));
    const int rc = tmp.need(bytes);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, (int)(n + 1), stream));
    LV_HIP(hipMemcpyAsync(total, out + n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::mesh_build(hipStream_t stream, int min_weight, uint64_t counts[4]) {
    LV_HIP(hipStreamSynchronize(stream));
    mesh_release();
    const GridDims g{grid.occ.nx, grid.occ.ny, grid.occ.nz};
    const uint32_t nv = (uint32_t)n_vox;
    uint32_t n_vert = 0, n_quad = 0;
    uint64_t st[4] = {0, 0, 0, 0};
    // the steps; whatever they return, the per-voxel work arrays are freed below
    const int built = [&]() -> int {
        int rc = d_flag.need(n_vox + 1);
        if (!rc) rc = d_vid.need(n_vox + 1);
        if (!rc) rc = d_fcnt.need(n_vox + 1);
        if (!rc) rc = d_foff.need(n_vox + 1);
        if (!rc) rc = stats.zero(stream);
        if (rc) return rc;
        hipLaunchKernelGGL(tsdf_classify_kernel, dim3(blocks_of(n_vox + 1)), dim3(256), 0, stream, d_S.p, d_W.p, g, nv, min_weight, d_flag.p);
        LV_HIP(hipGetLastError());
        rc = tsdf_scan(stream, d_tmp, d_flag.p, d_vid.p, n_vox, &n_vert);
        if (rc) return rc;
        hipLaunchKernelGGL(tsdf_face_count_kernel, dim3(blocks_of(n_vox + 1)), dim3(256), 0, stream, d_S.p, d_W.p, g, nv, min_weight, d_flag.p, d_fcnt.p,
                           stats.d.p);
        LV_HIP(hipGetLastError());
        rc = tsdf_scan(stream, d_tmp, d_fcnt.p, d_foff.p, n_vox, &n_quad);
        if (rc) return rc;
        if (n_vert) {
            rc = mesh.d_xyz.need(3 * (size_t)n_vert);
            if (!rc) rc = mesh.d_sub.need(3 * (size_t)n_vert);
            if (rc) return rc;
            hipLaunchKernelGGL(tsdf_vertex_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, d_S.p, d_W.p, g, nv, min_weight, d_flag.p, d_vid.p,
                               grid.occ.origin[0], grid.occ.origin[1], grid.occ.origin[2], grid.occ.resolution, mesh.d_sub.p, mesh.d_xyz.p);
            LV_HIP(hipGetLastError());
            if (colour.present) {
                rc = colour_vertices(stream, d_flag.p, d_vid.p, n_vert);
                if (rc) return rc;
            }
        }
        if (n_quad) {
            rc = mesh.d_tri.need(6 * (size_t)n_quad);
            if (rc) return rc;
            hipLaunchKernelGGL(tsdf_face_emit_kernel, dim3(blocks_of(n_vox)), dim3(256), 0, stream, d_S.p, d_W.p, g, nv, min_weight, d_flag.p, d_vid.p,
                               d_fcnt.p, d_foff.p, mesh.d_tri.p);
            LV_HIP(hipGetLastError());
        }
        return stats.read(stream, st);   // (waits for the stream)
    }();
    if (built != LV_OK) hipStreamSynchronize(stream);   // (a kernel of a failed build may still read the arrays)
    d_flag.release(); d_vid.release(); d_fcnt.release(); d_foff.release(); d_tmp.release();
    if (built != LV_OK) {
        mesh_release();
        return built;
    }
    mesh.built = true;
    mesh.coloured = colour.present;
    mesh.stale = 0;
    mesh.min_weight = min_weight;
    mesh.counts[0] = n_vert;
    mesh.counts[1] = 2 * (uint64_t)n_quad;
    mesh.counts[2] = n_vert;
    mesh.counts[3] = st[0];
    if (counts)
        for (int i = 0; i < 4; ++i) counts[i] = mesh.counts[i];
    return LV_OK;
}

int TsdfStore::mesh_fetch(hipStream_t stream, float* xyz, int32_t* sub, uint32_t* tri) {
    const size_t nv = (size_t)mesh.counts[0], nt = (size_t)mesh.counts[1];
    if (xyz && nv) LV_HIP(hipMemcpyAsync(xyz, mesh.d_xyz, 3 * nv * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (sub && nv) LV_HIP(hipMemcpyAsync(sub, mesh.d_sub, 3 * nv * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (tri && nt) LV_HIP(hipMemcpyAsync(tri, mesh.d_tri, 3 * nt * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
