// lv_tsdf_ray.hip — ray casting on the TSDF surface (include/limovelo_hip.h "Surface ray casting"; the rule's code is
// lv_tsdf_ray.hpp).
//
// On the context's stream:
//   surf_pack_kernel   one lane per voxel of the x rows padded to whole words: the state of its voxel (UNKNOWN / OUT / IN from S, W
//                      and min_weight), sixteen lanes' states folded into one word of the packed volume (2 bits per voxel,
//                      lv_ray.hpp's layout), stored by the first of them.  Runs in the first call after S or W changed, or with
//                      another min_weight.
//   surf_cast_kernel   one lane per ray: both ends quantised, then the walk of lv_tsdf_ray.hpp through the packed states.  The lane
//                      keeps the word it stands in in a register and loads again only when the walk leaves it; S, W and the colour
//                      layer are read only at the stop.  The record goes out as two 16-byte stores.
//   surf_view_kernel   per view, one lane per return: occ_return, then the same walk from the view's origin; the four counts of
//                      the call by one wave fold each.
#include "lv_tsdf_ray.hpp"

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

struct SurfPose {
    float R[9];
    float t[3];
};

// n: rows * wx16 * 16 lanes; lane id is voxel (id % (wx16 * 16)) of row id / (wx16 * 16).  A group of 16 lanes never straddles
// a row, nor a wavefront.
__global__ __launch_bounds__(256) void surf_pack_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, uint32_t n, int nx,
                                                        int32_t min_weight, uint32_t* __restrict__ words) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t padded = (uint32_t)ray_wx16(nx) * 16u;
    const uint32_t row = id / padded, i = id - row * padded;
    uint32_t v = 0;
    if (id < n && i < (uint32_t)nx) {
        const size_t at = (size_t)row * (size_t)nx + i;
        v = ray_pack(surf_state_voxel(S[at], W[at], min_weight), (int)i);
    }
    for (int o = 8; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    if (id < n && (i & 15u) == 0) words[id >> 4] = v;
}

__device__ __forceinline__ void surf_store(const lv_tsdf_ray_result& r, const float nrm[3], uint32_t rgba, size_t i,
                                           lv_tsdf_ray_result* __restrict__ out, float* __restrict__ normals, uint32_t* __restrict__ colours) {
    int4* o = reinterpret_cast<int4*>(out + i);
    o[0] = make_int4(r.status, r.cell, r.steps, r.axis);
    o[1] = make_int4(r.depth, r.t, r.n_known, r.n_unknown);
    if (normals) {
        normals[3 * i] = nrm[0];
        normals[3 * i + 1] = nrm[1];
        normals[3 * i + 2] = nrm[2];
    }
    if (colours) colours[i] = rgba;
}

// pts: n `from` points, then n `to` points, packed.  sums: the colour layer or NULL; normals, colours: NULL where not asked for
__global__ __launch_bounds__(256) void surf_cast_kernel(const float* __restrict__ pts, uint32_t n, OccGrid g, int32_t min_weight,
                                                        const uint32_t* __restrict__ words, const int32_t* __restrict__ S,
                                                        const int32_t* __restrict__ W, const uint32_t* __restrict__ sums,
                                                        lv_tsdf_ray_result* __restrict__ out, float* __restrict__ normals,
                                                        uint32_t* __restrict__ colours) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = pts + 3 * (size_t)i;
    const float* b = pts + 3 * ((size_t)n + i);
    const float from[3] = {a[0], a[1], a[2]}, to[3] = {b[0], b[1], b[2]};
    RayStates st(words);
    lv_tsdf_ray_result r;
    float nrm[3];
    uint32_t rgba;
    surf_cast(g, from, to, min_weight, st, S, W, sums, normals != nullptr, colours != nullptr, r, nrm, rgba);
    surf_store(r, nrm, rgba, i, out, normals, colours);
}

// pts: the n returns of one view; qs: its quantised origin; valid 0: the view gives no evidence, every return is IGNORED.
// out, normals, colours: the view's own entries.  stats: rays used, HIT, BLOCKED, CLEAR
__global__ __launch_bounds__(256) void surf_view_kernel(const float* __restrict__ pts, uint32_t n, OccGrid g, SurfPose pose, int valid, int32_t qsx,
                                                        int32_t qsy, int32_t qsz, int32_t min_weight, const uint32_t* __restrict__ words,
                                                        const int32_t* __restrict__ S, const int32_t* __restrict__ W,
                                                        const uint32_t* __restrict__ sums, lv_tsdf_ray_result* __restrict__ out,
                                                        float* __restrict__ normals, uint32_t* __restrict__ colours, unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int kind = OCC_RAY_IGNORED;
    int32_t qe[3] = {0, 0, 0};
    if (i < n && valid) kind = occ_return(g, pose.R, pose.t, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], qe);
    lv_tsdf_ray_result r;
    float nrm[3] = {0.f, 0.f, 0.f};
    uint32_t rgba = 0;
    surf_ignored(r);
    if (kind != OCC_RAY_IGNORED) {
        const int32_t qs[3] = {qsx, qsy, qsz};
        RayStates st(words);
        surf_cast_q(g, qs, qe, min_weight, st, S, W, sums, normals != nullptr, colours != nullptr, r, nrm, rgba);
    }
    if (i < n) surf_store(r, nrm, rgba, i, out, normals, colours);
    wave_add_to(stats + 0, kind != OCC_RAY_IGNORED ? 1u : 0u);
    wave_add_to(stats + 1, r.status == LV_SURF_HIT ? 1u : 0u);
    wave_add_to(stats + 2, r.status == LV_SURF_BLOCKED ? 1u : 0u);
    wave_add_to(stats + 3, r.status == LV_SURF_CLEAR ? 1u : 0u);
}

}  // namespace

int TsdfStore::rays_pack(hipStream_t stream, int min_weight) {
    if (rays.packed && rays.min_weight == min_weight) return LV_OK;
    const OccGrid& g = grid.occ;
    const size_t rows = (size_t)g.ny * (size_t)g.nz, n_words = rows * (size_t)ray_wx16(g.nx);
    const int rc = rays.d_states.need(n_words);
    if (rc) return rc;
    rays.packed = false;
    hipLaunchKernelGGL(surf_pack_kernel, dim3(blocks_of(n_words * 16)), dim3(256), 0, stream, d_S.p, d_W.p, (uint32_t)(n_words * 16), g.nx, min_weight,
                       rays.d_states.p);
    LV_HIP(hipGetLastError());
    rays.packed = true;
    rays.min_weight = min_weight;
    return LV_OK;
}

int TsdfStore::raycast(hipStream_t stream, int min_weight, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                       lv_tsdf_ray_result* out, float* normals, uint8_t* rgba) {
    if (n == 0) return LV_OK;
    int rc = rays.pts.reserve(stream, 2 * n);
    if (!rc) rc = rays.d_res.need(n);
    if (!rc && normals) rc = rays.d_nrm.need(3 * n);
    if (!rc && rgba) rc = rays.d_rgba.need(n);
    if (!rc) rc = rays_pack(stream, min_weight);
    if (rc) return rc;
    rays.pts.append(from, from_stride, n);
    rays.pts.append(to, to_stride, n);
    rc = rays.pts.upload(stream);
    if (rc) return rc;
    const uint32_t* sums = colour.present ? colour.d_sums.p : nullptr;
    hipLaunchKernelGGL(surf_cast_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, rays.pts.d.p, (uint32_t)n, grid.occ, min_weight, rays.d_states.p,
                       d_S.p, d_W.p, sums, rays.d_res.p, normals ? rays.d_nrm.p : nullptr, rgba ? rays.d_rgba.p : nullptr);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(out, rays.d_res, n * sizeof(lv_tsdf_ray_result), hipMemcpyDeviceToHost, stream));
    if (normals) LV_HIP(hipMemcpyAsync(normals, rays.d_nrm, 3 * n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (rgba) LV_HIP(hipMemcpyAsync(rgba, rays.d_rgba, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::raycast_views(hipStream_t stream, int min_weight, const lv_view* views, size_t n_views, lv_tsdf_ray_result* out, float* normals,
                             uint8_t* rgba, uint64_t st[4]) {
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) total += views[v].n;
    int rc = rays.pts.reserve(stream, total);   // (synchronises the stream)
    if (!rc && total) rc = rays.d_res.need(total);
    if (!rc && total && normals) rc = rays.d_nrm.need(3 * total);
    if (!rc && total && rgba) rc = rays.d_rgba.need(total);
    if (!rc) rc = rays_pack(stream, min_weight);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    for (size_t v = 0; v < n_views; ++v) rays.pts.append(views[v].points, views[v].stride, views[v].n);
    rc = rays.pts.upload(stream);
    if (rc) return rc;
    const uint32_t* sums = colour.present ? colour.d_sums.p : nullptr;
    size_t o = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const size_t n = views[v].n;
        if (!n) continue;
        int32_t qs[3] = {0, 0, 0};
        const int valid = occ_view_origin(grid.occ, views[v].t, qs) ? 1 : 0;
        SurfPose pose;
        std::memcpy(pose.R, views[v].R, sizeof(pose.R));
        std::memcpy(pose.t, views[v].t, sizeof(pose.t));
        hipLaunchKernelGGL(surf_view_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, rays.pts.d.p + 3 * o, (uint32_t)n, grid.occ, pose, valid, qs[0], qs[1],
                           qs[2], min_weight, rays.d_states.p, d_S.p, d_W.p, sums, rays.d_res.p + o, normals ? rays.d_nrm.p + 3 * o : nullptr,
                           rgba ? rays.d_rgba.p + o : nullptr, stats.d.p);
        LV_HIP(hipGetLastError());
        o += n;
    }
    if (total) {
        LV_HIP(hipMemcpyAsync(out, rays.d_res, total * sizeof(lv_tsdf_ray_result), hipMemcpyDeviceToHost, stream));
        if (normals) LV_HIP(hipMemcpyAsync(normals, rays.d_nrm, 3 * total * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (rgba) LV_HIP(hipMemcpyAsync(rgba, rays.d_rgba, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    return stats.read(stream, st);   // (waits for the stream)
}

}  // namespace lv
