// lv_depth.hip — lv_depth_integrate: depth-camera images fused into the TSDF volume (include/limovelo_hip.h "Depth fusion"; the
// rule's code is lv_depth.hpp, the projection lv_paint_dev.hpp's, shared with lv_map_paint and lv_colour_integrate).
//
// One call, on the context's stream: the images' rows staged back to back in pinned memory and copied once (U16 stays two bytes
// per pixel on the device), the views' records copied once, then ONE kernel:
//   depth_fuse_kernel   one lane per voxel of the box of voxels the views can judge at all (depth_view_box).  A workgroup owns a
//                       tile of 64 x 4 x 1 voxels: the lanes of a wavefront run along x, so its S and W accesses are 256
//                       contiguous bytes.  The views' records are read into LDS once per workgroup; lanes 0..31 judge one view
//                       each against the tile's box (depth_box_unseen) and the workgroup loops over the views that are left.
//                       Per view a lane projects its voxel's centre, reads ONE pixel and adds to (dS, dW) in registers; after
//                       the last view it folds, reading and writing S and W only where dW > 0.  No atomics on the volume, no use
//                       of the scratch words: the voxel has one owner.  The four statistics are summed per wavefront, then per
//                       workgroup through LDS, and added with one 64-bit atomic per counter and workgroup.
// Neither shortcut changes a result: both are conservative by a margin far above the f32 rounding of the projection, and a view
// that is kept judges every voxel by the full rule.  Nothing else depends on the launch geometry.
#include "lv_depth.hpp"

#include <cstring>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"   // (of lv_paint_dev.hpp this file takes paint_project alone, not its kernels)
#include "lv_paint_dev.hpp"
#pragma clang diagnostic pop

namespace lv {

namespace {

constexpr int DEPTH_TILE_X = 64, DEPTH_TILE_Y = 4;

// the voxels [x0, x1) x [y0, y1) x [z0, z1) of one launch
struct DepthBox {
    int x0, y0, z0, x1, y1, z1;
};

// grid (x tiles, y tiles, z layers) of the box; raw: the staged images; stats[0] += (voxel, view) pairs that pass step 2,
// stats[1] += those with a valid D, stats[2] += the sum of dW, stats[3] += voxels with dW > 0
__global__ __launch_bounds__(256) void depth_fuse_kernel(int32_t* __restrict__ S, int32_t* __restrict__ W, TsdfGrid g, DepthBox b,
                                                         const DepthCam* __restrict__ cams, DepthRule q, const uint8_t* __restrict__ raw,
                                                         unsigned long long* stats) {
    __shared__ DepthCam sh_cams[DEPTH_MAX_VIEWS];
    __shared__ uint32_t sh_live;
    __shared__ unsigned long long sh[4][4];
    const int n_views = q.view.n_views;
    {   // the records, dword by dword
        const uint32_t* src = reinterpret_cast<const uint32_t*>(cams);
        uint32_t* dst = reinterpret_cast<uint32_t*>(sh_cams);
        const uint32_t words = (uint32_t)n_views * (uint32_t)(sizeof(DepthCam) / 4);
        for (uint32_t w = threadIdx.x; w < words; w += 256u) dst[w] = src[w];
    }
    __syncthreads();
    const int i0 = b.x0 + (int)blockIdx.x * DEPTH_TILE_X, j0 = b.y0 + (int)blockIdx.y * DEPTH_TILE_Y, k = b.z0 + (int)blockIdx.z;
    if (threadIdx.x < 64u) {   // (the first wavefront, whole: one view per lane)
        bool live = false;
        if ((int)threadIdx.x < n_views) {
            const int i1 = min(i0 + DEPTH_TILE_X, b.x1) - 1, j1 = min(j0 + DEPTH_TILE_Y, b.y1) - 1;
            const float res = g.occ.resolution;
            const float lo[3] = {colour_centre(g.occ.origin[0], res, i0), colour_centre(g.occ.origin[1], res, j0), colour_centre(g.occ.origin[2], res, k)};
            const float hi[3] = {colour_centre(g.occ.origin[0], res, i1), colour_centre(g.occ.origin[1], res, j1), lo[2]};
            live = !depth_box_unseen(sh_cams[threadIdx.x].cam, q.view.min_depth, q.view.max_depth, q.rho, lo, hi);
        }
        const unsigned long long m = __ballot(live ? 1 : 0);
        if (threadIdx.x == 0) sh_live = (uint32_t)m;
    }
    __syncthreads();
    const uint32_t live_views = sh_live;
    const int i = i0 + (int)(threadIdx.x & 63u), j = j0 + (int)(threadIdx.x >> 6);
    uint32_t pairs = 0, valid = 0, dW = 0, touched = 0;
    if (live_views && i < b.x1 && j < b.y1) {
        const float4 p = make_float4(colour_centre(g.occ.origin[0], g.occ.resolution, i), colour_centre(g.occ.origin[1], g.occ.resolution, j),
                                     colour_centre(g.occ.origin[2], g.occ.resolution, k), 0.f);
        int32_t dS = 0;
        for (uint32_t rest = live_views; rest; rest &= rest - 1u) {
            const DepthCam& c = sh_cams[__ffs(rest) - 1];
            float z, u, v;
            if (!paint_project(c.cam, q.view, p, z, u, v)) continue;
            ++pairs;
            int px = (int)floorf(u + 0.5f), py = (int)floorf(v + 0.5f);   // (inside the image by step 2; the clamp only keeps every index inside the buffer)
            px = px < 0 ? 0 : (px > c.cam.width - 1 ? c.cam.width - 1 : px);
            py = py < 0 ? 0 : (py > c.cam.height - 1 ? c.cam.height - 1 : py);
            const size_t at = (size_t)py * (size_t)c.cam.width + (size_t)px;
            const uint8_t* img = raw + c.cam.raw_off;
            float D;
            const bool ok = c.cam.format == LV_DEPTH_U16 ? depth_of_u16(reinterpret_cast<const uint16_t*>(img)[at], c.scale, q.view.min_depth, q.view.max_depth, D)
                                                         : depth_of_f32(reinterpret_cast<const float*>(img)[at], q.view.min_depth, q.view.max_depth, D);
            if (!ok) continue;
            ++valid;
            int32_t s;
            if (!depth_quant(D, z, g.occ.resolution, g.T, q.carve, s)) continue;
            dS += s;
            ++dW;
        }
        if (dW > 0) {
            const size_t at = grid_at(g.occ, i, j, k);
            int32_t s = S[at], w = W[at];
            tsdf_fold(g.max_weight, (int64_t)dS, (int64_t)dW, s, w);
            S[at] = s;
            W[at] = w;
            touched = 1;
        }
    }
    const unsigned long long sum[4] = {wave_sum((unsigned long long)pairs), wave_sum((unsigned long long)valid), wave_sum((unsigned long long)dW),
                                       wave_sum((unsigned long long)touched)};
    if ((threadIdx.x & 63u) == 0)
        for (int c = 0; c < 4; ++c) sh[threadIdx.x >> 6][c] = sum[c];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long a = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (a) atomicAdd(stats + threadIdx.x, a);
    }
}

}  // namespace

int TsdfStore::integrate_depth(hipStream_t stream, const lv_depth_view* views, const DepthCam* cams, const DepthRule& q, uint64_t out[4]) {
    rays.packed = false;
    const int n_views = q.view.n_views;
    // the voxels some view can judge
    DepthBox b{0, 0, 0, 0, 0, 0};
    bool any = false;
    for (int w = 0; w < n_views; ++w) {
        int lo[3], hi[3];
        if (!depth_view_box(grid, cams[w].cam, q.view.max_depth, q.rho, lo, hi)) continue;
        if (!any) {
            b = DepthBox{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
        } else {
            b.x0 = lo[0] < b.x0 ? lo[0] : b.x0; b.y0 = lo[1] < b.y0 ? lo[1] : b.y0; b.z0 = lo[2] < b.z0 ? lo[2] : b.z0;
            b.x1 = hi[0] > b.x1 ? hi[0] : b.x1; b.y1 = hi[1] > b.y1 ? hi[1] : b.y1; b.z1 = hi[2] > b.z1 ? hi[2] : b.z1;
        }
        any = true;
    }
    if (!any) {   // nobody sees a voxel: nothing is staged, nothing runs
        LV_HIP(hipStreamSynchronize(stream));
        if (out) out[0] = out[1] = out[2] = out[3] = 0;
        return LV_OK;
    }
    int rc = depth.d_raw.need(q.raw_bytes);
    if (!rc) rc = depth.d_cams.need(DEPTH_MAX_VIEWS);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));   // (the previous call's copies out of the pinned buffers)
    rc = depth.h_cams.need(DEPTH_MAX_VIEWS);
    if (!rc) rc = depth.h_raw.need(q.raw_bytes);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    depth_stage_images(views, cams, n_views, depth.h_raw);
    std::memcpy(depth.h_cams, cams, (size_t)n_views * sizeof(DepthCam));
    LV_HIP(hipMemcpyAsync(depth.d_cams, depth.h_cams, (size_t)n_views * sizeof(DepthCam), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(depth.d_raw, depth.h_raw, q.raw_bytes, hipMemcpyHostToDevice, stream));
    const dim3 tiles((uint32_t)((b.x1 - b.x0 + DEPTH_TILE_X - 1) / DEPTH_TILE_X), (uint32_t)((b.y1 - b.y0 + DEPTH_TILE_Y - 1) / DEPTH_TILE_Y),
                     (uint32_t)(b.z1 - b.z0));
    hipLaunchKernelGGL(depth_fuse_kernel, tiles, dim3(256), 0, stream, d_S.p, d_W.p, grid, b, depth.d_cams.p, q, depth.d_raw.p, stats.d.p);
    LV_HIP(hipGetLastError());
    return stats.read(stream, out);   // (waits for the stream)
}

}  // namespace lv
