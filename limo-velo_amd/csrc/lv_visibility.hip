// lv_visibility.hip — lv_map_remove_dynamic: map points a sensor has seen through leave the map (include/limovelo_hip.h
// "Dynamic-point removal"; the reference's TODO "Try to add a module for removing dynamic objects such as people or vehicles").
//
// Three kernels, one lane per item, no scratch:
//   vis_image_kernel     one lane per return (every view at once): its pixel keeps the minimum range, an atomicMin on the f32 bits
//                        (a non-negative f32 orders like its bit pattern; +inf = empty): order-independent, deterministic;
//   vis_min_cols_kernel  the window-min, separable: along the columns (wrapping at +-pi), then
//   vis_min_rows_kernel  along the rows (clipped at the image's edge);
//   vis_classify_kernel  one lane per id: reads orig once, loops over the views, gathers from the filtered images (512 KiB per
//                        2048 x 64 view: they stay in the L2 / Infinity Cache), writes the hit count at the point's living rank
//                        and appends the removed ids to the map's dead list (dead_list_append, lv_query_dev.hpp).
// The dead list is then retired by MapStore::retire_dead_list, the path of every removal.
#include "lv_visibility.hpp"

#include "lv_query_dev.hpp"

#include <cmath>
#include <cstring>

namespace lv {

namespace {

constexpr float VIS_PI = 3.14159265358979323846f;

// the pixel of a sensor-frame point (x, y, z) with x*x + y*y = xy2; false outside the rows
__device__ __forceinline__ bool vis_pixel(const VisRule& q, float x, float y, float z, float xy2, uint32_t& pix) {
    const float v = (atan2f(z, sqrtf(xy2)) - q.v_min) * q.inv_row;
    if (!(v >= 0.f && v <= (float)q.height)) return false;
    int row = (int)floorf(v);
    if (row >= q.height) row = q.height - 1;   // (elevation v_max exactly: the top row)
    int col = (int)floorf((atan2f(y, x) + VIS_PI) * q.inv_col);
    if (col >= q.width) col -= q.width;        // (azimuth +pi is -pi)
    if (col < 0) col = 0;
    pix = (uint32_t)row * (uint32_t)q.width + (uint32_t)col;
    return true;
}

// pts: n returns of every view, w = the view's index (bits); img: n_views images initialised to +inf
__global__ __launch_bounds__(256) void vis_image_kernel(const float4* __restrict__ pts, uint32_t n, VisRule q, uint32_t* __restrict__ img) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    if (!(fabsf(p.x) < pos_inf() && fabsf(p.y) < pos_inf() && fabsf(p.z) < pos_inf())) return;
    const float xy2 = p.x * p.x + p.y * p.y;
    const float r = sqrtf(xy2 + p.z * p.z);
    if (!(r > q.min_range)) return;
    uint32_t pix;
    if (!vis_pixel(q, p.x, p.y, p.z, xy2, pix)) return;
    const size_t plane = (size_t)q.width * (size_t)q.height;
    atomicMin(&img[(size_t)__float_as_uint(p.w) * plane + pix], __float_as_uint(r));
}

// out[pixel] = min of in over the columns col - w .. col + w of its row (wrapping); total = n_views * height * width
__global__ __launch_bounds__(256) void vis_min_cols_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t total, int width, int w) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int col = (int)(i % (uint32_t)width);
    const uint32_t base = i - (uint32_t)col;
    float m = in[i];
    for (int d = 1; d <= w; ++d) {
        const int a = (col + d) % width, b = ((col - d) % width + width) % width;
        m = fminf(m, fminf(in[base + (uint32_t)a], in[base + (uint32_t)b]));
    }
    out[i] = m;
}

// out[pixel] = min of in over the rows row - w .. row + w of its column (clipped at the image's edge)
__global__ __launch_bounds__(256) void vis_min_rows_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t total, int width, int height,
                                                           int w) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t plane = (uint32_t)width * (uint32_t)height;
    const int row = (int)((i % plane) / (uint32_t)width);
    float m = in[i];
    for (int d = 1; d <= w; ++d) {
        if (row + d < height) m = fminf(m, in[i + (uint32_t)d * (uint32_t)width]);
        if (row - d >= 0) m = fminf(m, in[i - (uint32_t)d * (uint32_t)width]);
    }
    out[i] = m;
}

// One lane per id.  pose: 12 floats per view (R row-major, t); img: the filtered images.  hits (optional): the count at the
// point's rank (rank NULL: the id).  remove: the points seen through in >= min_hits views go to the dead list (x, y, z, id)
// and read x = +inf from here on.
__global__ __launch_bounds__(256) void vis_classify_kernel(float4* __restrict__ orig, uint32_t n_ids, const float* __restrict__ pose,
                                                           const float* __restrict__ img, VisRule q, const uint32_t* __restrict__ rank,
                                                           uint8_t* __restrict__ hits, int remove, float4* __restrict__ dead, uint32_t dead_cap,
                                                           MapCounters* cnt) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool gone = false;
    if (id < n_ids) p = orig[id];
    if (id < n_ids && pt_alive(p)) {
        const size_t plane = (size_t)q.width * (size_t)q.height;
        uint32_t h = 0;
        for (int v = 0; v < q.n_views; ++v) {
            const float* P = pose + 12 * v;
            const float dx = p.x - P[9], dy = p.y - P[10], dz = p.z - P[11];
            const float x = P[0] * dx + P[3] * dy + P[6] * dz;   // R^T d, summed left to right (unfused: -ffp-contract=off)
            const float y = P[1] * dx + P[4] * dy + P[7] * dz;
            const float z = P[2] * dx + P[5] * dy + P[8] * dz;
            const float xy2 = x * x + y * y;
            const float r = sqrtf(xy2 + z * z);
            if (!(r >= q.min_range && r <= q.max_range)) continue;
            uint32_t pix;
            if (!vis_pixel(q, x, y, z, xy2, pix)) continue;
            const float ri = img[(size_t)v * plane + pix];
            if (ri < pos_inf() && ri - r > fmaxf(q.margin_abs, q.margin_rel * r)) ++h;
        }
        if (hits) hits[rank_of(rank, id)] = (uint8_t)h;
        gone = remove && h >= (uint32_t)q.min_hits;
    }
    dead_list_append(gone, p, id, orig, dead, dead_cap, cnt);
}

}  // namespace

int VisStore::build(hipStream_t stream, const lv_view* views, size_t n_views, const VisRule& q) {
    size_t n = 0;
    for (size_t v = 0; v < n_views; ++v) n += views[v].n;
    const size_t pose_bytes = vis_pose_bytes(q.n_views);
    const size_t blob = vis_blob_bytes(q);
    const size_t pixels = (size_t)q.n_views * q.width * q.height;
    int rc = d_blob.need(blob);
    if (!rc) rc = d_tmp.need(pixels);
    if (!rc) rc = d_pts.need(n);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));   // (the previous call's copy out of h_pts, before it is overwritten or freed)
    rc = h_pts.need(n);
    if (rc) return rc;
    float pose[VIS_MAX_VIEWS * 12];
    size_t o = 0;
    for (size_t v = 0; v < n_views; ++v) {
        std::memcpy(pose + 12 * v, views[v].R, 9 * sizeof(float));
        std::memcpy(pose + 12 * v + 9, views[v].t, 3 * sizeof(float));
        const char* b = static_cast<const char*>(views[v].points);
        for (size_t i = 0; i < views[v].n; ++i, ++o) {
            float xyz[3];
            std::memcpy(xyz, b + i * views[v].stride, sizeof(xyz));
            h_pts[o] = make_float4(xyz[0], xyz[1], xyz[2], 0.f);
            uint32_t vi = (uint32_t)v;
            std::memcpy(&h_pts[o].w, &vi, sizeof(vi));
        }
    }
    // (pose is a stack array: the copy must have landed before this frame returns)
    LV_HIP(hipMemcpyAsync(d_blob, pose, n_views * 12 * sizeof(float), hipMemcpyHostToDevice, stream));
    float* img = reinterpret_cast<float*>(static_cast<char*>(d_blob.p) + pose_bytes);
    LV_HIP(hipMemsetD32Async((hipDeviceptr_t)img, 0x7F800000, pixels, stream));
    if (n) {
        LV_HIP(hipMemcpyAsync(d_pts, h_pts, n * sizeof(float4), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(vis_image_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_pts, (uint32_t)n, q, reinterpret_cast<uint32_t*>(img));
        LV_HIP(hipGetLastError());
    }
    if (q.window > 0) {
        hipLaunchKernelGGL(vis_min_cols_kernel, dim3(blocks_of(pixels)), dim3(256), 0, stream, img, d_tmp, (uint32_t)pixels, q.width, q.window);
        hipLaunchKernelGGL(vis_min_rows_kernel, dim3(blocks_of(pixels)), dim3(256), 0, stream, d_tmp, img, (uint32_t)pixels, q.width, q.height,
                           q.window);
        LV_HIP(hipGetLastError());
    }
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int VisStore::ensure_hits(size_t n) { return d_hits.need(n); }

void VisStore::release() {
    h_pts.release();
    d_pts.release();
    d_blob.release();
    d_tmp.release();
    d_hits.release();
}

int vis_classify(MapStore& map, hipStream_t stream, const void* d_blob, const VisRule& q, const uint32_t* rank, uint8_t* hits, bool remove,
                 uint32_t* n_removed) {
    if (n_removed) *n_removed = 0;
    if (!map.built || map.m == 0) return LV_OK;
    int rc = map.ensure_counters();
    if (rc) return rc;
    rc = map.reset_batch_counters(stream);
    if (rc) return rc;
    const float* pose = static_cast<const float*>(d_blob);
    const float* img = reinterpret_cast<const float*>(static_cast<const char*>(d_blob) + vis_pose_bytes(q.n_views));
    hipLaunchKernelGGL(vis_classify_kernel, dim3(blocks_of(map.n_ids)), dim3(256), 0, stream, map.d_orig, map.n_ids, pose, img, q, rank, hits,
                       remove ? 1 : 0, map.d_dead, (uint32_t)map.d_dead.cap, map.d_cnt);
    LV_HIP(hipGetLastError());
    if (!remove) {
        LV_HIP(hipStreamSynchronize(stream));
        return LV_OK;
    }
    return map.retire_dead_list(stream, n_removed);
}

}  // namespace lv
