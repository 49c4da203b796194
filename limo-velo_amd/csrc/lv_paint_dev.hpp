// lv_paint_dev.hpp — what projects a world point into a camera view and reads the view's image, shared by lv_paint.hip (the map's
// points) and lv_colour.hip (the TSDF volume's voxel centres): steps 1 to 4 and 6 of include/limovelo_hip.h "Map painting", the
// unpack of the staged image bytes and the separable window-min of the occlusion buffers.  Both files project through the same
// inline paint_project, so z, u and v are the same bits in a zbuf pass and the colour pass that follows it, and a cell's foremost
// point always finds itself in front.  Device code only; the kernels have internal linkage, each file gets its own.
#pragma once
#include <cstring>

#include "lv_common.hpp"
#include "lv_rules.hpp"   // PaintCam, PaintRule

namespace lv {

// The images' rows, back to back, at every view's raw_off of h_raw (one copy when the caller's rows already are)
inline void paint_stage_images(const lv_camera_view* views, const PaintCam* cams, const PaintRule& q, uint8_t* h_raw) {
    for (int w = 0; w < q.n_views; ++w) {
        const lv_camera_view& v = views[w];
        const size_t row = (size_t)v.width * (v.format == LV_IMAGE_MONO8 ? 1 : 3);
        uint8_t* dst = h_raw + cams[w].raw_off;
        const uint8_t* src = static_cast<const uint8_t*>(v.image);
        if (v.row_stride == row) {
            std::memcpy(dst, src, row * (size_t)v.height);
        } else {
            for (int y = 0; y < v.height; ++y) std::memcpy(dst + (size_t)y * row, src + (size_t)y * v.row_stride, row);
        }
    }
}

namespace {

// Steps 1-3 of the rule: the camera-frame depth z and the pixel coordinates (u, v) of world point p; false when the view does not
// judge it.  Every sum left to right, nothing fused (-ffp-contract=off).
__device__ __forceinline__ bool paint_project(const PaintCam& c, const PaintRule& q, const float4& p, float& z, float& u, float& v) {
    const float dx = p.x - c.t[0], dy = p.y - c.t[1], dz = p.z - c.t[2];
    const float X = c.R[0] * dx + c.R[3] * dy + c.R[6] * dz;   // R^T d
    const float Y = c.R[1] * dx + c.R[4] * dy + c.R[7] * dz;
    z = c.R[2] * dx + c.R[5] * dy + c.R[8] * dz;
    if (!(z >= q.min_depth && z <= q.max_depth)) return false;
    const float x = X / z, y = Y / z;
    const float r2 = x * x + y * y;
    if (!(r2 <= q.r2_max)) return false;
    const float r4 = r2 * r2, r6 = r4 * r2;
    const float cd = 1.f + c.k1 * r2 + c.k2 * r4 + c.k3 * r6;
    const float xy = x * y;
    const float xd = x * cd + 2.f * c.p1 * xy + c.p2 * (r2 + 2.f * x * x);
    const float yd = y * cd + c.p1 * (r2 + 2.f * y * y) + 2.f * c.p2 * xy;
    u = c.fx * xd + c.cx;
    v = c.fy * yd + c.cy;
    return u >= 0.f && u <= c.wm1 && v >= 0.f && v <= c.hm1;
}

// Step 4: the cell of pixel coordinates (u, v) inside [0, W-1] x [0, H-1] (clamped: f32 rounding cannot take it past the last cell,
// the clamp only keeps every index inside the buffer)
__device__ __forceinline__ uint32_t paint_cell(const PaintCam& c, const PaintRule& q, float u, float v) {
    int cx = (int)floorf((u + 0.5f) / q.s), cy = (int)floorf((v + 0.5f) / q.s);
    cx = cx < 0 ? 0 : (cx >= c.cw ? c.cw - 1 : cx);
    cy = cy < 0 ? 0 : (cy >= c.ch ? c.ch - 1 : cy);
    return c.cell_off + (uint32_t)cy * (uint32_t)c.cw + (uint32_t)cx;
}

// grid (pixels of the largest view / 256, n_views); raw: rows of width * channels bytes, back to back
__global__ __launch_bounds__(256) void paint_unpack_kernel(const uint8_t* __restrict__ raw, const PaintCam* __restrict__ cams,
                                                           uint32_t* __restrict__ tex) {
    const PaintCam& c = cams[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = (uint32_t)c.width * (uint32_t)c.height;
    if (i >= n) return;
    uint32_t r, g, b;
    if (c.format == LV_IMAGE_MONO8) {
        r = g = b = raw[c.raw_off + i];
    } else {
        const uint8_t* s = raw + c.raw_off + 3u * i;
        r = s[0];
        g = s[1];
        b = s[2];
        if (c.format == LV_IMAGE_BGR8) { const uint32_t x = r; r = b; b = x; }
    }
    tex[c.tex_off + i] = r | (g << 8) | (b << 16);
}

// grid (cells of the largest view / 256, n_views): out[cell] = min of in over the cells cx - w .. cx + w of its row (clipped)
__global__ __launch_bounds__(256) void paint_min_x_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const PaintCam* __restrict__ cams,
                                                          int w) {
    const PaintCam& c = cams[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)c.cw * (uint32_t)c.ch) return;
    const int cx = (int)(i % (uint32_t)c.cw);
    const uint32_t k = c.cell_off + i;
    uint32_t m = in[k];
    for (int d = 1; d <= w; ++d) {
        if (cx + d < c.cw) m = min(m, in[k + (uint32_t)d]);
        if (cx - d >= 0) m = min(m, in[k - (uint32_t)d]);
    }
    out[k] = m;
}

// grid (cells of the largest view / 256, n_views): out[cell] = min of in over the cells cy - w .. cy + w of its column (clipped)
__global__ __launch_bounds__(256) void paint_min_y_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const PaintCam* __restrict__ cams,
                                                          int w) {
    const PaintCam& c = cams[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)c.cw * (uint32_t)c.ch) return;
    const int cy = (int)(i / (uint32_t)c.cw);
    const uint32_t k = c.cell_off + i;
    const uint32_t row = (uint32_t)c.cw;
    uint32_t m = in[k];
    for (int d = 1; d <= w; ++d) {
        if (cy + d < c.ch) m = min(m, in[k + (uint32_t)d * row]);
        if (cy - d >= 0) m = min(m, in[k - (uint32_t)d * row]);
    }
    out[k] = m;
}

__device__ __forceinline__ float3 paint_texel(uint32_t t) {
    return make_float3((float)(t & 0xFFu), (float)((t >> 8) & 0xFFu), (float)((t >> 16) & 0xFFu));
}

// Step 6: the bilinear sample at (u, v) inside [0, W-1] x [0, H-1], taps clamped to the image:
// a = t00 + fx (t10 - t00), b = t01 + fx (t11 - t01), sample = a + fy (b - a)
__device__ __forceinline__ float3 paint_sample(const PaintCam& c, const uint32_t* __restrict__ tex, float u, float v) {
    int x0 = (int)floorf(u), y0 = (int)floorf(v);
    x0 = x0 < 0 ? 0 : (x0 > c.width - 1 ? c.width - 1 : x0);
    y0 = y0 < 0 ? 0 : (y0 > c.height - 1 ? c.height - 1 : y0);
    const float fx = u - (float)x0, fy = v - (float)y0;
    const int x1 = x0 + 1 < c.width ? x0 + 1 : x0, y1 = y0 + 1 < c.height ? y0 + 1 : y0;
    const uint32_t* T = tex + c.tex_off;
    const uint32_t W = (uint32_t)c.width;
    const float3 t00 = paint_texel(T[(uint32_t)y0 * W + (uint32_t)x0]), t10 = paint_texel(T[(uint32_t)y0 * W + (uint32_t)x1]);
    const float3 t01 = paint_texel(T[(uint32_t)y1 * W + (uint32_t)x0]), t11 = paint_texel(T[(uint32_t)y1 * W + (uint32_t)x1]);
    float3 a, b, s;
    a.x = t00.x + fx * (t10.x - t00.x);
    a.y = t00.y + fx * (t10.y - t00.y);
    a.z = t00.z + fx * (t10.z - t00.z);
    b.x = t01.x + fx * (t11.x - t01.x);
    b.y = t01.y + fx * (t11.y - t01.y);
    b.z = t01.z + fx * (t11.z - t01.z);
    s.x = a.x + fy * (b.x - a.x);
    s.y = a.y + fy * (b.y - a.y);
    s.z = a.z + fy * (b.z - a.z);
    return s;
}

}  // namespace

}  // namespace lv
