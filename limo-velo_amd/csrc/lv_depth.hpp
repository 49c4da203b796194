// lv_depth.hpp — depth-camera images fused into the TSDF volume (lv_depth_integrate, include/limovelo_hip.h "Depth fusion"; the
// kernel and the host side in lv_depth.hip, the call a member of TsdfStore).
//
// The rule's scalar steps as plain __host__ __device__ code: the measured depth of a raw pixel and its validity, the quantised
// distance with its three outcomes, and the two shortcuts (which views a box of voxels can be judged by, which voxels a view can
// judge at all).  The kernel of lv_depth.hip runs exactly these; tests/emu/depth_emu.cpp compiles them with g++ through
// tests/emu/hip/hip_runtime.h and tests/test_depth_host.py holds them to tests/depth_ref.py.  The centre is lv_colour.hpp's, the
// projection lv_paint_dev.hpp's, the fold lv_tsdf.hpp's.
#pragma once

#include "lv_colour.hpp"

namespace lv {

// Step 4: D is valid iff min_depth <= D <= max_depth; NaN, +-inf, 0 and negatives fall out by this comparison (max_depth is finite)
LV_OCC_HD bool depth_valid(float D, float min_depth, float max_depth) { return D >= min_depth && D <= max_depth; }

// LV_DEPTH_U16: raw 0 is "no measurement", otherwise D = (float)raw * scale
LV_OCC_HD bool depth_of_u16(uint16_t raw, float scale, float min_depth, float max_depth, float& D) {
    if (raw == 0) return false;
    D = (float)raw * scale;
    return depth_valid(D, min_depth, max_depth);
}

// LV_DEPTH_F32: the value itself
LV_OCC_HD bool depth_of_f32(float raw, float min_depth, float max_depth, float& D) {
    D = raw;
    return depth_valid(D, min_depth, max_depth);
}

// Step 5: q = floorf(((D - z) / resolution) * 256) in exactly that order, judged in f32 against T.  false: no contribution
// (behind the band, or in front of it without carve)
LV_OCC_HD bool depth_quant(float D, float z, float resolution, int32_t T, int carve, int32_t& s) {
    const float q = floorf(((D - z) / resolution) * OCC_SUB);
    const float t = (float)T;
    if (q < -t) return false;
    if (q > t) {
        if (!carve) return false;
        s = T;
        return true;
    }
    s = (int32_t)q;
    return true;
}

// ---- the shortcuts.  A point d = p - t that passes step 2 has z = a . d in [min_depth, max_depth] and |X| <= rho z, |Y| <= rho z
// with X = b . d, Y = c . d and rho = max_norm_radius (x^2 + y^2 <= rho^2 bounds each of them), where b, c, a are the columns of
// R: six half-spaces, whatever R is.  A box none of whose points is in one of them, by a margin far above the rounding of the
// kernel's f32 steps (1e-3 of the terms' magnitudes against 1e-6), is judged by nobody.  Neither shortcut changes a result.

// n . d over the box with centre m - t = d0 and half widths h: its least value, less the margin.  w >= |n| per component: the
// magnitudes of the terms n is made of
LV_OCC_HD float depth_plane_min(const float n[3], const float w[3], const float d0[3], const float h[3]) {
    const float mid = n[0] * d0[0] + n[1] * d0[1] + n[2] * d0[2];
    const float ext = fabsf(n[0]) * h[0] + fabsf(n[1]) * h[1] + fabsf(n[2]) * h[2];
    const float mag = w[0] * (fabsf(d0[0]) + h[0]) + w[1] * (fabsf(d0[1]) + h[1]) + w[2] * (fabsf(d0[2]) + h[2]);
    return mid - ext - (1e-3f * mag + 1e-6f);
}

// true: the view judges no point of the box of metres [lo, hi]
LV_OCC_HD bool depth_box_unseen(const PaintCam& c, float min_depth, float max_depth, float rho, const float lo[3], const float hi[3]) {
    float d0[3], h[3];
    for (int a = 0; a < 3; ++a) {
        d0[a] = 0.5f * (lo[a] + hi[a]) - c.t[a];
        h[a] = 0.5f * (hi[a] - lo[a]);
    }
    const float a[3] = {c.R[2], c.R[5], c.R[8]}, na[3] = {-a[0], -a[1], -a[2]}, wa[3] = {fabsf(a[0]), fabsf(a[1]), fabsf(a[2])};
    if (depth_plane_min(a, wa, d0, h) > max_depth) return true;      // z > max_depth everywhere
    if (depth_plane_min(na, wa, d0, h) > -min_depth) return true;    // z < min_depth everywhere
    for (int col = 0; col < 2; ++col) {
        const float b[3] = {c.R[col], c.R[3 + col], c.R[6 + col]};
        const float p[3] = {b[0] - rho * a[0], b[1] - rho * a[1], b[2] - rho * a[2]}, m[3] = {-b[0] - rho * a[0], -b[1] - rho * a[1], -b[2] - rho * a[2]};
        const float w[3] = {fabsf(b[0]) + rho * wa[0], fabsf(b[1]) + rho * wa[1], fabsf(b[2]) + rho * wa[2]};
        if (depth_plane_min(p, w, d0, h) > 0.f) return true;   // X > rho z everywhere
        if (depth_plane_min(m, w, d0, h) > 0.f) return true;   // -X > rho z everywhere
    }
    return false;
}

// The voxels [lo, hi) per axis a view can judge: the box of the pyramid 0 <= z <= max_depth, |X|, |Y| <= rho z (its apex and the
// four corners at max_depth, through R's inverse in f64), widened by a voxel and 1e-3 of its size, clipped to the grid.
// false: none.  A singular R gives the whole grid.
inline bool depth_view_box(const TsdfGrid& g, const PaintCam& c, float max_depth, float rho, int lo[3], int hi[3]) {
    const int n[3] = {g.occ.nx, g.occ.ny, g.occ.nz};
    const double m[9] = {c.R[0], c.R[3], c.R[6], c.R[1], c.R[4], c.R[7], c.R[2], c.R[5], c.R[8]};   // rows b, c, a: (X, Y, z) = m d
    const double co[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                          m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                          m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};   // the adjugate, row-major
    const double det = m[0] * co[0] + m[1] * co[3] + m[2] * co[6];
    double scale = 0.0;
    for (int i = 0; i < 9; ++i) scale = std::fmax(scale, std::fabs(m[i]));
    double dlo[3] = {0.0, 0.0, 0.0}, dhi[3] = {0.0, 0.0, 0.0};   // (the apex)
    const bool whole = !(std::fabs(det) > 1e-6 * scale * scale * scale);
    for (int k = 0; k < 4 && !whole; ++k) {
        const double X = (k & 1 ? 1.0 : -1.0) * (double)rho * (double)max_depth, Y = (k & 2 ? 1.0 : -1.0) * (double)rho * (double)max_depth, z = max_depth;
        for (int a = 0; a < 3; ++a) {
            const double d = (co[3 * a] * X + co[3 * a + 1] * Y + co[3 * a + 2] * z) / det;
            dlo[a] = std::fmin(dlo[a], d);
            dhi[a] = std::fmax(dhi[a], d);
        }
    }
    for (int a = 0; a < 3; ++a) {
        lo[a] = 0;
        hi[a] = n[a];
        if (whole) continue;
        const double res = g.occ.resolution, slack = res + 1e-3 * (dhi[a] - dlo[a]) + 1e-3 * std::fabs((double)c.t[a] - (double)g.occ.origin[a]);
        // centre i sits at origin + (i + 0.5) res
        const double flo = std::floor(((double)c.t[a] + dlo[a] - slack - (double)g.occ.origin[a]) / res - 0.5);
        const double fhi = std::ceil(((double)c.t[a] + dhi[a] + slack - (double)g.occ.origin[a]) / res - 0.5) + 1.0;
        if (!(flo < (double)n[a]) || !(fhi > 0.0)) return false;
        if (flo > 0.0) lo[a] = (int)flo;
        if (fhi < (double)n[a]) hi[a] = (int)fhi;
    }
    return true;
}

inline void default_depth_params(lv_depth_params* p) {
    if (!p) return;
    *p = lv_depth_params{};
    p->min_depth = 0.3f;
    p->max_depth = 10.f;
    p->max_norm_radius = 1.5f;
    p->carve = 0;
}

constexpr int DEPTH_MAX_VIEWS = PAINT_MAX_VIEWS;

inline size_t depth_pixel_bytes(int format) { return format == LV_DEPTH_U16 ? 2 : 4; }

// lv_depth_integrate's arguments against their limits, before the context: LV_EINVAL (nothing written) outside them; inside, the
// rule as the kernel takes it and every view's place in the staged bytes
inline int depth_rule(const lv_depth_view* views, size_t n_views, const lv_depth_params* p, DepthRule* q, DepthCam* cams) {
    if (!views || !p) { set_error("lv_depth_integrate: null argument"); return LV_EINVAL; }
    if (n_views < 1 || n_views > (size_t)DEPTH_MAX_VIEWS) { set_error("lv_depth_integrate: n_views = %zu: must be in 1..%d", n_views, DEPTH_MAX_VIEWS); return LV_EINVAL; }
    if (!(std::isfinite(p->min_depth) && std::isfinite(p->max_depth) && p->min_depth > 0.f && p->min_depth < p->max_depth)) {
        set_error("lv_depth_integrate: depths [%g, %g]: finite, 0 < min_depth < max_depth", p->min_depth, p->max_depth);
        return LV_EINVAL;
    }
    if (!(std::isfinite(p->max_norm_radius) && p->max_norm_radius > 0.f)) { set_error("lv_depth_integrate: max_norm_radius = %g: finite and > 0", p->max_norm_radius); return LV_EINVAL; }
    if (p->carve != 0 && p->carve != 1) { set_error("lv_depth_integrate: carve = %d: 0 or 1", p->carve); return LV_EINVAL; }
    size_t pixels = 0, raw = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const lv_depth_view& w = views[v];
        for (int i = 0; i < 9; ++i) if (!std::isfinite(w.R[i])) { set_error("lv_depth_integrate: view %zu: non-finite R", v); return LV_EINVAL; }
        for (int i = 0; i < 3; ++i) if (!std::isfinite(w.t[i])) { set_error("lv_depth_integrate: view %zu: non-finite t", v); return LV_EINVAL; }
        if (!(std::isfinite(w.fx) && std::isfinite(w.fy) && std::isfinite(w.cx) && std::isfinite(w.cy))) { set_error("lv_depth_integrate: view %zu: non-finite intrinsics", v); return LV_EINVAL; }
        for (int i = 0; i < 5; ++i) if (!std::isfinite(w.dist[i])) { set_error("lv_depth_integrate: view %zu: non-finite distortion", v); return LV_EINVAL; }
        if (w.width < 1 || w.height < 1 || w.width > PAINT_MAX_SIDE || w.height > PAINT_MAX_SIDE || (size_t)w.width * (size_t)w.height > PAINT_MAX_PIXELS) {
            set_error("lv_depth_integrate: view %zu: image of %d x %d pixels: each side 1..%d, at most 2^24 in all", v, w.width, w.height, PAINT_MAX_SIDE);
            return LV_EINVAL;
        }
        if (w.format != LV_DEPTH_U16 && w.format != LV_DEPTH_F32) { set_error("lv_depth_integrate: view %zu: format %d", v, w.format); return LV_EINVAL; }
        if (w.format == LV_DEPTH_U16 && !(std::isfinite(w.depth_scale) && w.depth_scale > 0.f)) {
            set_error("lv_depth_integrate: view %zu: depth_scale = %g: finite and > 0", v, w.depth_scale);
            return LV_EINVAL;
        }
        const size_t row = (size_t)w.width * depth_pixel_bytes(w.format);
        if (!w.depth || w.row_stride < row) { set_error("lv_depth_integrate: view %zu: null depth or row_stride %zu < %zu", v, w.row_stride, row); return LV_EINVAL; }
        pixels += (size_t)w.width * (size_t)w.height;
        if (pixels > PAINT_MAX_TOTAL_PIXELS) { set_error("lv_depth_integrate: the views hold more than 2^26 pixels together"); return LV_EINVAL; }
        DepthCam& c = cams[v];
        std::memset(&c, 0, sizeof(c));
        c.cam = paint_cam_of(w.R, w.t, w.fx, w.fy, w.cx, w.cy, w.dist, w.width, w.height);
        c.cam.format = w.format;
        c.cam.raw_off = (uint32_t)raw;
        c.scale = w.format == LV_DEPTH_U16 ? w.depth_scale : 1.f;
        raw += (row * (size_t)w.height + 255) & ~(size_t)255;
    }
    *q = DepthRule{};
    q->view.n_views = (int)n_views;
    q->view.min_depth = p->min_depth;
    q->view.max_depth = p->max_depth;
    q->view.r2_max = p->max_norm_radius * p->max_norm_radius;
    q->rho = p->max_norm_radius;
    q->carve = p->carve;
    q->raw_bytes = raw;
    return LV_OK;
}

// The images' rows, back to back, at every view's raw_off of h_raw (one copy when the caller's rows already are)
inline void depth_stage_images(const lv_depth_view* views, const DepthCam* cams, int n_views, uint8_t* h_raw) {
    for (int w = 0; w < n_views; ++w) {
        const lv_depth_view& v = views[w];
        const size_t row = (size_t)v.width * depth_pixel_bytes(v.format);
        uint8_t* dst = h_raw + cams[w].cam.raw_off;
        const uint8_t* src = static_cast<const uint8_t*>(v.depth);
        if (v.row_stride == row) {
            std::memcpy(dst, src, row * (size_t)v.height);
        } else {
            for (int y = 0; y < v.height; ++y) std::memcpy(dst + (size_t)y * row, src + (size_t)y * v.row_stride, row);
        }
    }
}

}  // namespace lv
