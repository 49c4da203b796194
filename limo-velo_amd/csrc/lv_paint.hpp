// lv_paint.hpp — colours for the map's points from camera images (lv_map_paint, include/limovelo_hip.h "Map painting"; kernels
// and host side in lv_paint.hip).
#pragma once
#include "lv_host.hpp"

namespace lv {

constexpr int PAINT_MAX_VIEWS = 32;
constexpr int PAINT_MAX_SIDE = 8192;                           // width and height of one image
constexpr size_t PAINT_MAX_PIXELS = (size_t)1 << 24;           // width * height of one image
constexpr size_t PAINT_MAX_TOTAL_PIXELS = (size_t)1 << 26;     // all images of a call together
constexpr int PAINT_MAX_SCALE = 16;
constexpr int PAINT_MAX_WINDOW = 8;

// One view as the kernels take it (128 B): the pose, the camera, and where its texels and occlusion cells sit in the call's
// buffers.  wm1 / hm1: width - 1 / height - 1 as f32 (the image test of the rule's step 3).
struct PaintCam {
    float R[9], t[3];
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float wm1, hm1;
    int width, height;
    int cw, ch;                // occlusion cells: ceil(width / s) x ceil(height / s)
    int format;                // LV_IMAGE_*
    uint32_t tex_off;          // first texel of the view (packed 0x00BBGGRR, one per pixel)
    uint32_t cell_off;         // first cell of the view
    uint32_t raw_off;          // first staged byte of the view (rows of width * channels bytes, back to back)
    uint32_t pad;
};
static_assert(sizeof(PaintCam) == 128, "PaintCam is 128 B");

// The call's parameters (r2_max = max_norm_radius^2 in f32, s = zbuf_scale as f32)
struct PaintRule {
    int n_views, window, blend;
    float min_depth, max_depth, r2_max, s, margin_abs, margin_rel;
    uint32_t max_pixels, max_cells;   // the largest view's pixels / cells (the grids of the per-view kernels)
    size_t total_pixels, total_cells, raw_bytes;
};

// The buffers of lv_map_paint (grown on demand, kept; released by lv_destroy): staged image bytes (pinned and on the device),
// the views, the packed texels, the occlusion cells and their filter's intermediate, the outputs by rank.
struct PaintStore {
    PinBuf<uint8_t> h_raw;
    PinBuf<PaintCam> h_cams;      // PAINT_MAX_VIEWS entries
    DevBuf<uint8_t> d_raw;
    DevBuf<PaintCam> d_cams;
    DevBuf<uint32_t> d_tex;
    DevBuf<uint32_t> d_cell;
    DevBuf<uint32_t> d_tmp;
    DevBuf<float> d_rgb;
    DevBuf<float> d_depth;
    DevBuf<uint8_t> d_seen;
    // Stages and unpacks the images, builds the occlusion buffers from every living point of `map` and writes the outputs of its
    // m living points at their ranks (rank NULL: ranks are ids) into d_rgb / d_depth / d_seen (those wanted), on `stream`.
    // cams: the views (tex_off, cell_off and raw_off filled in by the caller).  Synchronises the stream.
    int run(const MapStore& map, hipStream_t stream, const lv_camera_view* views, const PaintCam* cams, const PaintRule& q,
            const uint32_t* rank, bool want_rgb, bool want_depth, bool want_seen);
    void release();
};

}  // namespace lv
