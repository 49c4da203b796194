// lv_paint.hpp — colours for the map's points from camera images (lv_map_paint, include/limovelo_hip.h "Map painting"; kernels
// and host side in lv_paint.hip).
#pragma once
#include "lv_host.hpp"
#include "lv_rules.hpp"   // PAINT_MAX_*, PaintCam, PaintRule

namespace lv {

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
