// lv_colour.hpp — the colour layer of the TSDF volume and the vertex colours of its mesh (lv_colour_*, lv_mesh_colours,
// include/limovelo_hip.h "Colour layer"; kernels and host side in lv_colour.hip, the layer itself a member of TsdfStore).
//
// The rule's integer steps as plain __host__ __device__ code: the candidate test, the voxel centre, the quantisation of a sample,
// the fold, the voxel colour and the vertex colour.  The kernels of lv_colour.hip run exactly these; tests/emu/colour_emu.cpp
// compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_colour_host.py holds them to tests/colour_ref.py.
// The one float step before them, the projection and the bilinear sample, is lv_paint_dev.hpp's.
#pragma once

#include "lv_tsdf.hpp"

namespace lv {

constexpr int COLOUR_MAX_WEIGHT = 65535;

// W >= min_weight and |S| <= band * W
LV_OCC_HD bool colour_candidate(int32_t S, int32_t W, int32_t min_weight, int32_t band) {
    if (W < min_weight) return false;
    const int64_t s = S;
    return (s < 0 ? -s : s) <= (int64_t)band * (int64_t)W;
}

// The centre of voxel index i along one axis: tsdf_vertex_metres at v = 256 i + 128
LV_OCC_HD float colour_centre(float origin, float resolution, int i) { return tsdf_vertex_metres(origin, resolution, 256 * i + 128); }

// A sample s in [0, 255] to its level 0..255
LV_OCC_HD uint32_t colour_quant(float s) {
    const uint32_t q = (uint32_t)(s + 0.5f);
    return q > 255u ? 255u : q;
}

// The fold of one voxel's entry e = (C[0], C[1], C[2], Wc) with n > 0 seeing views whose levels sum to dC
LV_OCC_HD void colour_fold(uint32_t max_weight, uint32_t n, const uint32_t dC[3], uint32_t e[4]) {
    const uint32_t Wn = e[3] + n;
    for (int c = 0; c < 3; ++c) {
        const uint32_t Cn = e[c] + dC[c];
        e[c] = Wn > max_weight ? (uint32_t)(((uint64_t)Cn * (uint64_t)max_weight) / (uint64_t)Wn) : Cn;
    }
    e[3] = Wn > max_weight ? max_weight : Wn;
}

// r, g, b, a packed with r in the lowest byte: the byte order of the rgba outputs
LV_OCC_HD uint32_t colour_pack(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

// The colour of a voxel with entry e
LV_OCC_HD uint32_t colour_voxel(const uint32_t e[4]) {
    const uint32_t w = e[3];
    if (w == 0) return 0u;
    return colour_pack((2u * e[0] + w) / (2u * w), (2u * e[1] + w) / (2u * w), (2u * e[2] + w) / (2u * w), 255u);
}

// The colour of the vertex of an active cell from the entries of its 8 corner voxels
LV_OCC_HD uint32_t colour_vertex(const uint32_t e[8][4]) {
    uint32_t k = 0, sum[3] = {0, 0, 0};
    for (int n = 0; n < 8; ++n) {
        if (e[n][3] == 0) continue;
        const uint32_t v = colour_voxel(e[n]);
        sum[0] += v & 0xFFu;
        sum[1] += (v >> 8) & 0xFFu;
        sum[2] += (v >> 16) & 0xFFu;
        ++k;
    }
    if (k == 0) return 0u;
    return colour_pack((2u * sum[0] + k) / (2u * k), (2u * sum[1] + k) / (2u * k), (2u * sum[2] + k) / (2u * k), 255u);
}

inline void default_colour_params(lv_colour_params* p) {
    if (!p) return;
    *p = lv_colour_params{};
    default_paint_params(&p->view);
    p->view.zbuf_scale = 8;
    p->view.window = 1;
    p->view.margin_abs = 0.5f;
    p->band = 256;
    p->min_weight = 1;
    p->max_weight = 64;
}

// lv_colour_integrate's arguments against their limits, before the context: LV_EINVAL (nothing written) outside them; inside, the
// views' rule as the kernels take it (paint_rule).  band is held to the volume's T later, by VolumeTools.
inline int colour_rule(const lv_camera_view* views, size_t n_views, const lv_colour_params* p, PaintRule* q, PaintCam* cams) {
    if (!views || !p) { set_error("lv_colour_integrate: null argument"); return LV_EINVAL; }
    if (int rc = paint_rule(views, n_views, &p->view, q, cams)) return rc;
    if (p->view.blend != 0) { set_error("lv_colour_integrate: blend = %d: the layer takes the mean, blend 0", p->view.blend); return LV_EINVAL; }
    if (p->band < 1 || p->band > TSDF_MAX_TRUNC * 256) { set_error("lv_colour_integrate: band = %d: must be in 1..T", p->band); return LV_EINVAL; }
    if (p->min_weight < 1) { set_error("lv_colour_integrate: min_weight = %d: at least 1", p->min_weight); return LV_EINVAL; }
    if (p->max_weight < 1 || p->max_weight > COLOUR_MAX_WEIGHT) { set_error("lv_colour_integrate: max_weight = %d: must be in 1..65535", p->max_weight); return LV_EINVAL; }
    return LV_OK;
}

// The first voxel lv_colour_load refuses (Wc > 65535 or a sum above 255 * Wc), or n when every voxel holds
inline size_t colour_check_layer(const uint32_t* sums, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const uint32_t* e = sums + 4 * i;
        if (e[3] > (uint32_t)COLOUR_MAX_WEIGHT || e[0] > 255u * e[3] || e[1] > 255u * e[3] || e[2] > 255u * e[3]) return i;
    }
    return n;
}

}  // namespace lv
