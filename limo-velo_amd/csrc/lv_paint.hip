// lv_paint.hip — lv_map_paint: the map's points take the colour of the camera images that see them (include/limovelo_hip.h
// "Map painting"; the reference's TODO "Add vision buffer and ability to paint the map's points").
//
// Five kernels, one lane per item, no float atomics, no scratch:
//   paint_unpack_kernel  one lane per pixel (every view at once: blockIdx.y is the view): the staged rgb8 / bgr8 / mono8 bytes
//                        become one packed texel 0x00BBGGRR per pixel, so that each bilinear tap is one dword load;
//   paint_zbuf_kernel    one lane per id: reads orig once, loops over the views, atomicMin of the z bits into the point's cell
//                        (a positive f32 orders like its bit pattern; +inf = empty): order-independent, deterministic;
//   paint_min_x_kernel   the clipped window-min, separable: along the rows of cells, then
//   paint_min_y_kernel   along the columns;
//   paint_color_kernel   one lane per id: reads orig once, loops over the views, the occlusion test, the bilinear sample and the
//                        blend; writes the outputs at the point's living rank.
// paint_zbuf_kernel and paint_color_kernel project through the same inline paint_project, so z, u and v are the same bits in
// both passes and a cell's foremost point always finds itself in front.  The projection, the sample, the unpack and the two
// window-min kernels are lv_paint_dev.hpp's, which lv_colour.hip runs too.  The living-id test is pt_alive (lv_mapinc.hpp).  The
// file walks no neighbourhood, so it takes nothing from lv_query_dev.hpp: its one rank lookup stays a ternary.
#include "lv_paint.hpp"

#include <cstring>

#include "lv_paint_dev.hpp"

namespace lv {

namespace {

// one lane per id; cell: every view's cells, initialised to +inf
__global__ __launch_bounds__(256) void paint_zbuf_kernel(const float4* __restrict__ orig, uint32_t n_ids, const PaintCam* __restrict__ cams,
                                                         PaintRule q, uint32_t* __restrict__ cell) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const float4 p = orig[id];
    if (!pt_alive(p)) return;
    for (int w = 0; w < q.n_views; ++w) {
        const PaintCam& c = cams[w];
        float z, u, v;
        if (!paint_project(c, q, p, z, u, v)) continue;
        atomicMin(&cell[paint_cell(c, q, u, v)], __float_as_uint(z));
    }
}

// One lane per id.  cell: the window-min occlusion buffers; rank: NULL (ranks are ids) or the rank among the living by id.
// rgb / depth / seen: NULL or m entries by rank.
__global__ __launch_bounds__(256) void paint_color_kernel(const float4* __restrict__ orig, uint32_t n_ids, const PaintCam* __restrict__ cams,
                                                          PaintRule q, const uint32_t* __restrict__ cell, const uint32_t* __restrict__ tex,
                                                          const uint32_t* __restrict__ rank, float* __restrict__ rgb, float* __restrict__ depth,
                                                          uint8_t* __restrict__ seen) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const float4 p = orig[id];
    if (!pt_alive(p)) return;
    uint32_t n = 0;
    float best = pos_inf();
    float3 acc = make_float3(0.f, 0.f, 0.f);
    for (int w = 0; w < q.n_views; ++w) {
        const PaintCam& c = cams[w];
        float z, u, v;
        if (!paint_project(c, q, p, z, u, v)) continue;
        const float zw = __uint_as_float(cell[paint_cell(c, q, u, v)]);
        if (!(z - zw <= fmaxf(q.margin_abs, q.margin_rel * z))) continue;
        ++n;
        if (rgb) {
            const float3 s = paint_sample(c, tex, u, v);
            if (q.blend == 0) {
                acc.x = acc.x + s.x;
                acc.y = acc.y + s.y;
                acc.z = acc.z + s.z;
            } else if (z < best) {
                acc = s;
            }
        }
        best = fminf(best, z);
    }
    if (q.blend == 0 && n > 0) {
        const float fn = (float)n;
        acc.x = acc.x / fn;
        acc.y = acc.y / fn;
        acc.z = acc.z / fn;
    }
    const uint32_t k = rank ? rank[id] : id;
    if (rgb) {
        rgb[3u * k + 0u] = acc.x;
        rgb[3u * k + 1u] = acc.y;
        rgb[3u * k + 2u] = acc.z;
    }
    if (depth) depth[k] = best;
    if (seen) seen[k] = (uint8_t)n;
}

}  // namespace

int PaintStore::run(const MapStore& map, hipStream_t stream, const lv_camera_view* views, const PaintCam* cams, const PaintRule& q,
                    const uint32_t* rank, bool want_rgb, bool want_depth, bool want_seen) {
    const size_t m = map.m;
    int rc = d_raw.need(q.raw_bytes);
    if (!rc) rc = d_tex.need(q.total_pixels);
    if (!rc) rc = d_cell.need(q.total_cells);
    if (!rc && q.window > 0) rc = d_tmp.need(q.total_cells);
    if (!rc && want_rgb) rc = d_rgb.need(3 * m);
    if (!rc && want_depth) rc = d_depth.need(m);
    if (!rc && want_seen) rc = d_seen.need(m);
    if (!rc) rc = d_cams.need(PAINT_MAX_VIEWS);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));   // (the previous call's copies out of the pinned buffers)
    rc = h_cams.need(PAINT_MAX_VIEWS);
    if (!rc) rc = h_raw.need(q.raw_bytes);
    if (rc) return rc;
    paint_stage_images(views, cams, q, h_raw);
    std::memcpy(h_cams, cams, (size_t)q.n_views * sizeof(PaintCam));
    LV_HIP(hipMemcpyAsync(d_cams, h_cams, (size_t)q.n_views * sizeof(PaintCam), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_raw, h_raw, q.raw_bytes, hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetD32Async((hipDeviceptr_t)d_cell, 0x7F800000, q.total_cells, stream));
    hipLaunchKernelGGL(paint_unpack_kernel, dim3(blocks_of(q.max_pixels), q.n_views), dim3(256), 0, stream, d_raw, d_cams, d_tex);
    hipLaunchKernelGGL(paint_zbuf_kernel, dim3(blocks_of(map.n_ids)), dim3(256), 0, stream, map.d_orig, map.n_ids, d_cams, q, d_cell);
    if (q.window > 0) {
        hipLaunchKernelGGL(paint_min_x_kernel, dim3(blocks_of(q.max_cells), q.n_views), dim3(256), 0, stream, d_cell, d_tmp, d_cams, q.window);
        hipLaunchKernelGGL(paint_min_y_kernel, dim3(blocks_of(q.max_cells), q.n_views), dim3(256), 0, stream, d_tmp, d_cell, d_cams, q.window);
    }
    hipLaunchKernelGGL(paint_color_kernel, dim3(blocks_of(map.n_ids)), dim3(256), 0, stream, map.d_orig, map.n_ids, d_cams, q, d_cell, d_tex, rank,
                       want_rgb ? d_rgb.p : nullptr, want_depth ? d_depth.p : nullptr, want_seen ? d_seen.p : nullptr);
    LV_HIP(hipGetLastError());
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

void PaintStore::release() {
    h_raw.release(); h_cams.release(); d_raw.release(); d_cams.release(); d_tex.release(); d_cell.release(); d_tmp.release();
    d_rgb.release(); d_depth.release(); d_seen.release();
}

}  // namespace lv
