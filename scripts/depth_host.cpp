// scripts/depth_host.cpp — the host side of scripts/depth_timing.py: the rule of limo-velo_amd/csrc/lv_depth.hpp with the projection
// of lv_paint_dev.hpp (what the kernel of lv_depth.hip runs, shortcuts included: the views' box of voxels, and per row of voxels
// the views that cannot judge it) built with g++ -O2 through tests/emu/hip/hip_runtime.h, on binary files, timing itself: what
// fusing the frames costs on one CPU core.
//
//   depth_host PARAMS VIEWS IMAGES S W
// PARAMS: origin[3] resolution min_depth max_depth max_norm_radius (f32), then nx ny nz trunc_cells max_weight carve n_views (i32).
// VIEWS: per view R[9] t[3] fx fy cx cy dist[5] depth_scale (22 f32), then width height format (3 i32).  IMAGES: the views' rows
// back to back, packed, in view order.  S, W (read, then written): nx * ny * nz i32 each.
// stdout: one JSON object: fuse_ms and the four stats.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lv_depth.hpp"

// (what lv_paint_dev.hpp's sample needs beyond the stand-in header; the projection, the one thing taken from it here, does not)
struct float3 { float x, y, z; };
static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
#include "lv_paint_dev.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

using namespace lv;

void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

template <class T>
static std::vector<T> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

template <class T>
static void spill(const char* path, const std::vector<T>& v) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const std::vector<float> pf = slurp<float>(argv[1]);
    lv_tsdf_params tp;
    default_tsdf_params(&tp);
    for (int a = 0; a < 3; ++a) tp.origin[a] = pf[a];
    tp.resolution = pf[3];
    lv_depth_params dp{};
    dp.min_depth = pf[4]; dp.max_depth = pf[5]; dp.max_norm_radius = pf[6];
    int32_t ints[7];
    std::memcpy(ints, &pf[7], sizeof(ints));
    tp.nx = ints[0]; tp.ny = ints[1]; tp.nz = ints[2]; tp.trunc_cells = ints[3]; tp.max_weight = ints[4];
    dp.carve = ints[5];
    const int n_views = ints[6];
    const TsdfGrid g = tsdf_grid_of(tp);
    const std::vector<float> vf = slurp<float>(argv[2]);
    const std::vector<uint8_t> images = slurp<uint8_t>(argv[3]);
    if (n_views < 1 || vf.size() != (size_t)n_views * 25) return 2;
    std::vector<lv_depth_view> views((size_t)n_views);
    size_t at = 0;
    for (int w = 0; w < n_views; ++w) {
        const float* r = &vf[(size_t)w * 25];
        lv_depth_view& v = views[(size_t)w];
        v = lv_depth_view{};
        std::memcpy(v.R, r, 9 * sizeof(float));
        std::memcpy(v.t, r + 9, 3 * sizeof(float));
        v.fx = r[12]; v.fy = r[13]; v.cx = r[14]; v.cy = r[15];
        std::memcpy(v.dist, r + 16, 5 * sizeof(float));
        v.depth_scale = r[21];
        int32_t whf[3];
        std::memcpy(whf, r + 22, sizeof(whf));
        v.width = whf[0]; v.height = whf[1]; v.format = whf[2];
        v.row_stride = (size_t)v.width * depth_pixel_bytes(v.format);
        v.depth = images.data() + at;
        at += v.row_stride * (size_t)v.height;
    }
    if (at != images.size()) return 2;
    DepthRule q;
    std::vector<DepthCam> cams((size_t)DEPTH_MAX_VIEWS);
    if (depth_rule(views.data(), (size_t)n_views, &dp, &q, cams.data()) != LV_OK) return 2;
    std::vector<int32_t> S = slurp<int32_t>(argv[4]), W = slurp<int32_t>(argv[5]);
    if (S.size() != grid_cells(g.occ) || W.size() != S.size()) return 2;

    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> raw(q.raw_bytes);
    depth_stage_images(views.data(), cams.data(), n_views, raw.data());
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool any = false;
    for (int w = 0; w < n_views; ++w) {
        int l[3], h[3];
        if (!depth_view_box(g, cams[(size_t)w].cam, q.view.max_depth, q.rho, l, h)) continue;
        for (int a = 0; a < 3; ++a) {
            lo[a] = any && lo[a] < l[a] ? lo[a] : l[a];
            hi[a] = any && hi[a] > h[a] ? hi[a] : h[a];
        }
        any = true;
    }
    unsigned long long st[4] = {0, 0, 0, 0};
    const float res = g.occ.resolution;
    std::vector<int> live;
    for (int k = lo[2]; any && k < hi[2]; ++k)
        for (int j = lo[1]; j < hi[1]; ++j) {
            const float py = colour_centre(g.occ.origin[1], res, j), pz = colour_centre(g.occ.origin[2], res, k);
            const float blo[3] = {colour_centre(g.occ.origin[0], res, lo[0]), py, pz}, bhi[3] = {colour_centre(g.occ.origin[0], res, hi[0] - 1), py, pz};
            live.clear();
            for (int w = 0; w < n_views; ++w)
                if (!depth_box_unseen(cams[(size_t)w].cam, q.view.min_depth, q.view.max_depth, q.rho, blo, bhi)) live.push_back(w);
            if (live.empty()) continue;
            for (int i = lo[0]; i < hi[0]; ++i) {
                const float4 p = make_float4(colour_centre(g.occ.origin[0], res, i), py, pz, 0.f);
                int32_t dS = 0, dW = 0;
                for (int w : live) {
                    const DepthCam& c = cams[(size_t)w];
                    float z, u, v;
                    if (!paint_project(c.cam, q.view, p, z, u, v)) continue;
                    ++st[0];
                    int px = (int)floorf(u + 0.5f), pyx = (int)floorf(v + 0.5f);
                    px = px < 0 ? 0 : (px > c.cam.width - 1 ? c.cam.width - 1 : px);
                    pyx = pyx < 0 ? 0 : (pyx > c.cam.height - 1 ? c.cam.height - 1 : pyx);
                    const size_t pix = (size_t)pyx * (size_t)c.cam.width + (size_t)px;
                    const uint8_t* img = raw.data() + c.cam.raw_off;
                    float D;
                    bool ok;
                    if (c.cam.format == LV_DEPTH_U16) {
                        uint16_t r16;
                        std::memcpy(&r16, img + 2 * pix, 2);
                        ok = depth_of_u16(r16, c.scale, q.view.min_depth, q.view.max_depth, D);
                    } else {
                        float r32;
                        std::memcpy(&r32, img + 4 * pix, 4);
                        ok = depth_of_f32(r32, q.view.min_depth, q.view.max_depth, D);
                    }
                    if (!ok) continue;
                    ++st[1];
                    int32_t s;
                    if (!depth_quant(D, z, res, g.T, q.carve, s)) continue;
                    dS += s;
                    ++dW;
                }
                if (dW > 0) {
                    const size_t vox = grid_at(g.occ, i, j, k);
                    tsdf_fold(g.max_weight, dS, dW, S[vox], W[vox]);
                    st[2] += (unsigned long long)dW;
                    ++st[3];
                }
            }
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    spill(argv[4], S);
    spill(argv[5], W);
    printf("{\"fuse_ms\": %.3f, \"stats\": [%llu, %llu, %llu, %llu], \"box\": [%d, %d, %d, %d, %d, %d]}\n", ms, st[0], st[1], st[2], st[3], lo[0], lo[1], lo[2],
           hi[0], hi[1], hi[2]);
    return 0;
}
