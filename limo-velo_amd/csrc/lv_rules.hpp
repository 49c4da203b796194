// lv_rules.hpp — the argument rules of the tools on the point map: limits, defaults, what a call is refused for (LV_EINVAL and the
// message; the first refusal wins, nothing is touched) and the resolved rule the kernels take.  Pure host arithmetic on
// include/limovelo_hip.h, no HIP header: plain g++ compiles it (tests/test_rules_host.py).  lv_api.hip judges the context first.
// (The tools on the volumes keep their argument rules in their own headers, lv_occupancy.hpp .. lv_tsdf.hpp, and what they ask
// of the context's state, with what makes what stale, in lv_volumes.hpp; of this header they share views_ok.)
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/limovelo_hip.h"

namespace lv {

void set_error(const char* fmt, ...);

// Every view of lv_map_remove_dynamic, lv_occ_integrate and lv_occ_view_gain; max_returns bounds one view's returns and their sum.
// judge_t: only lv_map_remove_dynamic refuses a non-finite t, to the occupancy walks it is a view without evidence (OCC_T_LIMIT).
inline int views_ok(const lv_view* views, size_t n_views, const char* prefix, bool judge_t, size_t max_returns) {
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const lv_view& w = views[v];
        for (int i = 0; i < 9; ++i) if (!std::isfinite(w.R[i])) { set_error("%sview %zu: non-finite R", prefix, v); return LV_EINVAL; }
        for (int i = 0; judge_t && i < 3; ++i) if (!std::isfinite(w.t[i])) { set_error("%sview %zu: non-finite t", prefix, v); return LV_EINVAL; }
        if (w.n && (!w.points || w.stride < 12)) { set_error("%sview %zu: bad point array (stride %zu)", prefix, v, w.stride); return LV_EINVAL; }
        total += w.n;
        if (w.n > max_returns || total > max_returns) { set_error("%stoo many returns", prefix); return LV_EINVAL; }
    }
    return LV_OK;
}

// ---- Dynamic-point removal (lv_visibility.hip)
constexpr int VIS_MAX_VIEWS = 32;
constexpr size_t VIS_MAX_PIXELS = (size_t)1 << 20;   // width * height of one view's image
constexpr int VIS_MAX_WINDOW = 8;

// The rule of one call, as the kernels take it (angles in radians, the bin scales precomputed on the host)
struct VisRule {
    int width, height, n_views, window, min_hits;
    float inv_col;      // width / (2 pi): columns per radian of azimuth
    float v_min;        // lowest elevation (rad)
    float inv_row;      // height / (v_max - v_min): rows per radian of elevation
    float min_range, max_range, margin_abs, margin_rel;
};

inline void default_visibility_params(lv_visibility_params* p) {
    if (!p) return;
    p->width = 2048;
    p->height = 64;
    p->v_min_deg = -25.f;
    p->v_max_deg = 3.f;
    p->min_range = 1.f;
    p->max_range = 80.f;
    p->margin_abs = 0.3f;
    p->margin_rel = 0.02f;
    p->window = 1;
    p->min_hits = 1;
    p->dry_run = 0;
}

// The views and parameters of lv_map_remove_dynamic against its limits: LV_EINVAL (nothing touched) outside them
inline int visibility_rule(const lv_view* views, size_t n_views, const lv_visibility_params* p, VisRule* q) {
    if (!views || !p) { set_error("null argument"); return LV_EINVAL; }
    if (n_views < 1 || n_views > (size_t)VIS_MAX_VIEWS) { set_error("n_views = %zu: must be in 1..%d", n_views, VIS_MAX_VIEWS); return LV_EINVAL; }
    if (p->width < 1 || p->height < 1 || (size_t)p->width * (size_t)p->height > VIS_MAX_PIXELS) {
        set_error("image of %d x %d pixels: both >= 1, at most 2^20 in all", p->width, p->height);
        return LV_EINVAL;
    }
    if (!(std::isfinite(p->v_min_deg) && std::isfinite(p->v_max_deg) && p->v_min_deg < p->v_max_deg && p->v_min_deg >= -90.f && p->v_max_deg <= 90.f)) {
        set_error("vertical field of view [%g, %g] deg: v_min_deg < v_max_deg inside [-90, 90]", p->v_min_deg, p->v_max_deg);
        return LV_EINVAL;
    }
    if (!(std::isfinite(p->min_range) && std::isfinite(p->max_range) && p->min_range > 0.f && p->min_range < p->max_range)) {
        set_error("ranges [%g, %g]: finite, 0 < min_range < max_range", p->min_range, p->max_range);
        return LV_EINVAL;
    }
    if (!(std::isfinite(p->margin_abs) && std::isfinite(p->margin_rel) && p->margin_abs > 0.f && p->margin_rel > 0.f)) {
        set_error("margins %g m, %g: finite and > 0", p->margin_abs, p->margin_rel);
        return LV_EINVAL;
    }
    if (p->window < 0 || p->window > VIS_MAX_WINDOW) { set_error("window = %d: must be in 0..%d", p->window, VIS_MAX_WINDOW); return LV_EINVAL; }
    if (p->min_hits < 1 || (size_t)p->min_hits > n_views) { set_error("min_hits = %d: must be in 1..n_views", p->min_hits); return LV_EINVAL; }
    if (int rc = views_ok(views, n_views, "", true, 0xFFFFFFF0ull)) return rc;
    const double rad = 3.14159265358979323846 / 180.0;
    q->width = p->width;
    q->height = p->height;
    q->n_views = (int)n_views;
    q->window = p->window;
    q->min_hits = p->min_hits;
    q->inv_col = (float)((double)p->width / (2.0 * 3.14159265358979323846));
    q->v_min = (float)((double)p->v_min_deg * rad);
    q->inv_row = (float)((double)p->height / (((double)p->v_max_deg - (double)p->v_min_deg) * rad));
    q->min_range = p->min_range;
    q->max_range = p->max_range;
    q->margin_abs = p->margin_abs;
    q->margin_rel = p->margin_rel;
    return LV_OK;
}

// ---- Surface normals and outlier removal (lv_surface.hip)
constexpr int SURF_MAX_K = 32;

struct SurfRule {
    int job;               // 0: normals (covariance + mean distance), 1: statistical outliers (mean distance), 2: radius outliers (count)
    int k;                 // jobs 0, 1: neighbours searched, the point itself included (job 1: the caller's k + 1); job 2: unused, 0
    int min_neighbours;
    int orient;
    float max_dist;        // jobs 0, 1; job 2: the radius
    float std_mul;         // job 1
    double viewpoint[3];
    double threshold;      // jobs 1, 2: what a point's value is judged against
    int fixed_threshold;   // job 1: threshold is given (a replay), not computed from the store's own statistics
};

inline void default_surface_params(lv_surface_params* p) {
    if (!p) return;
    p->k = 10;
    p->max_dist = 2.f;
    p->min_neighbours = 5;
    p->orient = 0;
    p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0;
}

inline void default_outlier_params(lv_outlier_params* p) {
    if (!p) return;
    p->mode = 0;
    p->k = 10;
    p->max_dist = 2.f;
    p->std_mul = 2.f;
    p->radius = 0.5f;
    p->min_neighbours = 5;
    p->dry_run = 0;
}

// The parameters of lv_map_normals against their limits; *q zeroed by the caller
inline int surface_rule(const lv_surface_params* p, SurfRule* q) {
    if (!p) { set_error("null argument"); return LV_EINVAL; }
    if (p->k < 2 || p->k > SURF_MAX_K) { set_error("k = %d: must be in 2..%d", p->k, SURF_MAX_K); return LV_EINVAL; }
    if (!(std::isfinite(p->max_dist) && p->max_dist > 0.f)) { set_error("max_dist = %g: finite and > 0", p->max_dist); return LV_EINVAL; }
    if (p->min_neighbours < 3 || p->min_neighbours > p->k) { set_error("min_neighbours = %d: must be in 3..k", p->min_neighbours); return LV_EINVAL; }
    if (p->orient != 0 && p->orient != 1) { set_error("orient = %d: 0 or 1", p->orient); return LV_EINVAL; }
    for (int a = 0; a < 3; ++a) if (!std::isfinite(p->viewpoint[a])) { set_error("non-finite viewpoint"); return LV_EINVAL; }
    q->job = 0;
    q->k = p->k;
    q->min_neighbours = p->min_neighbours;
    q->orient = p->orient;
    q->max_dist = p->max_dist;
    for (int a = 0; a < 3; ++a) q->viewpoint[a] = p->viewpoint[a];
    return LV_OK;
}

// The parameters of lv_map_remove_outliers against their limits, by mode; *q zeroed by the caller
inline int outlier_rule(const lv_outlier_params* p, SurfRule* q) {
    if (!p) { set_error("null argument"); return LV_EINVAL; }
    if (p->mode == 0) {
        if (p->k < 1 || p->k > SURF_MAX_K - 1) { set_error("k = %d: must be in 1..%d", p->k, SURF_MAX_K - 1); return LV_EINVAL; }
        if (!(std::isfinite(p->max_dist) && p->max_dist > 0.f)) { set_error("max_dist = %g: finite and > 0", p->max_dist); return LV_EINVAL; }
        if (!std::isfinite(p->std_mul)) { set_error("std_mul must be finite"); return LV_EINVAL; }
        q->job = 1;
        q->k = p->k + 1;
        q->max_dist = p->max_dist;
        q->std_mul = p->std_mul;
    } else if (p->mode == 1) {
        if (!(std::isfinite(p->radius) && p->radius > 0.f)) { set_error("radius = %g: finite and > 0", p->radius); return LV_EINVAL; }
        if (p->min_neighbours < 1) { set_error("min_neighbours = %d: must be >= 1", p->min_neighbours); return LV_EINVAL; }
        q->job = 2;
        q->max_dist = p->radius;
        q->min_neighbours = p->min_neighbours;
        q->threshold = (double)p->min_neighbours;
        q->fixed_threshold = 1;
    } else {
        set_error("mode = %d: 0 (statistical) or 1 (radius)", p->mode);
        return LV_EINVAL;
    }
    return LV_OK;
}

// ---- Map clustering (lv_cluster.hip)
struct ClusterRule {
    float radius;
    uint32_t min_size, max_size;
    int seeded;   // lv_map_remove_clusters: 1 with seeds (object growth), 0 without (debris)
};

inline void default_cluster_params(lv_cluster_params* p) {
    if (!p) return;
    p->radius = 0.5f;
    p->min_size = 1;
    p->max_size = 0;
    p->dry_run = 0;
}

// The parameters of lv_map_cluster / lv_map_remove_clusters against their limits: LV_EINVAL (nothing touched) outside them
inline int cluster_rule(const lv_cluster_params* p, ClusterRule* q) {
    if (!p) { set_error("null argument"); return LV_EINVAL; }
    if (!(std::isfinite(p->radius) && p->radius > 0.f)) { set_error("radius = %g: finite and > 0", p->radius); return LV_EINVAL; }
    if (p->min_size < 1) { set_error("min_size = 0: must be >= 1"); return LV_EINVAL; }
    q->radius = p->radius;
    q->min_size = p->min_size;
    q->max_size = p->max_size;
    q->seeded = 0;
    return LV_OK;
}

// ---- Map painting (lv_paint.hip)
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

// What paint_project reads of a view, from its pose and intrinsics (dist: k1, k2, p1, p2, k3); every other field zero
inline PaintCam paint_cam_of(const float R[9], const float t[3], float fx, float fy, float cx, float cy, const float dist[5], int width, int height) {
    PaintCam c;
    std::memset(&c, 0, sizeof(c));
    std::memcpy(c.R, R, sizeof(c.R));
    std::memcpy(c.t, t, sizeof(c.t));
    c.fx = fx;
    c.fy = fy;
    c.cx = cx;
    c.cy = cy;
    c.k1 = dist[0];
    c.k2 = dist[1];
    c.p1 = dist[2];
    c.p2 = dist[3];
    c.k3 = dist[4];
    c.wm1 = (float)(width - 1);
    c.hm1 = (float)(height - 1);
    c.width = width;
    c.height = height;
    return c;
}

// The call's parameters (r2_max = max_norm_radius^2 in f32, s = zbuf_scale as f32)
struct PaintRule {
    int n_views, window, blend;
    float min_depth, max_depth, r2_max, s, margin_abs, margin_rel;
    uint32_t max_pixels, max_cells;   // the largest view's pixels / cells (the grids of the per-view kernels)
    size_t total_pixels, total_cells, raw_bytes;
};

inline void default_paint_params(lv_paint_params* p) {
    if (!p) return;
    p->min_depth = 0.3f;
    p->max_depth = 60.f;
    p->max_norm_radius = 1.5f;
    p->zbuf_scale = 4;
    p->window = 1;
    p->margin_abs = 0.1f;
    p->margin_rel = 0.01f;
    p->blend = 0;
}

// The views and parameters of lv_map_paint against its limits: LV_EINVAL (nothing written) outside them; inside, the rule as the
// kernels take it and every view's place in the call's buffers
inline int paint_rule(const lv_camera_view* views, size_t n_views, const lv_paint_params* p, PaintRule* q, PaintCam* cams) {
    if (!views || !p) { set_error("null argument"); return LV_EINVAL; }
    if (n_views < 1 || n_views > (size_t)PAINT_MAX_VIEWS) { set_error("n_views = %zu: must be in 1..%d", n_views, PAINT_MAX_VIEWS); return LV_EINVAL; }
    if (!(std::isfinite(p->min_depth) && std::isfinite(p->max_depth) && p->min_depth > 0.f && p->min_depth < p->max_depth)) {
        set_error("depths [%g, %g]: finite, 0 < min_depth < max_depth", p->min_depth, p->max_depth);
        return LV_EINVAL;
    }
    if (!(std::isfinite(p->max_norm_radius) && p->max_norm_radius > 0.f)) { set_error("max_norm_radius = %g: finite and > 0", p->max_norm_radius); return LV_EINVAL; }
    if (p->zbuf_scale < 1 || p->zbuf_scale > PAINT_MAX_SCALE) { set_error("zbuf_scale = %d: must be in 1..%d", p->zbuf_scale, PAINT_MAX_SCALE); return LV_EINVAL; }
    if (p->window < 0 || p->window > PAINT_MAX_WINDOW) { set_error("window = %d: must be in 0..%d", p->window, PAINT_MAX_WINDOW); return LV_EINVAL; }
    if (!(std::isfinite(p->margin_abs) && std::isfinite(p->margin_rel) && p->margin_abs > 0.f && p->margin_rel > 0.f)) {
        set_error("margins %g m, %g: finite and > 0", p->margin_abs, p->margin_rel);
        return LV_EINVAL;
    }
    if (p->blend != 0 && p->blend != 1) { set_error("blend = %d: must be 0 or 1", p->blend); return LV_EINVAL; }
    const int s = p->zbuf_scale;
    size_t pixels = 0, cells = 0, raw = 0;
    uint32_t max_pixels = 0, max_cells = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const lv_camera_view& w = views[v];
        for (int i = 0; i < 9; ++i) if (!std::isfinite(w.R[i])) { set_error("view %zu: non-finite R", v); return LV_EINVAL; }
        for (int i = 0; i < 3; ++i) if (!std::isfinite(w.t[i])) { set_error("view %zu: non-finite t", v); return LV_EINVAL; }
        if (!(std::isfinite(w.fx) && std::isfinite(w.fy) && std::isfinite(w.cx) && std::isfinite(w.cy))) { set_error("view %zu: non-finite intrinsics", v); return LV_EINVAL; }
        for (int i = 0; i < 5; ++i) if (!std::isfinite(w.dist[i])) { set_error("view %zu: non-finite distortion", v); return LV_EINVAL; }
        if (w.width < 1 || w.height < 1 || w.width > PAINT_MAX_SIDE || w.height > PAINT_MAX_SIDE || (size_t)w.width * (size_t)w.height > PAINT_MAX_PIXELS) {
            set_error("view %zu: image of %d x %d pixels: each side 1..%d, at most 2^24 in all", v, w.width, w.height, PAINT_MAX_SIDE);
            return LV_EINVAL;
        }
        if (w.format != LV_IMAGE_RGB8 && w.format != LV_IMAGE_BGR8 && w.format != LV_IMAGE_MONO8) { set_error("view %zu: format %d", v, w.format); return LV_EINVAL; }
        const size_t row = (size_t)w.width * (w.format == LV_IMAGE_MONO8 ? 1 : 3);
        if (!w.image || w.row_stride < row) { set_error("view %zu: null image or row_stride %zu < %zu", v, w.row_stride, row); return LV_EINVAL; }
        const size_t np = (size_t)w.width * (size_t)w.height;
        const int cw = (w.width + s - 1) / s, ch = (w.height + s - 1) / s;
        PaintCam& c = cams[v];
        c = paint_cam_of(w.R, w.t, w.fx, w.fy, w.cx, w.cy, w.dist, w.width, w.height);
        c.cw = cw;
        c.ch = ch;
        c.format = w.format;
        c.tex_off = (uint32_t)pixels;
        c.cell_off = (uint32_t)cells;
        c.raw_off = (uint32_t)raw;
        pixels += np;
        cells += (size_t)cw * (size_t)ch;
        raw += (row * (size_t)w.height + 255) & ~(size_t)255;
        if (pixels > PAINT_MAX_TOTAL_PIXELS) { set_error("the views hold more than 2^26 pixels together"); return LV_EINVAL; }
        if (np > max_pixels) max_pixels = (uint32_t)np;
        if ((uint32_t)(cw * ch) > max_cells) max_cells = (uint32_t)(cw * ch);
    }
    q->n_views = (int)n_views;
    q->window = p->window;
    q->blend = p->blend;
    q->min_depth = p->min_depth;
    q->max_depth = p->max_depth;
    q->r2_max = p->max_norm_radius * p->max_norm_radius;
    q->s = (float)s;
    q->margin_abs = p->margin_abs;
    q->margin_rel = p->margin_rel;
    q->max_pixels = max_pixels;
    q->max_cells = max_cells;
    q->total_pixels = pixels;
    q->total_cells = cells;
    q->raw_bytes = raw;
    return LV_OK;
}

// ---- Depth fusion (lv_depth.hip; its argument rule, depth_rule, is lv_depth.hpp's)
// One depth view as the kernel takes it (144 B): cam.format is LV_DEPTH_*, cam.raw_off the first staged byte of the view (rows of
// width * 2 or width * 4 bytes, back to back; a multiple of 256); cam.tex_off, cell_off, cw and ch are not used.
struct DepthCam {
    PaintCam cam;
    float scale;               // depth_scale (U16)
    uint32_t pad[3];
};
static_assert(sizeof(DepthCam) == 144, "DepthCam is 144 B");

// The call's parameters: view holds what paint_project reads (n_views, min_depth, max_depth, r2_max), the rest of it is zero;
// rho = max_norm_radius
struct DepthRule {
    PaintRule view;
    float rho;
    int carve;
    size_t raw_bytes;
};

// ---- Place recognition (lv_place.hip)
constexpr int PLACE_MAX_RINGS = 32;
constexpr int PLACE_MAX_SECTORS = 64;                       // one lane per shift in the scoring wavefront
constexpr int PLACE_MAX_BINS = PLACE_MAX_RINGS * PLACE_MAX_SECTORS;
constexpr size_t PLACE_MAX_COUNT = (size_t)1 << 20;         // ids fit the 20 bits of the retrieval key
constexpr size_t PLACE_MAX_MAP_CENTRES = 65536;             // per lv_place_add_map call
constexpr int PLACE_MAX_K = 64;

inline void default_place_params(lv_place_params* p) {
    if (!p) return;
    p->n_rings = 20;
    p->n_sectors = 60;
    p->rmin = 0.f;
    p->rmax = 80.f;
    p->z_offset = 2.f;
}

inline int place_params_ok(const lv_place_params* p) {
    if (!p) { set_error("null argument"); return LV_EINVAL; }
    if (p->n_rings < 1 || p->n_rings > PLACE_MAX_RINGS) { set_error("n_rings = %d: must be in 1..%d", p->n_rings, PLACE_MAX_RINGS); return LV_EINVAL; }
    if (p->n_sectors < 2 || p->n_sectors > PLACE_MAX_SECTORS) { set_error("n_sectors = %d: must be in 2..%d", p->n_sectors, PLACE_MAX_SECTORS); return LV_EINVAL; }
    if (!(std::isfinite(p->rmin) && std::isfinite(p->rmax) && p->rmin >= 0.f && p->rmin < p->rmax && p->rmax <= 1000.f)) {
        set_error("rmin %g, rmax %g: finite, 0 <= rmin < rmax <= 1000", p->rmin, p->rmax);
        return LV_EINVAL;
    }
    if (!std::isfinite(p->z_offset)) { set_error("z_offset = %g: must be finite", p->z_offset); return LV_EINVAL; }
    return LV_OK;
}

inline int place_state_ok(const lv_state* x) {
    if (!x) { set_error("null state"); return LV_EINVAL; }
    const double* v = reinterpret_cast<const double*>(x);
    for (size_t i = 0; i < sizeof(lv_state) / sizeof(double); ++i)
        if (!std::isfinite(v[i])) { set_error("non-finite state"); return LV_EINVAL; }
    return LV_OK;
}

// the n centres (3 doubles each) of lv_place_add_map / lv_place_load
inline int place_centres_ok(const double* centres, size_t n) {
    for (size_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(centres[i])) { set_error("centre %zu is not finite", i / 3); return LV_EINVAL; }
    return LV_OK;
}

}  // namespace lv
