// lv_tsdf.hpp — TSDF fusion of LiDAR sweeps and the surface mesh taken from it (lv_tsdf_*, include/limovelo_hip.h "TSDF and mesh";
// kernels and host side in lv_tsdf.hip).
//
// The first part is the rule itself as plain __host__ __device__ code without atomics: the ray (its exact length, the extension
// behind the surface, where the walk starts), the signed distance of a cell, the packed scratch word, the fold, and the mesh
// (active cells, crossings, vertices, faces).  The returns, their quantisation and the walk are lv_occupancy.hpp's, run on an
// OccGrid filled from the TSDF's own grid.  The kernels of lv_tsdf.hip run exactly these functions; tests/emu/tsdf_emu.cpp
// compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_tsdf_host.py holds them to tests/tsdf_ref.py.  After
// occ_quant every step is integer arithmetic, so the three agree on every voxel, vertex and index.
#pragma once

#include "lv_align.hpp"   // AlignStage: the scratch of lv_surf_align
#include "lv_occupancy.hpp"
#include "lv_rules.hpp"   // PaintCam, PaintRule: what the colour layer's integrate takes

namespace lv {

constexpr int TSDF_MAX_TRUNC = 16;
constexpr int TSDF_MAX_WEIGHT = 1 << 18;
constexpr size_t TSDF_MAX_RETURNS = (size_t)1 << 24;   // of one lv_tsdf_integrate, over its views

// The grid and the constants of one call as the kernels take them
struct TsdfGrid {
    OccGrid occ;      // origin, resolution, dimensions and ranges: what occ_view_origin / occ_return / the walk read
    int32_t T;        // trunc_cells * 256
    int32_t max_weight;
    int32_t carve;
};

LV_OCC_HD int64_t tsdf_floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return q - ((a % b) < 0 ? 1 : 0);
}

// floor(sqrt(l2)) exactly, l2 < 2^52: the f64 root, then corrected by integer comparison
LV_OCC_HD int64_t tsdf_isqrt(int64_t l2) {
    int64_t r = (int64_t)sqrt((double)l2);
    while (r * r > l2) --r;
    while ((r + 1) * (r + 1) <= l2) ++r;
    return r;
}

// One ray as its walk needs it.  Named scalars, no indexed arrays: the state lives in registers on the device.
struct TsdfRay {
    int32_t start[3], qb[3];   // the walk runs start -> qb (filled and read with constant indices only)
    int32_t ex, ey, ez;        // the original end point qe ...
    int32_t dx, dy, dz;        // ... and d = qe - qs: what s is measured against
    int64_t len;
    bool cut;                  // a carved CUT return: every cell takes s = T
};

// ext_a = (d_a * T) / len by truncating division; |ext_a| <= T
LV_OCC_HD int32_t tsdf_ext(int32_t d, int32_t T, int64_t len) { return (int32_t)(((int64_t)d * (int64_t)T) / len); }

// false: the ray gives nothing and is not counted (len == 0, or a CUT return without carve).  kind: OCC_RAY_HIT or OCC_RAY_CUT.
LV_OCC_HD bool tsdf_ray_init(const TsdfGrid& g, const int32_t qs[3], const int32_t qe[3], int kind, TsdfRay& r) {
    if (kind == OCC_RAY_CUT && !g.carve) return false;
    r.ex = qe[0]; r.ey = qe[1]; r.ez = qe[2];
    r.dx = qe[0] - qs[0]; r.dy = qe[1] - qs[1]; r.dz = qe[2] - qs[2];
    r.len = tsdf_isqrt((int64_t)r.dx * (int64_t)r.dx + (int64_t)r.dy * (int64_t)r.dy + (int64_t)r.dz * (int64_t)r.dz);
    if (r.len == 0) return false;
    r.cut = kind == OCC_RAY_CUT;
    r.start[0] = qs[0]; r.start[1] = qs[1]; r.start[2] = qs[2];
    r.qb[0] = qe[0]; r.qb[1] = qe[1]; r.qb[2] = qe[2];
    if (r.cut) return true;
    const int32_t ax = tsdf_ext(r.dx, g.T, r.len), ay = tsdf_ext(r.dy, g.T, r.len), az = tsdf_ext(r.dz, g.T, r.len);
    r.qb[0] += ax; r.qb[1] += ay; r.qb[2] += az;
    if (!(g.carve || r.len <= (int64_t)g.T)) { r.start[0] = qe[0] - ax; r.start[1] = qe[1] - ay; r.start[2] = qe[2] - az; }
    return true;
}

// The contribution of the ray to the cell (vx, vy, vz) it stands in; false: none (s < -T).  The division happens only inside
// the truncation band: num >= (T + 1) * len is s > T, num < -T * len is s < -T.
LV_OCC_HD bool tsdf_cell_s(const TsdfGrid& g, const TsdfRay& r, int32_t vx, int32_t vy, int32_t vz, int32_t& s) {
    if (r.cut) { s = g.T; return true; }
    const int64_t num = (int64_t)(r.ex - (256 * vx + 128)) * (int64_t)r.dx + (int64_t)(r.ey - (256 * vy + 128)) * (int64_t)r.dy +
                        (int64_t)(r.ez - (256 * vz + 128)) * (int64_t)r.dz;
    if (num >= (int64_t)(g.T + 1) * r.len) { s = g.T; return true; }
    if (num < -(int64_t)g.T * r.len) return false;
    s = (int32_t)tsdf_floor_div(num, r.len);
    return true;
}

// The scratch word of a voxel: dW above a signed 39-bit dS.  |dS| <= 4096 * 2^24 = 2^36 and dW <= 2^24 < 2^25, so neither
// field overflows whatever a call brings; the words add as plain 64-bit integers (a negative dS borrows from dW and unpack
// gives it back), and a word is zero iff nothing was added.
constexpr int TSDF_PACK_SHIFT = 39;
LV_OCC_HD unsigned long long tsdf_pack(int32_t s) { return ((unsigned long long)1 << TSDF_PACK_SHIFT) + (unsigned long long)(long long)s; }
LV_OCC_HD void tsdf_unpack(unsigned long long w, int64_t& dS, int64_t& dW) {
    dS = (int64_t)(w << (64 - TSDF_PACK_SHIFT)) >> (64 - TSDF_PACK_SHIFT);
    dW = (int64_t)((w - (unsigned long long)dS) >> TSDF_PACK_SHIFT);
}

// The fold of one voxel with dW > 0
LV_OCC_HD void tsdf_fold(int32_t max_weight, int64_t dS, int64_t dW, int32_t& S, int32_t& W) {
    const int64_t Wn = (int64_t)W + dW, Sn = (int64_t)S + dS;
    if (Wn > (int64_t)max_weight) {
        S = (int32_t)tsdf_floor_div(Sn * (int64_t)max_weight, Wn);
        W = max_weight;
    } else {
        S = (int32_t)Sn;
        W = (int32_t)Wn;
    }
}

// f32, unfused; NaN where W = 0 (0 / 0)
LV_OCC_HD float tsdf_metres(float resolution, int32_t S, int32_t W) { return resolution * (((float)S / (float)W) / 256.0f); }

// ---- the mesh: naive surface nets.  S, W: the volume by grid_at; G: any struct with nx, ny, nz.
// the 8 corners of a cell
struct TsdfCorners {
    int32_t S[8], W[8];   // corner (dx, dy, dz) at dx + 2 * dy + 4 * dz
};

// The corners of cell (i, j, k); false: the cell does not exist, a corner is not known, or all are of one sign
template <class G>
LV_OCC_HD bool tsdf_cell_active(const G& g, const int32_t* S, const int32_t* W, int32_t min_weight, int i, int j, int k, TsdfCorners& c) {
    if (i < 0 || j < 0 || k < 0 || i > g.nx - 2 || j > g.ny - 2 || k > g.nz - 2) return false;
    int inside = 0;
    for (int n = 0; n < 8; ++n) {
        const size_t at = grid_at(g, i + (n & 1), j + ((n >> 1) & 1), k + (n >> 2));
        c.W[n] = W[at];
        if (c.W[n] < min_weight) return false;
        c.S[n] = S[at];
        inside += c.S[n] < 0;
    }
    return inside != 0 && inside != 8;
}

// where the surface crosses the edge A -> B (signs differ): 0..256 sub-units from A
LV_OCC_HD int32_t tsdf_crossing(int32_t SA, int32_t WA, int32_t SB, int32_t WB) {
    int64_t num = (int64_t)SA * (int64_t)WB;
    int64_t den = num - (int64_t)SB * (int64_t)WA;
    if (den < 0) { num = -num; den = -den; }
    return (int32_t)((256 * num) / den);
}

// The vertex of the active cell (i, j, k) in sub-units: per axis the mean of its crossings' coordinates
LV_OCC_HD void tsdf_vertex(const TsdfCorners& c, int i, int j, int k, int32_t v[3]) {
    const int32_t base[3] = {256 * i + 128, 256 * j + 128, 256 * k + 128};
    int64_t sum[3] = {0, 0, 0};
    int count = 0;
    for (int a = 0; a < 3; ++a) {
        const int step = 1 << a;
        for (int n = 0; n < 8; ++n) {
            if (n & step) continue;   // the edge runs from corner n to n + step along axis a
            const int m = n + step;
            if ((c.S[n] < 0) == (c.S[m] < 0)) continue;
            const int32_t t = tsdf_crossing(c.S[n], c.W[n], c.S[m], c.W[m]);
            for (int b = 0; b < 3; ++b) sum[b] += base[b] + 256 * ((n >> b) & 1) + (b == a ? t : 0);
            ++count;
        }
    }
    for (int b = 0; b < 3; ++b) v[b] = (int32_t)(sum[b] / count);
}

// f32, unfused
LV_OCC_HD float tsdf_vertex_metres(float origin, float resolution, int32_t v) { return origin + resolution * ((float)v / 256.0f); }

// The grid edge from voxel p = (i, j, k) along axis a.  0: no face (an end outside the grid or not known, or no sign change);
// 1: a quad, cells[4] the linear indices of q0..q3 already in the emitted order; 2: refused, a cell is missing or not active.
// `active` answers whether a cell (by its linear index) is active.
template <class G, class Active>
LV_OCC_HD int tsdf_edge_face(const G& g, const int32_t* S, const int32_t* W, int32_t min_weight, int i, int j, int k, int a, Active active,
                             uint32_t cells[4]) {
    const int p[3] = {i, j, k};
    const int n[3] = {g.nx, g.ny, g.nz};
    if (p[a] + 1 >= n[a]) return 0;
    int e[3] = {i, j, k};
    e[a] += 1;
    const size_t pa = grid_at(g, i, j, k), pb = grid_at(g, e[0], e[1], e[2]);
    if (W[pa] < min_weight || W[pb] < min_weight) return 0;
    const bool inside = S[pa] < 0;
    if (inside == (S[pb] < 0)) return 0;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const int ob[4] = {-1, 0, 0, -1}, oc[4] = {-1, -1, 0, 0};
    uint32_t q[4];
    for (int m = 0; m < 4; ++m) {
        int v[3] = {i, j, k};
        v[b] += ob[m];
        v[c] += oc[m];
        if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[0] > g.nx - 2 || v[1] > g.ny - 2 || v[2] > g.nz - 2) return 2;
        q[m] = (uint32_t)grid_at(g, v[0], v[1], v[2]);
        if (!active(q[m])) return 2;
    }
    cells[0] = q[0];
    cells[1] = inside ? q[1] : q[3];
    cells[2] = q[2];
    cells[3] = inside ? q[3] : q[1];
    return 1;
}

inline void default_tsdf_params(lv_tsdf_params* p) {
    if (!p) return;
    lv_occupancy_params o;
    default_occupancy_params(&o);   // (the occupancy grid's footprint)
    *p = lv_tsdf_params{};
    for (int a = 0; a < 3; ++a) p->origin[a] = o.origin[a];
    p->resolution = o.resolution;
    p->nx = o.nx;
    p->ny = o.ny;
    p->nz = o.nz;
    p->min_range = o.min_range;
    p->max_range = o.max_range;
    p->trunc_cells = 3;
    p->max_weight = 10000;
    p->carve = 0;
}

// The parameters against their limits: NULL when they hold, otherwise what is wrong (lv_tsdf_configure: LV_EINVAL)
inline const char* tsdf_check_params(const lv_tsdf_params* p) {
    if (!p) return "null params";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(p->origin[a])) return "origin: must be finite";
    if (!(std::isfinite(p->resolution) && p->resolution > 0.f)) return "resolution: must be finite and > 0";
    if (p->nx < 1 || p->nx > OCC_MAX_DIM || p->ny < 1 || p->ny > OCC_MAX_DIM || p->nz < 1 || p->nz > OCC_MAX_DIM)
        return "nx, ny, nz: each must be in 1..1024";
    if ((uint64_t)p->nx * (uint64_t)p->ny * (uint64_t)p->nz > OCC_MAX_VOXELS) return "nx * ny * nz: at most 2^28 voxels";
    if (!(std::isfinite(p->min_range) && std::isfinite(p->max_range) && p->min_range > 0.f && p->min_range < p->max_range))
        return "ranges: finite, 0 < min_range < max_range";
    if (!(p->max_range / p->resolution <= OCC_RANGE_LIMIT)) return "max_range / resolution: at most 4096";
    if (p->trunc_cells < 1 || p->trunc_cells > TSDF_MAX_TRUNC) return "trunc_cells: must be in 1..16";
    if (p->max_weight < 1 || p->max_weight > TSDF_MAX_WEIGHT) return "max_weight: must be in 1..2^18";
    if (p->carve != 0 && p->carve != 1) return "carve: 0 or 1";
    return nullptr;
}

inline TsdfGrid tsdf_grid_of(const lv_tsdf_params& p) {
    TsdfGrid g{};
    for (int a = 0; a < 3; ++a) g.occ.origin[a] = p.origin[a];
    g.occ.resolution = p.resolution;
    g.occ.nx = p.nx; g.occ.ny = p.ny; g.occ.nz = p.nz;
    g.occ.wx = (p.nx + 31) / 32;
    g.occ.min_range2 = p.min_range * p.min_range;
    g.occ.max_range2 = p.max_range * p.max_range;
    g.occ.max_range = p.max_range;
    g.T = p.trunc_cells * 256;
    g.max_weight = p.max_weight;
    g.carve = p.carve;
    return g;
}

// The first voxel lv_tsdf_load refuses (W < 0, W > max_weight, |S| > T * W), or n when every voxel holds
inline size_t tsdf_check_volume(const TsdfGrid& g, const int32_t* S, const int32_t* W, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const int64_t w = W[i], s = S[i];
        if (w < 0 || w > g.max_weight || (s < 0 ? -s : s) > (int64_t)g.T * w) return i;
    }
    return n;
}

// The mesh of the volume at its last build: a snapshot, as the distance field is
struct TsdfMesh {
    bool built = false;
    int stale = 0;
    int min_weight = 0;
    uint64_t counts[4] = {0, 0, 0, 0};   // vertices, triangles, active cells, edges refused
    DevBuf<float> d_xyz;                 // 3 per vertex
    DevBuf<int32_t> d_sub;               // 3 per vertex
    DevBuf<uint32_t> d_tri;              // 3 per triangle
    bool coloured = false;               // built while the colour layer was present: d_rgba holds the vertex colours
    DevBuf<uint32_t> d_rgba;             // one packed r, g, b, a per vertex (bytes in that order)
};

// The colour layer of the volume ("Colour layer"; rule in lv_colour.hpp, kernels in lv_colour.hip) and the buffers of
// lv_colour_integrate.  Nothing is allocated before the first lv_colour_integrate or lv_colour_load.
struct ColourLayer {
    bool present = false;
    DevBuf<uint32_t> d_sums;             // 4 per voxel by grid_at: the sums of R, G, B and the colour weight Wc
    DevBuf<uint32_t> d_next;             // recentre's second buffer, freed when the move is through
    DevBuf<uint32_t> d_bcnt, d_boff;     // candidates per workgroup of the compaction and their exclusive sum
    DevBuf<uint32_t> d_list;             // the candidates' voxel indices in linear order
    DevBuf<uint32_t> d_rgba;             // lv_colour_fetch's and lv_colour_query's packed colours
    PinBuf<uint8_t> h_raw;               // the staged images, the views, the texels, the occlusion cells: as PaintStore's
    PinBuf<PaintCam> h_cams;             // PAINT_MAX_VIEWS entries
    DevBuf<uint8_t> d_raw;
    DevBuf<PaintCam> d_cams;
    DevBuf<uint32_t> d_tex, d_cell, d_tmp;
    void release() {
        release_all(d_sums, d_next, d_bcnt, d_boff, d_list, d_rgba, h_raw, h_cams, d_raw, d_cams, d_tex, d_cell, d_tmp);
        present = false;
    }
};

// The packed cell states of the volume ("Surface ray casting"; rule in lv_tsdf_ray.hpp, kernels in lv_tsdf_ray.hip) and the buffers
// of lv_surf_raycast / lv_surf_raycast_views.  Nothing is allocated before the first of them; the states are built by the first
// call after S or W changed (`packed` false) or with another min_weight.
struct TsdfRays {
    bool packed = false;
    int min_weight = 0;                  // what d_states was packed with
    DevBuf<uint32_t> d_states;           // 2 bits per voxel in lv_ray.hpp's layout
    PointStage pts;                      // lv_surf_raycast: every `from`, then every `to`; _views: every view's returns
    DevBuf<lv_tsdf_ray_result> d_res;
    DevBuf<float> d_nrm;                 // 3 per ray
    DevBuf<uint32_t> d_rgba;             // one packed r, g, b, a per ray
    void release() {
        d_states.release(); pts.release(); d_res.release(); d_nrm.release(); d_rgba.release();
        packed = false;
        min_weight = 0;
    }
};

// The buffers of lv_depth_integrate ("Depth fusion"; rule in lv_depth.hpp, kernel in lv_depth.hip): the staged images and the
// views, pinned and on the device.  Nothing is allocated before the first call that some voxel is judged in.
struct DepthStage {
    PinBuf<uint8_t> h_raw;
    PinBuf<DepthCam> h_cams;             // PAINT_MAX_VIEWS entries
    DevBuf<uint8_t> d_raw;
    DevBuf<DepthCam> d_cams;
    void release() { release_all(h_raw, h_cams, d_raw, d_cams); }
};

// The scratch of lv_surf_sample and lv_surf_align ("Surface registration"; rule in lv_surf_align.hpp, kernels in
// lv_surf_align.hip).  Nothing is allocated before the first of them.
struct SurfAlignStage {
    AlignStage<lv_surf_align_result> loop;   // lv_surf_align's scratch (lv_align.hpp); loop.src holds lv_surf_sample's points too
    DevBuf<double> d_out;                // lv_surf_sample: 4 per point
    DevBuf<uint8_t> d_status;            // lv_surf_sample: one per point
    void release() { release_all(loop, d_out, d_status); }
};

// The staging of lv_surf_merge ("Submap merging"; rule in lv_surf_merge.hpp, kernel in lv_surf_merge.hip): the submap as
// interleaved (S, W) pairs, pinned and on the device, grown on demand.  Nothing is allocated before the first call that launches.
struct SurfMergeRule;   // lv_surf_merge.hpp: one call as the kernel takes it
struct MergeStage {
    PinBuf<int32_t> h_sw;                // 2 per source voxel
    DevBuf<int32_t> d_sw;
    void release() { release_all(h_sw, d_sw); }
};

// The volume of a context and the buffers of its calls.  Nothing is allocated before configure().
struct TsdfStore {
    bool configured = false;
    lv_tsdf_params prm{};
    TsdfGrid grid{};
    size_t n_vox = 0;
    DevBuf<int32_t> d_S, d_W;                 // by grid_at; W = 0: never observed
    DevBuf<unsigned long long> d_scratch;     // one packed word per voxel; all zero between calls
    float origin0[3] = {0.f, 0.f, 0.f};       // the origin of configure(); prm.origin and grid.occ.origin follow the shift
    int32_t shift[3] = {0, 0, 0};             // the accumulated recentre, in voxels
    Counters4 stats;
    PointStage pts;                           // every view's returns, or the query points
    DevBuf<float> d_out;                      // lv_tsdf_query's metres, lv_tsdf_fetch's metres
    DevBuf<int32_t> d_wout;                   // lv_tsdf_query's weights
    TsdfMesh mesh;
    DevBuf<uint32_t> d_flag, d_vid, d_fcnt, d_foff;   // the build's per-voxel arrays (n_vox + 1 each), freed when it ends
    DevBuf<void> d_tmp;                       // hipcub scratch
    ColourLayer colour;                       // the colour layer: zeroed by clear() and load(), moved by recentre(), read by mesh_build(), freed by release()
    TsdfRays rays;                            // the rays' packed states: invalidated by integrate(), integrate_depth(), load(), clear() and recentre() (and for merge() by VolumeTools::surf_merge), freed by release()
    DepthStage depth;                         // integrate_depth()'s staging, freed by release()
    SurfAlignStage align;                     // surf_sample()'s and surf_align()'s scratch, freed by release()
    MergeStage merged;                        // merge()'s staging, freed by release()

    int configure(hipStream_t stream, const lv_tsdf_params& p);
    int clear(hipStream_t stream);
    int integrate(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t out[4]);
    int query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* metres, int32_t* weight);
    int fetch(hipStream_t stream, int32_t* S, int32_t* W, float* metres);
    int load(hipStream_t stream, const int32_t* S, const int32_t* W);
    // as OccStore::recentre; a voxel held evidence iff W > 0
    int recentre(hipStream_t stream, const int32_t d[3], const int32_t s_new[3], const float origin_new[3], uint64_t out[4]);
    int mesh_build(hipStream_t stream, int min_weight, uint64_t counts[4]);
    int mesh_fetch(hipStream_t stream, float* xyz, int32_t* sub, uint32_t* tri);
    void mesh_release();
    void release();

    // ---- ray casting (lv_tsdf_ray.hip).  normals, rgba may be NULL.  Both wait for the stream.
    int raycast(hipStream_t stream, int min_weight, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                lv_tsdf_ray_result* out, float* normals, uint8_t* rgba);
    int raycast_views(hipStream_t stream, int min_weight, const lv_view* views, size_t n_views, lv_tsdf_ray_result* out, float* normals,
                      uint8_t* rgba, uint64_t stats[4]);
    int rays_pack(hipStream_t stream, int min_weight);   // builds the packed states where they are not those of S, W and min_weight

    // ---- depth fusion (lv_depth.hip).  cams, q: depth_rule's.  Marks the rays' states not packed, leaves the colour layer alone,
    // waits for the stream.
    int integrate_depth(hipStream_t stream, const lv_depth_view* views, const DepthCam* cams, const DepthRule& q, uint64_t out[4]);

    // ---- registration (lv_surf_align.hip).  Both read S and W, write nothing of the store but `align`, and wait for the stream.
    int surf_sample(hipStream_t stream, int min_weight, const void* pts, size_t stride, size_t n, double* out, uint8_t* status);
    int surf_align(hipStream_t stream, const lv_surf_align_params& prm, const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses,
                   size_t K, lv_surf_align_result* results, int32_t best[2]);

    // ---- submap merging (lv_surf_merge.hip).  q: surf_merge_rule's with kq filled; lo..hi: surf_merge_box's voxels [lo, hi), not
    // empty.  Writes S and W only, waits for the stream.
    int merge(hipStream_t stream, const lv_surf_submap& sub, const SurfMergeRule& q, const int lo[3], const int hi[3], uint64_t out[4]);

    // ---- the colour layer (lv_colour.hip).  cams, q: paint_rule's.  All of them wait for the stream.
    int colour_ensure(hipStream_t stream);   // allocates the layer, all zero, where it is not present
    int colour_integrate(hipStream_t stream, const lv_camera_view* views, const PaintCam* cams, const PaintRule& q, int band, int min_weight,
                         int max_weight, uint64_t out[4]);
    int colour_fetch(hipStream_t stream, uint32_t* sums, uint8_t* rgba);
    int colour_load(hipStream_t stream, const uint32_t* sums);
    int colour_query(hipStream_t stream, const void* pts, size_t stride, size_t n, uint8_t* rgba);
    int colour_clear(hipStream_t stream);
    int colour_count(hipStream_t stream, uint64_t* coloured);
    int colour_shift(hipStream_t stream, const int32_t d[3]);   // recentre's part: gathers into colour.d_next (the caller swaps)
    int colour_vertices(hipStream_t stream, const uint32_t* flag, const uint32_t* vid, uint32_t n_vert);   // mesh_build's part
    int mesh_colours(hipStream_t stream, uint8_t* rgba);
};

// exclusive sum of in[0 .. n] into out[0 .. n] (n + 1 items: out[n] is the total), then the total to the host (lv_tsdf.hip)
int tsdf_scan(hipStream_t stream, DevBuf<void>& tmp, const uint32_t* in, uint32_t* out, size_t n, uint32_t* total);

}  // namespace lv
