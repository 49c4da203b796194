// lv_surf_merge.hpp — a TSDF submap resampled into the volume under a rigid pose (lv_surf_merge, include/limovelo_hip.h "Submap
// merging"; the kernel and the host side in lv_surf_merge.hip, the call a member of TsdfStore).
//
// The rule's steps 2 to 7 as plain __host__ __device__ code: the destination centre carried into the submap's lattice, the
// position rounded to 1/32 of a source voxel, the eight corners with their integer weights, the distance carried into destination
// units and the (dS, dW) that folds; then the argument rule, the scale kq, and the two shortcuts (which destination voxels the
// submap's box can reach, which tiles of them cannot meet it).  The kernel of lv_surf_merge.hip runs exactly these;
// tests/emu/surf_merge_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and tests/test_surf_merge_host.py holds
// them to tests/surf_merge_ref.py.  The centre is lv_colour.hpp's, the fold lv_tsdf.hpp's, R(q) lv_graph.hpp's.  f64 up to the
// lattice, every operation single and unfused (the library is built with -ffp-contract=off); integers after it.
#pragma once

#include "lv_colour.hpp"
#include "lv_graph.hpp"

namespace lv {

static_assert(sizeof(lv_surf_submap) == 48, "lv_surf_submap is 48 bytes");
static_assert(sizeof(lv_surf_merge_params) == 16, "lv_surf_merge_params is 16 bytes");

constexpr int MERGE_FR = 32;                      // the position is rounded to 1 / FR of a source voxel; the weights sum to FR^3 = 2^15
constexpr double MERGE_U_LIMIT = 16777216.0;      // 2^24: a centre this many source voxels from the submap's origin is OUTSIDE
constexpr int64_t MERGE_KQ_MIN = 512, MERGE_KQ_MAX = 32768;   // kq / 4096 = sub.resolution / resolution in 1/8 .. 8
enum { MERGE_OUTSIDE = 0, MERGE_UNKNOWN = 1, MERGE_KNOWN = 2 };
constexpr int MERGE_TILE_X = 16, MERGE_TILE_Y = 4, MERGE_TILE_Z = 4;   // a workgroup's voxels (lv_surf_merge.hip), a wavefront one z layer of them

// One call as the kernel takes it
struct SurfMergeRule {
    double R[9];          // R(q), row-major: submap -> world
    double t[3];
    double so[3];         // (double)sub.origin_a
    double sr;            // (double)sub.resolution
    int nx, ny, nz;       // the submap's grid
    int32_t min_weight;
    int32_t interp;       // LV_MERGE_*
    int32_t Ts;           // the submap's T = trunc_cells * 256
    int64_t kq;           // floorf((sub.resolution / resolution) * 4096 + 0.5): filled against the volume (surf_merge_scale)
};

// One staged source voxel: a corner is one 8-byte load
struct MergePair {
    int32_t S, W;
};

// Steps 2 and 3: the f32 centre p of a destination voxel -> e[3], its place in the submap's lattice in 1/32 voxel.  false: OUTSIDE
// (a u that is not finite or has |u| >= 2^24)
LV_OCC_HD bool surf_merge_lattice(const SurfMergeRule& q, const float p[3], int64_t e[3]) {
    const double d0 = (double)p[0] - q.t[0], d1 = (double)p[1] - q.t[1], d2 = (double)p[2] - q.t[2];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double x = (q.R[b] * d0 + q.R[3 + b] * d1) + q.R[6 + b] * d2;   // (R^T d)_b
        const double u = (x - q.so[b]) / q.sr - 0.5;
        if (!(fabs(u) < MERGE_U_LIMIT)) return false;   // (a NaN compares false)
        e[b] = q.interp == LV_MERGE_NEAREST ? (int64_t)MERGE_FR * (int64_t)floor(u + 0.5) : (int64_t)floor(u * 32.0 + 0.5);
    }
    return true;
}

// Steps 4 and 5 on the staged pairs (x fastest): the state; for a KNOWN voxel m = sum w a_c and Wn = sum w W_c.  A corner of
// weight 0 is not read and need not exist.
LV_OCC_HD int surf_merge_gather(const SurfMergeRule& q, const int64_t e[3], const MergePair* __restrict__ sw, int64_t& m, int64_t& Wn) {
    const int n[3] = {q.nx, q.ny, q.nz};
    int i[3], f[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const int64_t ib = e[b] >> 5;   // (floor)
        f[b] = (int)(e[b] & 31);
        if (ib < 0 || ib > (int64_t)n[b] - 1 || (f[b] != 0 && ib + 1 > (int64_t)n[b] - 1)) return MERGE_OUTSIDE;
        i[b] = (int)ib;
    }
    const size_t sy = (size_t)q.nx, sz = (size_t)q.nx * (size_t)q.ny;
    const size_t at = ((size_t)i[2] * (size_t)q.ny + (size_t)i[1]) * (size_t)q.nx + (size_t)i[0];
    // corner (a, b, c) at a + 2 b + 4 c; the loads first: they are in flight together
    MergePair c[8];
    int32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int a0 = k & 1, a1 = (k >> 1) & 1, a2 = k >> 2;
        w[k] = (a0 ? f[0] : MERGE_FR - f[0]) * (a1 ? f[1] : MERGE_FR - f[1]) * (a2 ? f[2] : MERGE_FR - f[2]);
        c[k] = MergePair{0, 0};
        if (w[k]) c[k] = sw[at + (size_t)a0 + (size_t)a1 * sy + (size_t)a2 * sz];
    }
    bool known = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) known = known && (w[k] == 0 || c[k].W >= q.min_weight);
    if (!known) return MERGE_UNKNOWN;
    m = 0;
    Wn = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (!w[k]) continue;
        m += (int64_t)w[k] * tsdf_floor_div((int64_t)c[k].S * 256, (int64_t)c[k].W);   // (W >= min_weight >= 1)
        Wn += (int64_t)w[k] * (int64_t)c[k].W;
    }
    return MERGE_KNOWN;
}

// Steps 6 and 7: (m, Wn) -> (dS, dW) in the destination's units, Td the destination's T.  false: DROPPED (behind the band)
LV_OCC_HD bool surf_merge_delta(int64_t kq, int32_t Td, int64_t m, int64_t Wn, int64_t& dS, int64_t& dW) {
    int64_t sbar = tsdf_floor_div(m * kq, (int64_t)1 << 27);
    const int64_t lim = 256 * (int64_t)Td;
    if (sbar < -lim) return false;
    if (sbar > lim) sbar = lim;
    dW = Wn >> 15;
    if (dW < 1) dW = 1;
    dS = tsdf_floor_div(sbar * dW, 256);
    return true;
}

// What one destination voxel with the f32 centre p does: the state, and for a KNOWN voxel whether it contributes (dW > 0) or is
// DROPPED (dW = 0)
LV_OCC_HD int surf_merge_voxel(const SurfMergeRule& q, int32_t Td, const float p[3], const MergePair* __restrict__ sw, int64_t& dS, int64_t& dW) {
    dS = 0;
    dW = 0;
    int64_t e[3], m, Wn;
    if (!surf_merge_lattice(q, p, e)) return MERGE_OUTSIDE;
    const int st = surf_merge_gather(q, e, sw, m, Wn);
    if (st != MERGE_KNOWN) return st;
    if (!surf_merge_delta(q.kq, Td, m, Wn, dS, dW)) dS = dW = 0;
    return MERGE_KNOWN;
}

// ---- the shortcuts.  A voxel that is not OUTSIDE has, on every axis, u in [-1/64, n - 1 + 1/64) (TRILINEAR) or [-1/2, n - 1/2)
// (NEAREST): its centre lies in the submap's box of metres so + [0, n] sr carried to the world.  Neither shortcut changes a result.

// The destination voxels [lo, hi) per axis the submap's box can reach: its eight corners R c + t in f64, widened by a voxel and
// 1e-3 of the box's size and of its distance from the volume's origin, clipped to the grid.  false: none.
inline bool surf_merge_box(const TsdfGrid& g, const SurfMergeRule& q, int lo[3], int hi[3]) {
    const int n[3] = {g.occ.nx, g.occ.ny, g.occ.nz};
    const int ns[3] = {q.nx, q.ny, q.nz};
    double wlo[3] = {0, 0, 0}, whi[3] = {0, 0, 0};
    for (int k = 0; k < 8; ++k) {
        double c[3];
        for (int b = 0; b < 3; ++b) c[b] = q.so[b] + ((k >> b) & 1 ? (double)ns[b] * q.sr : 0.0);
        for (int a = 0; a < 3; ++a) {
            const double x = ((q.R[3 * a] * c[0] + q.R[3 * a + 1] * c[1]) + q.R[3 * a + 2] * c[2]) + q.t[a];
            if (k == 0 || x < wlo[a]) wlo[a] = x;
            if (k == 0 || x > whi[a]) whi[a] = x;
        }
    }
    for (int a = 0; a < 3; ++a) {
        const double res = g.occ.resolution, o = g.occ.origin[a];
        const double slack = res + 1e-3 * (whi[a] - wlo[a]) + 1e-3 * std::fmax(std::fabs(wlo[a] - o), std::fabs(whi[a] - o));
        // centre i sits at origin + (i + 0.5) res
        const double flo = std::floor((wlo[a] - slack - o) / res - 0.5);
        const double fhi = std::ceil((whi[a] + slack - o) / res - 0.5) + 1.0;
        if (!(flo < (double)n[a]) || !(fhi > 0.0)) return false;   // (a NaN: none; surf_merge_rule lets none through)
        lo[a] = flo > 0.0 ? (int)flo : 0;
        hi[a] = fhi < (double)n[a] ? (int)fhi : n[a];
    }
    return true;
}

// true: no voxel whose f32 centre lies in the box of metres [lo, hi] can be anything but OUTSIDE.  The box's centre goes through
// steps 2 and 3 in f64, its half widths through |R|; the tile is given up only when, on some axis, all of it lies beyond
// [-1/2, n - 1/2] by the margin 1e-3 voxel + 1e-6 of the terms' magnitudes, far above the 1e-8 voxel that f64 rounding can move a
// u below 2^24.
LV_OCC_HD bool surf_merge_tile_outside(const SurfMergeRule& q, const float lo[3], const float hi[3]) {
    double d[3], h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = 0.5 * ((double)lo[a] + (double)hi[a]) - q.t[a];
        h[a] = 0.5 * ((double)hi[a] - (double)lo[a]);
    }
    const int n[3] = {q.nx, q.ny, q.nz};
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double x = (q.R[b] * d[0] + q.R[3 + b] * d[1]) + q.R[6 + b] * d[2];
        const double ext = (fabs(q.R[b]) * h[0] + fabs(q.R[3 + b]) * h[1]) + fabs(q.R[6 + b]) * h[2];
        const double mag = (fabs(q.R[b] * d[0]) + fabs(q.R[3 + b] * d[1])) + fabs(q.R[6 + b] * d[2]) + fabs(q.so[b]) + ext;
        const double u = (x - q.so[b]) / q.sr - 0.5, eu = ext / q.sr, margin = 1e-3 + 1e-6 * (mag / q.sr);
        if (u + eu + margin < -0.5) return true;
        if (u - eu - margin > (double)n[b] - 0.5) return true;
    }
    return false;
}

inline void default_surf_merge_params(lv_surf_merge_params* p) {
    if (!p) return;
    *p = lv_surf_merge_params{};
    p->min_weight = 1;
    p->interp = LV_MERGE_TRILINEAR;
}

// Step 6's scale against the volume's resolution: LV_EINVAL outside 512..32768
inline int surf_merge_scale(float sub_resolution, float resolution, int64_t* kq) {
    const float k = floorf((sub_resolution / resolution) * 4096.0f + 0.5f);
    if (!(k >= (float)MERGE_KQ_MIN && k <= (float)MERGE_KQ_MAX)) {
        set_error("lv_surf_merge: the submap's resolution %g against the volume's %g: a ratio of 1/8 to 8", sub_resolution, resolution);
        return LV_EINVAL;
    }
    *kq = (int64_t)k;
    return LV_OK;
}

// lv_surf_merge's arguments against their limits, before the context: LV_EINVAL (nothing written) outside them; inside, the rule
// as the kernel takes it but for kq.  p NULL: the defaults.
inline int surf_merge_rule(const lv_surf_submap* sub, const lv_graph_pose* pose, const lv_surf_merge_params* p, SurfMergeRule* q) {
    using namespace graph_detail;
    if (!sub || !pose) { set_error("lv_surf_merge: null argument"); return LV_EINVAL; }
    lv_surf_merge_params prm;
    default_surf_merge_params(&prm);
    if (p) prm = *p;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(sub->origin[a])) { set_error("lv_surf_merge: submap origin: must be finite"); return LV_EINVAL; }
    if (!(std::isfinite(sub->resolution) && sub->resolution > 0.f)) { set_error("lv_surf_merge: submap resolution = %g: finite and > 0", sub->resolution); return LV_EINVAL; }
    if (sub->nx < 1 || sub->nx > OCC_MAX_DIM || sub->ny < 1 || sub->ny > OCC_MAX_DIM || sub->nz < 1 || sub->nz > OCC_MAX_DIM) {
        set_error("lv_surf_merge: submap of %d x %d x %d voxels: each must be in 1..1024", sub->nx, sub->ny, sub->nz);
        return LV_EINVAL;
    }
    const uint64_t nv = (uint64_t)sub->nx * (uint64_t)sub->ny * (uint64_t)sub->nz;
    if (nv > OCC_MAX_VOXELS) { set_error("lv_surf_merge: submap of %d x %d x %d voxels: at most 2^28", sub->nx, sub->ny, sub->nz); return LV_EINVAL; }
    if (sub->trunc_cells < 1 || sub->trunc_cells > TSDF_MAX_TRUNC) { set_error("lv_surf_merge: submap trunc_cells = %d: must be in 1..16", sub->trunc_cells); return LV_EINVAL; }
    if (!sub->S || !sub->W) { set_error("lv_surf_merge: null S or W"); return LV_EINVAL; }
    if (!finite_all(pose->t, 3)) { set_error("lv_surf_merge: pose: t: a non-finite number"); return LV_EINVAL; }
    if (!finite_all(pose->q, 4)) { set_error("lv_surf_merge: pose: q: a non-finite number"); return LV_EINVAL; }
    if (!unit_quat(pose->q)) { set_error("lv_surf_merge: pose: q: norm off 1 by more than 1e-6"); return LV_EINVAL; }
    if (prm.min_weight < 1) { set_error("lv_surf_merge: min_weight = %d: at least 1", prm.min_weight); return LV_EINVAL; }
    if (prm.interp != LV_MERGE_TRILINEAR && prm.interp != LV_MERGE_NEAREST) { set_error("lv_surf_merge: interp = %d: LV_MERGE_TRILINEAR or LV_MERGE_NEAREST", prm.interp); return LV_EINVAL; }
    TsdfGrid sg{};   // what tsdf_check_volume reads
    sg.T = sub->trunc_cells * 256;
    sg.max_weight = TSDF_MAX_WEIGHT;
    const size_t bad = tsdf_check_volume(sg, sub->S, sub->W, (size_t)nv);
    if (bad != (size_t)nv) {
        set_error("lv_surf_merge: submap voxel %zu: S = %d, W = %d: 0 <= W <= 2^18 and |S| <= T * W", bad, sub->S[bad], sub->W[bad]);
        return LV_EINVAL;
    }
    *q = SurfMergeRule{};
    gr_rot(pose->q, q->R);
    for (int a = 0; a < 3; ++a) {
        q->t[a] = pose->t[a];
        q->so[a] = (double)sub->origin[a];
    }
    q->sr = (double)sub->resolution;
    q->nx = sub->nx;
    q->ny = sub->ny;
    q->nz = sub->nz;
    q->min_weight = prm.min_weight;
    q->interp = prm.interp;
    q->Ts = sg.T;
    q->kq = 0;
    return LV_OK;
}

// The submap's S and W as interleaved pairs
inline void surf_merge_stage(const lv_surf_submap& sub, MergePair* out) {
    const size_t nv = (size_t)sub.nx * (size_t)sub.ny * (size_t)sub.nz;
    for (size_t i = 0; i < nv; ++i) out[i] = MergePair{sub.S[i], sub.W[i]};
}

}  // namespace lv
