// lv_planes.hpp — RANSAC plane segmentation of the device map (lv_map_planes, include/limovelo_hip.h "Plane segmentation";
// kernels and host side in lv_planes.hip).
//
// The first part is plain inline arithmetic that also compiles for the host (LV_PLANES_HOST_ONLY with LV_SURFACE_HOST_ONLY:
// tests/test_planes_host.py holds it to tests/planes_ref.py by bits): the argument rule, the hash that draws the samples, the
// plane of a hypothesis, the inlier test, the quantisation of the refit and its exact 128-bit fold.  Everything the result
// depends on is either f64 arithmetic of one lane in a written order, an f32 test of one point, or an integer sum: the launch
// geometry cannot change it.
#pragma once

#include <math.h>
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "../../include/limovelo_hip.h"
#include "lv_surface.hpp"   // sym3_eig, surf_sign

#if defined(__HIPCC__)
#define LV_PL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LV_PL_HD inline
#endif

namespace lv {

void set_error(const char* fmt, ...);

// ---- the argument rule
constexpr uint32_t PLANE_MAX_ITERATIONS = 65536;
constexpr uint32_t PLANE_MAX_PLANES = 32;
constexpr uint32_t PLANE_MIN_INLIERS = 3;
constexpr uint32_t PLANE_MAX_IDS = 0x7FFFFF00u;   // (the scans count in int)

// The rule of one call, as the kernels take it: the axis normalised and both thresholds resolved once, in f64, on the host
struct PlaneRule {
    float distance;
    uint32_t iterations, max_planes, min_inliers;
    uint64_t seed;
    int constraint;
    int refine;
    double axis[3];    // unit (constraint 0: zero)
    double cos_max;    // constraint 1: a hypothesis needs t >= cos_max
    double sin_max;    // constraint 2: a hypothesis needs t <= sin_max
};

inline void default_plane_params(lv_plane_params* p) {
    if (!p) return;
    p->distance = 0.1f;
    p->iterations = 512;
    p->max_planes = 1;
    p->min_inliers = 100;
    p->seed = 0;
    p->constraint = 0;
    p->axis[0] = 0.f;
    p->axis[1] = 0.f;
    p->axis[2] = 1.f;
    p->max_angle = (float)(10.0 * 3.14159265358979323846 / 180.0);
    p->refine = 1;
}

// The parameters of lv_map_planes against their limits: LV_EINVAL (nothing written) outside them; *q zeroed by the caller.
// axis and max_angle are judged only where they are read (constraint != 0).
inline int plane_rule(const lv_plane_params* p, PlaneRule* q) {
    if (!p) { set_error("null argument"); return LV_EINVAL; }
    if (!(std::isfinite(p->distance) && p->distance > 0.f)) { set_error("distance = %g: finite and > 0", p->distance); return LV_EINVAL; }
    if (p->iterations < 1 || p->iterations > PLANE_MAX_ITERATIONS) { set_error("iterations = %u: must be in 1..%u", p->iterations, PLANE_MAX_ITERATIONS); return LV_EINVAL; }
    if (p->max_planes < 1 || p->max_planes > PLANE_MAX_PLANES) { set_error("max_planes = %u: must be in 1..%u", p->max_planes, PLANE_MAX_PLANES); return LV_EINVAL; }
    if (p->min_inliers < PLANE_MIN_INLIERS) { set_error("min_inliers = %u: must be >= %u", p->min_inliers, PLANE_MIN_INLIERS); return LV_EINVAL; }
    if (p->constraint < 0 || p->constraint > 2) { set_error("constraint = %d: 0 (none), 1 (along the axis) or 2 (perpendicular to it)", p->constraint); return LV_EINVAL; }
    q->distance = p->distance;
    q->iterations = p->iterations;
    q->max_planes = p->max_planes;
    q->min_inliers = p->min_inliers;
    q->seed = p->seed;
    q->constraint = p->constraint;
    q->refine = p->refine != 0 ? 1 : 0;
    q->axis[0] = q->axis[1] = q->axis[2] = 0.0;
    q->cos_max = 0.0;
    q->sin_max = 0.0;
    if (p->constraint != 0) {
        const double x = (double)p->axis[0], y = (double)p->axis[1], z = (double)p->axis[2];
        const double len = sqrt((x * x + y * y) + z * z);
        if (!(std::isfinite(p->axis[0]) && std::isfinite(p->axis[1]) && std::isfinite(p->axis[2]) && len > 0.0)) {
            set_error("axis (%g, %g, %g): finite and non-zero", p->axis[0], p->axis[1], p->axis[2]);
            return LV_EINVAL;
        }
        const double a = (double)p->max_angle;
        if (!(a > 0.0 && a < 1.57079632679489661923)) { set_error("max_angle = %g: must be inside (0, pi / 2)", p->max_angle); return LV_EINVAL; }
        q->axis[0] = x / len;
        q->axis[1] = y / len;
        q->axis[2] = z / len;
        q->cos_max = cos(a);
        q->sin_max = sin(a);
    }
    return LV_OK;
}

// ---- the draws
// splitmix64's finaliser with its additive constant
LV_PL_HD uint64_t pl_mix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the high 64 bits of a * b, from 32-bit halves (the same code on both sides)
LV_PL_HD uint64_t pl_umulhi(uint64_t a, uint64_t b) {
    const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
// draw j (0..2) of hypothesis h in round r among n candidates: an index in [0, n)
LV_PL_HD uint32_t pl_draw(uint64_t seed, uint32_t r, uint32_t h, uint32_t j, uint32_t n) {
    const uint64_t u = pl_mix(seed ^ pl_mix(((uint64_t)r << 40) | ((uint64_t)h << 8) | (uint64_t)j));
    return (uint32_t)pl_umulhi(u, (uint64_t)n);
}

// ---- the plane of a hypothesis
// the sign of a plane's normal: constraint 1 towards the axis, otherwise (and when that dot product is 0) surf_sign's orient 0
LV_PL_HD double pl_sign(double nx, double ny, double nz, int constraint, double ax, double ay, double az) {
    return surf_sign(nx, ny, nz, constraint == 1 ? 1 : 0, ax, ay, az);
}
// The plane through p0, p1, p2 (f32 points, f64 arithmetic, unfused, in the order written): false = the hypothesis is invalid
// (a sliver: cc <= 1e-12 uu vv, NaN included; or outside the constraint).  normal: the unit normal rounded to f32; the anchor is p0.
LV_PL_HD bool pl_hypothesis(const float p0[3], const float p1[3], const float p2[3], int constraint, double ax, double ay, double az,
                            double cos_max, double sin_max, float normal[3]) {
    const double ux = (double)p1[0] - (double)p0[0], uy = (double)p1[1] - (double)p0[1], uz = (double)p1[2] - (double)p0[2];
    const double vx = (double)p2[0] - (double)p0[0], vy = (double)p2[1] - (double)p0[1], vz = (double)p2[2] - (double)p0[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    const double cc = (cx * cx + cy * cy) + cz * cz;
    const double uu = (ux * ux + uy * uy) + uz * uz;
    const double vv = (vx * vx + vy * vy) + vz * vz;
    normal[0] = normal[1] = normal[2] = 0.f;
    if (!(cc > 1e-12 * (uu * vv))) return false;
    const double len = sqrt(cc);
    double nx = cx / len, ny = cy / len, nz = cz / len;
    const double sg = pl_sign(nx, ny, nz, constraint, ax, ay, az);
    nx = sg * nx; ny = sg * ny; nz = sg * nz;
    if (constraint != 0) {
        const double t = fabs((nx * ax + ny * ay) + nz * az);
        if (constraint == 1 && !(t >= cos_max)) return false;
        if (constraint == 2 && !(t <= sin_max)) return false;
    }
    normal[0] = (float)nx;
    normal[1] = (float)ny;
    normal[2] = (float)nz;
    return true;
}

// ---- the inlier test (f32, unfused)
LV_PL_HD float pl_signed(float nx, float ny, float nz, float ax, float ay, float az, float px, float py, float pz) {
    const float qx = px - ax, qy = py - ay, qz = pz - az;
    return (nx * qx + ny * qy) + nz * qz;
}
LV_PL_HD bool pl_inlier(float nx, float ny, float nz, float ax, float ay, float az, float px, float py, float pz, float distance) {
    return fabsf(pl_signed(nx, ny, nz, ax, ay, az, px, py, pz)) <= distance;
}

// ---- the refit
constexpr float PL_QUANT = 256.f;            // 1 / 256 m
constexpr float PL_QUANT_MAX = 4194304.f;    // 2^22: |g| beyond it is left out of the sums
// g = rint((p - a) * 256) (the f32 subtraction, the exact scaling, round half to even); false: |g| > 2^22 (or not a number), g = 0
LV_PL_HD bool pl_quant(float p, float a, int32_t* g) {
    const float r = rintf((p - a) * PL_QUANT);
    const bool ok = fabsf(r) <= PL_QUANT_MAX;
    *g = ok ? (int32_t)r : 0;
    return ok;
}
// the sums of one point set: n, S1 (x, y, z), S2 (xx, xy, xz, yy, yz, zz); int64 holds 2^19 points (2^44 each)
constexpr int PL_SUMS = 10;
LV_PL_HD void pl_accumulate(long long s[PL_SUMS], int32_t gx, int32_t gy, int32_t gz) {
    const long long x = gx, y = gy, z = gz;
    s[0] += 1;
    s[1] += x; s[2] += y; s[3] += z;
    s[4] += x * x; s[5] += x * y; s[6] += x * z; s[7] += y * y; s[8] += y * z; s[9] += z * z;
}

// (host code from here to the geometry: the fold, the 3 x 3 and the offset run once per plane)
// The fixed slots of the workgroups (PL_SUMS int64 each) folded in 128 bits, then M = n S2 - S1 S1^T exactly, each entry
// converted to f64 once.  Returns n_fit.
inline uint64_t pl_fold(const long long* slots, size_t n_slots, double m[6], double s1[3]) {
    __int128 t[PL_SUMS];
    for (int k = 0; k < PL_SUMS; ++k) t[k] = 0;
    for (size_t i = 0; i < n_slots; ++i)
        for (int k = 0; k < PL_SUMS; ++k) t[k] += (__int128)slots[i * PL_SUMS + k];
    const __int128 n = t[0];
    m[0] = (double)(n * t[4] - t[1] * t[1]);
    m[1] = (double)(n * t[5] - t[1] * t[2]);
    m[2] = (double)(n * t[6] - t[1] * t[3]);
    m[3] = (double)(n * t[7] - t[2] * t[2]);
    m[4] = (double)(n * t[8] - t[2] * t[3]);
    m[5] = (double)(n * t[9] - t[3] * t[3]);
    for (int a = 0; a < 3; ++a) s1[a] = (double)t[1 + a];
    return (uint64_t)n;
}
// The least-squares plane of the folded sums around `anchor`: normal (sign rule of the hypotheses), anchor and rms in place.
// n_fit < 3: nothing changes, false.
inline bool pl_refit(uint64_t n_fit, const double m[6], const double s1[3], int constraint, const double axis[3], float normal[3],
                     float anchor[3], double* rms) {
    if (n_fit < 3) return false;
    double l[3], v[3];
    sym3_eig(m, l, v);
    const double sg = pl_sign(v[0], v[1], v[2], constraint, axis[0], axis[1], axis[2]);
    for (int a = 0; a < 3; ++a) {
        normal[a] = (float)(sg * v[a]);
        anchor[a] = (float)((double)anchor[a] + s1[a] / (256.0 * (double)n_fit));
    }
    *rms = sqrt(l[0] > 0.0 ? l[0] : 0.0) / (256.0 * (double)n_fit);
    return true;
}
// d of normal . p + d = 0
inline double pl_offset(const float normal[3], const float anchor[3]) {
    return -(((double)normal[0] * (double)anchor[0] + (double)normal[1] * (double)anchor[1]) + (double)normal[2] * (double)anchor[2]);
}

// launch geometry of the scoring kernel (tests/test_gpu_map_planes.py sizes its edge cases by them)
constexpr int PL_CHUNK = 256;     // hypotheses per workgroup, one lane each
constexpr int PL_TILE = 1024;     // candidates per workgroup, staged in the LDS
constexpr int PL_FIT_PER = 16;    // refit: candidates per lane, 4096 per workgroup (2^44 * 2^12 < 2^63)

}  // namespace lv

#if !defined(LV_PLANES_HOST_ONLY)
#include "lv_host.hpp"

namespace lv {

// The buffers of lv_map_planes (grown on demand, kept)
struct PlaneStore {
    DevBuf<int32_t> d_state;        // by id: PL_OUT (dead or excluded), PL_FREE (a candidate), or the plane that took it
    DevBuf<uint32_t> d_flag;        // by id: 1 at a candidate; d_pos: its exclusive scan (n_ids + 1: the last entry is n)
    DevBuf<uint32_t> d_pos;
    DevBuf<float4> d_cand;          // the round's candidates in map order: x, y, z, id
    DevBuf<float4> d_hyp;           // two per hypothesis: (normal, valid), (anchor, 0)
    DevBuf<uint32_t> d_count;       // the hypotheses' counts; [iterations]: the members the classify kernel labelled
    DevBuf<long long> d_slot;       // PL_SUMS per refit workgroup
    DevBuf<int32_t> d_labels;       // output at living ranks
    DevBuf<uint8_t> d_mask;         // the caller's mask at living ranks
    DevBuf<void> d_tmp;             // hipcub scratch
    PinBuf<uint32_t> h_count;       // the counts read back; [iterations + 1]: n
    PinBuf<long long> h_slot;
    int ensure(size_t n_ids, size_t m, uint32_t iterations);
    void release();
};

// Up to q.max_planes planes of `map` under `q` (mask: device, m bytes at living ranks, or NULL; rank: QueryStore::ensure_rank's):
// the labels at the living ranks in st.d_labels (want_labels), the records in planes[0 .. *n_planes), which has room for
// PLANE_MAX_PLANES.  Synchronises.
int planes_extract(const MapStore& map, hipStream_t stream, PlaneStore& st, const PlaneRule& q, const uint32_t* rank, const uint8_t* mask,
                   bool want_labels, lv_plane* planes, size_t* n_planes);

}  // namespace lv
#endif
