// lv_surface.hpp — surface normals and outlier removal on the device map (lv_map_normals / lv_map_remove_outliers,
// include/limovelo_hip.h "Surface normals and outlier removal"; kernels and host side in lv_surface.hip).
//
// The first part is plain inline arithmetic that also compiles for the host (LV_SURFACE_HOST_ONLY: tests/test_surface_host.py
// holds sym3_eig to numpy.linalg.eigh): the 3 x 3 symmetric eigen-solver and the rule that turns a covariance into a normal.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define LV_SURF_HD __host__ __device__ inline __attribute__((always_inline))
#define LV_SURF_UNROLL _Pragma("unroll")
#else
#define LV_SURF_HD inline
#define LV_SURF_UNROLL
#endif

namespace lv {

constexpr int SURF_JACOBI_SWEEPS = 5;   // cyclic Jacobi converges quadratically on a 3 x 3: 4 sweeps reach f64 rounding, the fifth is margin

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 held in scalars: app, aqq, apq the plane's entries, aop, aoq the
// third index's; (v0p, v0q) .. (v2p, v2q) the rows of the accumulated vectors.  Rutishauser's form, the tangent without the
// quotient theta (no overflow): t = 2 apq sgn(d) / (|d| + sqrt(d^2 + 4 apq^2)), d = aqq - app.  An exactly zero apq is skipped.
LV_SURF_HD void sym3_rotate(double& app, double& aqq, double& apq, double& aop, double& aoq, double& v0p, double& v0q, double& v1p,
                            double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double d = aqq - app, two = 2.0 * apq;
    const double den = fabs(d) + sqrt(d * d + two * two);
    double t = den > 0.0 ? two / den : (two < 0.0 ? -1.0 : 1.0);   // (den underflows only with d = 0 and a subnormal apq: 45 degrees)
    if (d < 0.0) t = -t;
    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs, tau = sn / (1.0 + cs);
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double op = aop, oq = aoq;
    aop = op - sn * (oq + tau * op);
    aoq = oq + sn * (op - tau * oq);
    double vp = v0p, vq = v0q;
    v0p = vp - sn * (vq + tau * vp);
    v0q = vq + sn * (vp - tau * vq);
    vp = v1p; vq = v1q;
    v1p = vp - sn * (vq + tau * vp);
    v1q = vq + sn * (vp - tau * vq);
    vp = v2p; vq = v2q;
    v2p = vp - sn * (vq + tau * vp);
    v2q = vq + sn * (vp - tau * vq);
}

// Rayleigh quotient of the normalised (x, y, z) against the symmetric m; normalises in place
LV_SURF_HD double sym3_rayleigh(double m00, double m01, double m02, double m11, double m12, double m22, double& x, double& y, double& z) {
    const double nn = sqrt(x * x + y * y + z * z);
    x /= nn; y /= nn; z /= nn;
    const double mx = m00 * x + m01 * y + m02 * z, my = m01 * x + m11 * y + m12 * z, mz = m02 * x + m12 * y + m22 * z;
    return x * mx + y * my + z * mz;
}

// Eigen-decomposition of the symmetric C = [c[0] c[1] c[2]; c[1] c[3] c[4]; c[2] c[4] c[5]] in f64: l[0] <= l[1] <= l[2] and the
// unit eigenvector v0 of l[0].  Cyclic Jacobi over (0,1), (0,2), (1,2) with a fixed sweep count (no data-dependent loop), every
// rotation written out on scalars (no indexed access: nothing leaves the registers on the device), then every eigenvalue once
// more as the Rayleigh quotient of its accumulated vector, which sheds the rounding the rotations piled up on the diagonal.
// Scale-free: C is scaled by a power of two (exact) so that its largest magnitude is in [1, 2).
// (scalars in and out: the kernel keeps everything in registers; the array form below is the same function)
LV_SURF_HD void sym3_eig(double c0, double c1, double c2, double c3, double c4, double c5, double& e0, double& e1, double& e2, double& nx,
                         double& ny, double& nz) {
    const double big = fmax(fmax(fmax(fabs(c0), fabs(c1)), fmax(fabs(c2), fabs(c3))), fmax(fabs(c4), fabs(c5)));
    if (!(big > 0.0) || !(big < INFINITY)) {   // the zero matrix (or a non-finite one): no direction
        e0 = e1 = e2 = big > 0.0 ? big : 0.0;
        nx = 0.0; ny = 0.0; nz = 1.0;
        return;
    }
    const int e = ilogb(big);
    const double s = scalbn(1.0, -e), si = scalbn(1.0, e);
    const double m00 = c0 * s, m01 = c1 * s, m02 = c2 * s, m11 = c3 * s, m12 = c4 * s, m22 = c5 * s;
    double a00 = m00, a01 = m01, a02 = m02, a11 = m11, a12 = m12, a22 = m22;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // vij: row i, column j
    LV_SURF_UNROLL
    for (int sweep = 0; sweep < SURF_JACOBI_SWEEPS; ++sweep) {
        sym3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third index 2
        sym3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third index 1
        sym3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third index 0
    }
    const double q0 = sym3_rayleigh(m00, m01, m02, m11, m12, m22, v00, v10, v20);
    const double q1 = sym3_rayleigh(m00, m01, m02, m11, m12, m22, v01, v11, v21);
    const double q2 = sym3_rayleigh(m00, m01, m02, m11, m12, m22, v02, v12, v22);
    // the smallest eigenvalue's vector, blended with exact 0 / 1 weights (a chain of selects over nine values is turned into an
    // indexed table in private memory by the compiler; ties go to the lower column)
    const double l0 = fmin(q0, fmin(q1, q2));
    const double w0 = q0 == l0 ? 1.0 : 0.0, w1 = (q0 != l0 && q1 == l0) ? 1.0 : 0.0, w2 = 1.0 - w0 - w1;
    const double x0 = (w0 * v00 + w1 * v01) + w2 * v02, y0 = (w0 * v10 + w1 * v11) + w2 * v12, z0 = (w0 * v20 + w1 * v21) + w2 * v22;
    const double l2 = fmax(q0, fmax(q1, q2));
    // the middle one: what is neither the minimum nor the maximum (by value: equal values are interchangeable)
    const double l1 = fmax(fmin(q0, q1), fmin(fmax(q0, q1), q2));
    e0 = l0 * si; e1 = l1 * si; e2 = l2 * si;
    nx = x0; ny = y0; nz = z0;
}
LV_SURF_HD void sym3_eig(const double c[6], double l[3], double v0[3]) {
    sym3_eig(c[0], c[1], c[2], c[3], c[4], c[5], l[0], l[1], l[2], v0[0], v0[1], v0[2]);
}

// The sign of a normal (include/limovelo_hip.h): +1 or -1 to multiply (vx, vy, vz) by.  orient 1: (tx, ty, tz) = viewpoint - p.
LV_SURF_HD double surf_sign(double vx, double vy, double vz, int orient, double tx, double ty, double tz) {
    if (orient) {
        const double d = (vx * tx + vy * ty) + vz * tz;
        if (d > 0.0) return 1.0;
        if (d < 0.0) return -1.0;
    }
    double big = vx;   // the component of largest magnitude, ties to the lower axis
    if (fabs(vy) > fabs(big)) big = vy;
    if (fabs(vz) > fabs(big)) big = vz;
    return big < 0.0 ? -1.0 : 1.0;
}

// Normal (f32, rounded once) and curvature of one point from its covariance; n < min_neighbours: (0, 0, 0) and NaN
LV_SURF_HD void surf_normal(double c0, double c1, double c2, double c3, double c4, double c5, int n, int min_neighbours, int orient, double tx,
                            double ty, double tz, float& n0, float& n1, float& n2, float& curv) {
    if (n < min_neighbours) {
        n0 = n1 = n2 = 0.f;
        curv = NAN;
        return;
    }
    double l0, l1, l2, vx, vy, vz;
    sym3_eig(c0, c1, c2, c3, c4, c5, l0, l1, l2, vx, vy, vz);
    const double sg = surf_sign(vx, vy, vz, orient, tx, ty, tz);
    n0 = (float)(sg * vx);
    n1 = (float)(sg * vy);
    n2 = (float)(sg * vz);
    const double tr = (l0 + l1) + l2;
    curv = tr > 0.0 ? (float)(l0 / tr) : 0.f;
}

}  // namespace lv

#if !defined(LV_SURFACE_HOST_ONLY)
#include "lv_host.hpp"
#include "lv_rules.hpp"   // SURF_MAX_K, SurfRule

namespace lv {

// The buffers of lv_map_normals / lv_map_remove_outliers (grown on demand, kept)
struct SurfaceStore {
    DevBuf<double> d_val;           // by id: 6 covariance entries (job 0) or the point's value (jobs 1, 2)
    DevBuf<double> d_part;          // block partials of the statistics; the journaled rule's device copy
    DevBuf<float> d_normals;        // outputs at living ranks
    DevBuf<float> d_curv;
    DevBuf<float> d_mean;
    DevBuf<int32_t> d_used;
    DevBuf<uint8_t> d_flags;
    PinBuf<double> h_part;
    uint64_t val_gen = 0;           // the map stamp (MapStore::gen) and rule d_val was computed for by the last surface_search
    SurfRule val_rule{};
    int ensure(size_t n_ids, size_t m, int job);
    void release();
};

// k nearest living neighbours of every living point of `map` and the rule's reduction over them, enqueued on `stream`
int surface_search(const MapStore& map, hipStream_t stream, SurfaceStore& st, const SurfRule& q, const uint32_t* rank);
// job 0: normals / curvature at the living ranks from the covariances of surface_search
int surface_finish(const MapStore& map, hipStream_t stream, SurfaceStore& st, const SurfRule& q, const uint32_t* rank);
// jobs 1, 2: search, statistics (unless fixed), classification; flags (device, may be NULL) at the living ranks; remove: the
// outliers leave the map (its dead list, MapStore::kill_dead_list).  q.threshold is resolved on return.  reuse_values: the values
// of the store's last search stand if they were computed for this state of this map (its stamp) and this search.  Synchronises.
int surface_outliers(MapStore& map, hipStream_t stream, SurfaceStore& st, SurfRule& q, const uint32_t* rank, bool want_flags, bool remove,
                     uint32_t* n_removed, double stats[3], bool reuse_values = false);

}  // namespace lv
#endif
