// lv_traj.hip — the device trajectory (include/limovelo_hip.h "Trajectory"): the kernels that run the rule of lv_traj.hpp and the
// host side of the store.
//
// Plain stream launches, no float atomics, one lane per item:
//   traj_derive_kernel     per knot the interval record (p_b - p_a, Log(q_a^-1 q_b)) and its time into the packed time array; runs
//                          after set, smooth and correct, so a point costs one Exp, one quaternion product and one rotation;
//   traj_sample_kernel     per time the sample rule on the whole trajectory;
//   traj_smooth_kernel     per knot one Jacobi step from the old buffer into the other;
//   traj_correct_kernel    per knot the correction sampled at the knot's time, applied in place;
//   traj_frame_kernel      one lane: F = (T(frame_time) E)^-1 of a register call;
//   traj_register_kernel   a workgroup of 256 consecutive points: the least and greatest finite time of the chunk, the knot range
//                          that brackets them (two wavefronts search the time array 64 ways a round), then either the range staged
//                          in LDS and searched there by every lane (tile route) or every lane's own search of the global time
//                          array (search route); the same traj_pose_at on the same knots either way.  The four counters are integer
//                          atomics, one per workgroup.
// Host arrays go through pinned staging in pieces of TRAJ_CHUNK points, one after the other: such a call is bound by its transfers
// (DESIGN.md "Trajectory" has the split).
#include "lv_traj.hpp"

#include <algorithm>

namespace lv {

namespace {

constexpr int TB = (int)TRAJ_WG;

__global__ __launch_bounds__(TB) void traj_derive_kernel(const lv_traj_knot* __restrict__ knots, uint32_t n, TrajDerived* __restrict__ der,
                                                         double* __restrict__ times) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    TrajDerived d;
    if (i + 1 < n) {
        traj_derive(knots[i], knots[i + 1], &d);
    } else {
        for (int k = 0; k < 3; ++k) d.dp[k] = d.w[k] = 0.0;
    }
    der[i] = d;
    times[i] = knots[i].time;
}

__global__ __launch_bounds__(TB) void traj_sample_kernel(const double* __restrict__ times, const lv_traj_knot* __restrict__ knots,
                                                         const TrajDerived* __restrict__ der, uint32_t n, const double* __restrict__ at,
                                                         uint32_t count, int extrapolate, lv_graph_pose* __restrict__ out,
                                                         uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= count) return;
    lv_graph_pose o;
    const int st = traj_pose_at(times, knots, der, 0, n, n, at[i], extrapolate, &o);
    out[i] = o;
    status[i] = (uint8_t)st;
}

__global__ __launch_bounds__(TB) void traj_smooth_kernel(const lv_traj_knot* __restrict__ knots, uint32_t n, const uint8_t* __restrict__ fixed,
                                                         int pin_ends, double sigma, uint32_t half_window, lv_traj_knot* __restrict__ next) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if ((fixed && fixed[i]) || (pin_ends && (i == 0 || i + 1 == n))) {
        next[i] = knots[i];
        return;
    }
    lv_traj_knot o;
    traj_smooth_knot(knots, n, i, sigma, half_window, &o);
    next[i] = o;
}

__global__ __launch_bounds__(TB) void traj_correct_kernel(const double* __restrict__ ctimes, const lv_traj_knot* __restrict__ corr,
                                                          const TrajDerived* __restrict__ cder, uint32_t m, lv_traj_knot* __restrict__ knots,
                                                          uint32_t n) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const lv_traj_knot a = knots[i];
    lv_graph_pose D;
    traj_pose_at(ctimes, corr, cder, 0, m, m, a.time, LV_TRAJ_CLAMP, &D);
    lv_traj_knot o;
    traj_correct_knot(D, a, &o);
    knots[i] = o;
}

struct TrajRigid {
    double m[12];
};

__global__ void traj_frame_kernel(const double* __restrict__ times, const lv_traj_knot* __restrict__ knots, const TrajDerived* __restrict__ der,
                                  uint32_t n, double frame_time, TrajRigid E, double* __restrict__ F) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    lv_graph_pose T;
    traj_pose_at(times, knots, der, 0, n, n, frame_time, LV_TRAJ_CLAMP, &T);
    double f[12];
    traj_frame(T, E.m, f);
    for (int k = 0; k < 12; ++k) F[k] = f[k];
}

// The first index in [0, n) whose time is > bound, found by one wavefront: 64 samples a round (the predicate is monotone, so the
// count of samples at or below the bound says which of the 64 pieces holds the answer).  The same index as traj_bracket.
__device__ __forceinline__ uint32_t wave_bracket(const double* __restrict__ times, uint32_t n, double bound) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t span = hi - lo;
        const uint32_t step = (span + 63u) / 64u;
        const uint64_t idx = (uint64_t)lo + (uint64_t)lane * step;
        bool below = false;
        if (idx < hi) below = times[idx] <= bound;
        const uint32_t c = (uint32_t)__popcll(__ballot(below));
        if (step == 1u) return lo + c;
        if (c == 0u) return lo;
        const uint32_t nlo = lo + (c - 1u) * step + 1u;
        const uint32_t nhi = lo + c * step < hi ? lo + c * step : hi;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(TB) void traj_register_kernel(const double* __restrict__ times, const lv_traj_knot* __restrict__ knots,
                                                           const TrajDerived* __restrict__ der, uint32_t n, TrajPoints in, uint32_t count,
                                                           int extrapolate, TrajRigid E, const double* __restrict__ F, int use_tile,
                                                           float* __restrict__ out, uint8_t* __restrict__ status,
                                                           unsigned long long* __restrict__ stats) {
    __shared__ double s_times[TRAJ_TILE];
    __shared__ lv_traj_knot s_knots[TRAJ_TILE];
    __shared__ TrajDerived s_der[TRAJ_TILE];
    __shared__ double s_fold[2][TB / 64];
    __shared__ uint32_t s_ub[2];
    __shared__ uint32_t s_inside[TB / 64];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t i = blockIdx.x * TB + tid;
    const bool live = i < count;
    float p[3] = {0.f, 0.f, 0.f};
    double t = NAN;
    if (live) {
        const float* src = in.xyz + (size_t)i * in.xyz_stride;
        p[0] = src[0];
        p[1] = src[1];
        p[2] = src[2];
        t = in.times[(size_t)i * in.time_stride];
    }
    // the chunk's least and greatest finite time: wavefronts by butterfly, then the four of them
    const bool fin = live && traj_finite(t);
    const double lo_w = wave_min(fin ? t : INFINITY), hi_w = wave_max(fin ? t : -INFINITY);
    if (lane == 0) {
        s_fold[0][wave] = lo_w;
        s_fold[1][wave] = hi_w;
    }
    __syncthreads();
    double t_min = s_fold[0][0], t_max = s_fold[1][0];
#pragma unroll
    for (int w = 1; w < TB / 64; ++w) {
        t_min = s_fold[0][w] < t_min ? s_fold[0][w] : t_min;
        t_max = s_fold[1][w] > t_max ? s_fold[1][w] : t_max;
    }
    const bool any = t_min <= t_max;
    // the range of knots: wavefront 0 brackets the least time, wavefront 1 the greatest
    if (use_tile && any && wave < 2) {
        const uint32_t ub = wave_bracket(times, n, wave ? t_max : t_min);
        if (lane == 0) s_ub[wave] = ub;
    }
    __syncthreads();
    uint32_t k_lo = 0, k_end = 0;
    bool tile = false;
    if (use_tile) {
        traj_tile_range_from(any ? s_ub[0] : 0, any ? s_ub[1] : 0, n, any, &k_lo, &k_end);
        tile = k_end - k_lo <= TRAJ_TILE;
    }
    lv_graph_pose T;
    int st;
    if (tile) {   // (uniform over the workgroup)
        const uint32_t cnt = k_end - k_lo;
        for (uint32_t k = tid; k < cnt; k += TB) {
            s_times[k] = times[k_lo + k];
            s_knots[k] = knots[k_lo + k];
            s_der[k] = der[k_lo + k];
        }
        __syncthreads();
        st = traj_pose_at(s_times, s_knots, s_der, k_lo, cnt, n, t, extrapolate, &T);
    } else {
        st = traj_pose_at(times, knots, der, 0, n, n, t, extrapolate, &T);
    }
    float o[3];
    st = traj_register_point(E.m, T, st, F, p, o);
    if (live) {
        if (out) {
            out[3 * (size_t)i] = o[0];
            out[3 * (size_t)i + 1] = o[1];
            out[3 * (size_t)i + 2] = o[2];
        }
        if (status) status[i] = (uint8_t)st;
    }
    const uint32_t inside_w = (uint32_t)__popcll(__ballot(live && st == LV_TRAJ_INSIDE));
    if (lane == 0) s_inside[wave] = inside_w;
    __syncthreads();
    if (tid == 0) {
        uint32_t inside = 0;
        for (int w = 0; w < TB / 64; ++w) inside += s_inside[w];
        const uint32_t here = count - blockIdx.x * TB < (uint32_t)TB ? count - blockIdx.x * TB : (uint32_t)TB;
        atomicAdd(&stats[0], (unsigned long long)inside);
        atomicAdd(&stats[1], (unsigned long long)(here - inside));
        atomicAdd(&stats[tile ? 2 : 3], 1ull);
    }
}

}  // namespace

int TrajStore::derive(hipStream_t stream) {
    hipLaunchKernelGGL(traj_derive_kernel, dim3(blocks_of(n, TB)), dim3(TB), 0, stream, d_knots.p, (uint32_t)n, d_der.p, d_times.p);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int TrajStore::assign(hipStream_t stream, const lv_traj_knot* knots, size_t nn) {
    LV_HIP(hipStreamSynchronize(stream));   // nothing of the old trajectory is in flight when its buffers go
    set = false;
    int rc = need_all(nn, d_knots, d_next, d_der, d_times, d_fixed);
    if (!rc) rc = d_F.need(12);
    if (!rc) rc = counters.need();
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_knots.p, knots, nn * sizeof(lv_traj_knot), hipMemcpyHostToDevice, stream));
    n = nn;
    rc = derive(stream);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));   // (the caller's array is the copy's source)
    info = lv_traj_info{};
    info.set = 1;
    info.n = (uint32_t)nn;
    info.t_first = knots[0].time;
    info.t_last = knots[nn - 1].time;
    set = true;
    return LV_OK;
}

int TrajStore::fetch(hipStream_t stream, lv_traj_knot* knots) {
    LV_HIP(hipMemcpyAsync(knots, d_knots.p, n * sizeof(lv_traj_knot), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TrajStore::sample(hipStream_t stream, const double* at, size_t count, int extrapolate, lv_graph_pose* out, uint8_t* status) {
    for (size_t off = 0; off < count; off += TRAJ_CHUNK) {
        const size_t c = std::min(TRAJ_CHUNK, count - off);
        LV_HIP(hipStreamSynchronize(stream));
        int rc = d_t.need_pow2(c, 4096);
        if (!rc) rc = d_poses.need_pow2(c, 4096);
        if (!rc) rc = d_status.need_pow2(c, 4096);
        if (rc) return rc;
        LV_HIP(hipMemcpyAsync(d_t.p, at + off, c * sizeof(double), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(traj_sample_kernel, dim3(blocks_of(c, TB)), dim3(TB), 0, stream, d_times.p, d_knots.p, d_der.p, (uint32_t)n, d_t.p,
                           (uint32_t)c, extrapolate, d_poses.p, d_status.p);
        LV_HIP(hipGetLastError());
        if (out) LV_HIP(hipMemcpyAsync(out + off, d_poses.p, c * sizeof(lv_graph_pose), hipMemcpyDeviceToHost, stream));
        if (status) LV_HIP(hipMemcpyAsync(status + off, d_status.p, c, hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
    }
    return LV_OK;
}

int TrajStore::smooth(hipStream_t stream, const lv_traj_smooth_params& prm, const uint8_t* fixed) {
    if (prm.iterations == 0) return LV_OK;
    if (fixed) LV_HIP(hipMemcpyAsync(d_fixed.p, fixed, n, hipMemcpyHostToDevice, stream));
    for (int it = 0; it < prm.iterations; ++it) {
        hipLaunchKernelGGL(traj_smooth_kernel, dim3(blocks_of(n, TB)), dim3(TB), 0, stream, d_knots.p, (uint32_t)n, fixed ? d_fixed.p : nullptr,
                           prm.pin_ends ? 1 : 0, prm.sigma, (uint32_t)prm.half_window, d_next.p);
        LV_HIP(hipGetLastError());
        std::swap(d_knots, d_next);
    }
    const int rc = derive(stream);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));   // (fixed is the caller's)
    info.smooth_iterations += (uint32_t)prm.iterations;
    return LV_OK;
}

int TrajStore::correct(hipStream_t stream, const lv_traj_knot* corr, size_t m) {
    LV_HIP(hipStreamSynchronize(stream));
    int rc = need_all(m, d_corr, d_cder, d_ctimes);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_corr.p, corr, m * sizeof(lv_traj_knot), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(traj_derive_kernel, dim3(blocks_of(m, TB)), dim3(TB), 0, stream, d_corr.p, (uint32_t)m, d_cder.p, d_ctimes.p);
    LV_HIP(hipGetLastError());
    hipLaunchKernelGGL(traj_correct_kernel, dim3(blocks_of(n, TB)), dim3(TB), 0, stream, d_ctimes.p, d_corr.p, d_cder.p, (uint32_t)m, d_knots.p,
                       (uint32_t)n);
    LV_HIP(hipGetLastError());
    rc = derive(stream);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));
    ++info.corrections;
    return LV_OK;
}

// the extrinsic as a rigid map, the counters zeroed, and F on the device when the frame asks for it
int TrajStore::begin_register(hipStream_t stream, const lv_traj_register_params& prm, double* E) {
    traj_rigid(prm.ext_t, prm.ext_q, E);
    LV_HIP(hipStreamSynchronize(stream));
    const int rc = counters.zero(stream);
    if (rc) return rc;
    if (prm.frame == LV_TRAJ_FRAME_AT) {
        TrajRigid e;
        std::memcpy(e.m, E, sizeof(e.m));
        hipLaunchKernelGGL(traj_frame_kernel, dim3(1), dim3(64), 0, stream, d_times.p, d_knots.p, d_der.p, (uint32_t)n, prm.frame_time, e, d_F.p);
        LV_HIP(hipGetLastError());
    }
    return LV_OK;
}

// one launch over count <= TRAJ_CHUNK points; the results land in d_out / d_status
int TrajStore::launch_register(hipStream_t stream, const lv_traj_register_params& prm, const double* E, const TrajPoints& in, size_t count,
                               bool want_out, bool want_status) {
    int rc = LV_OK;
    if (want_out) rc = d_out.need_pow2(3 * count, 3 * 4096);
    if (!rc && want_status) rc = d_status.need_pow2(count, 4096);
    if (rc) return rc;
    TrajRigid e;
    std::memcpy(e.m, E, sizeof(e.m));
    hipLaunchKernelGGL(traj_register_kernel, dim3(blocks_of(count, TB)), dim3(TB), 0, stream, d_times.p, d_knots.p, d_der.p, (uint32_t)n, in,
                       (uint32_t)count, prm.extrapolate, e, prm.frame == LV_TRAJ_FRAME_AT ? d_F.p : nullptr, tile ? 1 : 0,
                       want_out ? d_out.p : nullptr, want_status ? d_status.p : nullptr, counters.d.p);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int TrajStore::end_register(hipStream_t stream, uint64_t stats[4]) {
    const int rc = counters.read(stream, info.last_register);
    if (rc) return rc;
    if (stats)
        for (int k = 0; k < 4; ++k) stats[k] = info.last_register[k];
    return LV_OK;
}

int TrajStore::register_host(hipStream_t stream, const lv_traj_register_params& prm, const void* pts, size_t stride, size_t time_offset,
                             size_t count, float* out, uint8_t* status, uint64_t stats[4]) {
    double E[12];
    int rc = begin_register(stream, prm, E);
    if (rc) return rc;
    const char* base = static_cast<const char*>(pts);
    for (size_t off = 0; off < count; off += TRAJ_CHUNK) {
        const size_t c = std::min(TRAJ_CHUNK, count - off);
        LV_HIP(hipStreamSynchronize(stream));   // the piece before has left the pinned buffers
        rc = h_xyz.need_pow2(3 * c, 3 * 4096);
        if (!rc) rc = h_t.need_pow2(c, 4096);
        if (!rc) rc = d_xyz.need_pow2(3 * c, 3 * 4096);
        if (!rc) rc = d_t.need_pow2(c, 4096);
        if (rc) return rc;
        for (size_t k = 0; k < c; ++k) {   // (offsets need not be aligned)
            const char* rec = base + (off + k) * stride;
            std::memcpy(h_xyz.p + 3 * k, rec, 3 * sizeof(float));
            std::memcpy(h_t.p + k, rec + time_offset, sizeof(double));
        }
        LV_HIP(hipMemcpyAsync(d_xyz.p, h_xyz.p, 3 * c * sizeof(float), hipMemcpyHostToDevice, stream));
        LV_HIP(hipMemcpyAsync(d_t.p, h_t.p, c * sizeof(double), hipMemcpyHostToDevice, stream));
        const TrajPoints in{d_xyz.p, d_t.p, 3u, 1u};
        rc = launch_register(stream, prm, E, in, c, out != nullptr, status != nullptr);
        if (rc) return rc;
        if (out) LV_HIP(hipMemcpyAsync(out + 3 * off, d_out.p, 3 * c * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (status) LV_HIP(hipMemcpyAsync(status + off, d_status.p, c, hipMemcpyDeviceToHost, stream));
    }
    return end_register(stream, stats);
}

int TrajStore::register_device(hipStream_t stream, const lv_traj_register_params& prm, const TrajPoints& in, size_t count, float* out,
                               uint8_t* status, uint64_t stats[4]) {
    double E[12];
    int rc = begin_register(stream, prm, E);
    if (rc) return rc;
    for (size_t off = 0; off < count; off += TRAJ_CHUNK) {
        const size_t c = std::min(TRAJ_CHUNK, count - off);
        LV_HIP(hipStreamSynchronize(stream));   // (d_out / d_status of the piece before have been read)
        const TrajPoints piece{in.xyz + off * in.xyz_stride, in.times + off * in.time_stride, in.xyz_stride, in.time_stride};
        rc = launch_register(stream, prm, E, piece, c, out != nullptr, status != nullptr);
        if (rc) return rc;
        if (out) LV_HIP(hipMemcpyAsync(out + 3 * off, d_out.p, 3 * c * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (status) LV_HIP(hipMemcpyAsync(status + off, d_status.p, c, hipMemcpyDeviceToHost, stream));
    }
    return end_register(stream, stats);
}

void TrajStore::release() {
    release_all(d_knots, d_next, d_corr, d_der, d_cder, d_times, d_ctimes, d_fixed, h_xyz, h_t, d_xyz, d_out, d_t, d_F, d_status, d_poses,
                counters);
    const bool keep_tile = tile;
    *this = TrajStore();
    tile = keep_tile;
}

}  // namespace lv
