// lv_surf_align.hip — registration against the TSDF surface (include/limovelo_hip.h "Surface registration"; the rule's code is
// lv_surf_align.hpp).
//
// Plain stream launches, no captured graphs, no grid-wide barriers or spins, no float atomics.  The kernels read S and W of the
// live volume and write the scratch of TsdfStore::align alone.
//   surf_sample_kernel      one lane per point: surf_sample at (double)p.
//   surf_align_eval_kernel  one workgroup of 256 lanes per (chunk of SURF_ALIGN_CHUNK source points, hypothesis): lane l takes the
//                           points l and l + 256 of the chunk in ascending order, for each the 8 gathers of W and of S and the
//                           trilinear algebra, into 28 f64 accumulators and a count in registers; the wavefronts fold by an
//                           xor-butterfly (a + b == b + a: every lane holds the same bits), the four of them add in order through
//                           LDS, and the workgroup writes one partial of SURF_PART doubles.  The chunk is a constant of the header:
//                           the sums do not depend on the chip.
//   surf_align_turn_kernel  one workgroup per hypothesis: its four wavefronts stage the partials in LDS, 64 chunks at a time; the
//                           first wavefront adds them, lane a < 29 its entry in chunk order, then lane 0 runs surf_turn.  A
//                           hypothesis that finishes lowers the count of running ones (an integer atomic); the host enqueues
//                           SURF_ITER_CHUNK turns between two looks at that count, and the workgroups of a finished hypothesis
//                           return at once.
#include "lv_surf_align.hpp"

#include <algorithm>
#include <cstring>

#include "lv_host.hpp"

namespace lv {

namespace {

constexpr int NB = 256;        // lanes per workgroup of the evaluation
constexpr int NT = 256;        // lanes per workgroup of the turn
constexpr int NT_TILE = 64;    // partials staged in LDS at a time

__global__ __launch_bounds__(256) void surf_sample_kernel(SurfView v, const float* __restrict__ pts, uint32_t n, double* __restrict__ out,
                                                          uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x[3] = {(double)pts[3 * (size_t)i], (double)pts[3 * (size_t)i + 1], (double)pts[3 * (size_t)i + 2]};
    double d, g[3];
    const int s = surf_sample(v, x, d, g);
    if (out) {
        out[4 * (size_t)i] = d;
        out[4 * (size_t)i + 1] = g[0];
        out[4 * (size_t)i + 2] = g[1];
        out[4 * (size_t)i + 3] = g[2];
    }
    if (status) status[i] = (uint8_t)s;
}

// grid (chunks, K).  part: SURF_PART doubles per (hypothesis, chunk)
__global__ __launch_bounds__(NB) void surf_align_eval_kernel(SurfView v, const float* __restrict__ src, uint32_t n_src, uint32_t n_chunks,
                                                             const lv_surf_align_result* __restrict__ res, const NdtHyp* __restrict__ hyp,
                                                             double max_dist, double huber, double* __restrict__ part) {
    __shared__ double sh[NB / 64][SURF_ACC + 1];
    const uint32_t h = blockIdx.y, chunk = blockIdx.x;
    if (res[h].status != SURF_RUNNING) return;   // (uniform over the workgroup)
    const lv_graph_pose x = hyp[h].trial;
    double R[9];
    gr_rot(x.q, R);
    double acc[SURF_ACC];
#pragma unroll
    for (int a = 0; a < SURF_ACC; ++a) acc[a] = 0.0;
    uint32_t cnt = 0;
    const uint32_t end = min(n_src, (chunk + 1) * SURF_ALIGN_CHUNK);
    for (uint32_t i = chunk * SURF_ALIGN_CHUNK + threadIdx.x; i < end; i += NB) {
        const float p[3] = {src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]};
        cnt += surf_point_terms(v, R, x.t, p, max_dist, huber, acc) ? 1u : 0u;
    }
#pragma unroll
    for (int a = 0; a < SURF_ACC; ++a) acc[a] = wave_sum(acc[a]);
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < SURF_ACC; ++a) sh[threadIdx.x >> 6][a] = acc[a];
        sh[threadIdx.x >> 6][SURF_ACC] = (double)cnt;   // (at most SURF_ALIGN_CHUNK: exact)
    }
    __syncthreads();
    if (threadIdx.x <= SURF_ACC) {
        double t = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NB / 64; ++w) t = t + sh[w][threadIdx.x];
        part[((size_t)h * n_chunks + chunk) * SURF_PART + threadIdx.x] = t;
    }
}

// One workgroup per hypothesis.  All four wavefronts stage the partials in LDS, NT_TILE chunks at a time (coalesced, the loads of a
// tile in flight together); the first wavefront then adds each entry in chunk order and its lane 0 runs the turn.
__global__ __launch_bounds__(NT) void surf_align_turn_kernel(lv_surf_align_params prm, uint32_t n_src, int first, const double* __restrict__ part,
                                                             uint32_t n_chunks, lv_surf_align_result* __restrict__ res, NdtHyp* __restrict__ hyp,
                                                             uint32_t* running) {
    __shared__ double tile[NT_TILE][SURF_PART];
    __shared__ double tot[SURF_PART];
    const uint32_t h = blockIdx.x;
    if (res[h].status != SURF_RUNNING) return;   // (uniform over the workgroup)
    const double* p = part + (size_t)h * n_chunks * SURF_PART;
    const uint32_t a = threadIdx.x % SURF_PART, row = threadIdx.x / SURF_PART;
    double t = 0.0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NT_TILE) {
        const uint32_t m = min((uint32_t)NT_TILE, n_chunks - c0);
        for (uint32_t c = row; c < m; c += NT / SURF_PART) tile[c][a] = p[(size_t)(c0 + c) * SURF_PART + a];
        __syncthreads();
        if (threadIdx.x <= SURF_ACC)
            for (uint32_t c = 0; c < m; ++c) t = t + tile[c][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x <= SURF_ACC) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        lv_surf_align_result r = res[h];
        NdtHyp y = hyp[h];
        const bool done = surf_turn(prm, n_src, first != 0, tot, (uint32_t)tot[SURF_ACC], r, y);
        res[h] = r;
        hyp[h] = y;
        if (done) atomicSub(running, 1u);
    }
}

}  // namespace

int TsdfStore::surf_sample(hipStream_t stream, int min_weight, const void* pts, size_t stride, size_t n, double* out, uint8_t* status) {
    if (n == 0) return LV_OK;
    int rc = align.pts.reserve(stream, n);   // (synchronises the stream)
    if (!rc && out) rc = align.d_out.need(4 * n);
    if (!rc && status) rc = align.d_status.need(n);
    if (rc) return rc;
    align.pts.append(pts, stride, n);
    rc = align.pts.upload(stream);
    if (rc) return rc;
    const SurfView view = surf_view_of(grid, min_weight, d_S.p, d_W.p);
    hipLaunchKernelGGL(surf_sample_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, view, align.pts.d.p, (uint32_t)n, out ? align.d_out.p : nullptr,
                       status ? align.d_status.p : nullptr);
    LV_HIP(hipGetLastError());
    if (out) LV_HIP(hipMemcpyAsync(out, align.d_out.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (status) LV_HIP(hipMemcpyAsync(status, align.d_status.p, n, hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::surf_align(hipStream_t stream, const lv_surf_align_params& prm, const void* points, size_t stride, size_t n_src,
                          const lv_graph_pose* guesses, size_t K, lv_surf_align_result* results, int32_t best[2]) {
    if (K == 0) {
        best[0] = best[1] = -1;
        return LV_OK;
    }
    SurfAlignStage& s = align;
    const uint32_t n_chunks = blocks_of(n_src, SURF_ALIGN_CHUNK);
    int rc = s.pts.reserve(stream, n_src, 3 * 4096);   // (synchronises the stream: the pinned records below are free)
    if (!rc) rc = s.d_res.need_pow2(K, 64);
    if (!rc) rc = s.h_res.need_pow2(K, 64);
    if (!rc) rc = s.d_hyp.need_pow2(K, 64);
    if (!rc) rc = s.h_hyp.need_pow2(K, 64);
    if (!rc) rc = s.d_part.need_pow2(std::max<size_t>((size_t)K * n_chunks * SURF_PART, 1), 64 * SURF_PART);
    if (!rc) rc = s.d_running.need(1);
    if (!rc) rc = s.h_running.need(2);
    if (rc) return rc;
    // the records as the loop starts them
    for (size_t k = 0; k < K; ++k) {
        lv_surf_align_result r{};
        r.pose = guesses[k];
        r.lambda = prm.lambda_init;
        r.status = n_src ? SURF_RUNNING : LV_SURF_ALIGN_NO_OVERLAP;
        s.h_res.p[k] = r;
        NdtHyp y{};
        y.trial = guesses[k];   // the first evaluation stands at the guess
        s.h_hyp.p[k] = y;
    }
    if (n_src == 0) {   // nothing to evaluate: every guess comes back as it is
        std::memcpy(results, s.h_res.p, K * sizeof(lv_surf_align_result));
        surf_align_best(results, K, best);
        return LV_OK;
    }
    s.pts.append(points, stride, n_src);
    rc = s.pts.upload(stream);
    if (rc) return rc;
    s.h_running.p[1] = (uint32_t)K;
    LV_HIP(hipMemcpyAsync(s.d_res.p, s.h_res.p, K * sizeof(lv_surf_align_result), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(s.d_running.p, s.h_running.p + 1, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(s.d_hyp.p, s.h_hyp.p, K * sizeof(NdtHyp), hipMemcpyHostToDevice, stream));
    const SurfView view = surf_view_of(grid, prm.min_weight, d_S.p, d_W.p);
    const dim3 eg(n_chunks, (uint32_t)K);
    for (int it = 0; it <= prm.max_iterations;) {
        const int end = std::min(prm.max_iterations + 1, it + SURF_ITER_CHUNK);
        for (; it < end; ++it) {
            hipLaunchKernelGGL(surf_align_eval_kernel, eg, dim3(NB), 0, stream, view, s.pts.d.p, (uint32_t)n_src, n_chunks, s.d_res.p, s.d_hyp.p,
                               prm.max_dist, prm.huber, s.d_part.p);
            LV_HIP(hipGetLastError());
            hipLaunchKernelGGL(surf_align_turn_kernel, dim3((uint32_t)K), dim3(NT), 0, stream, prm, (uint32_t)n_src, it == 0 ? 1 : 0, s.d_part.p, n_chunks,
                               s.d_res.p, s.d_hyp.p, s.d_running.p);
            LV_HIP(hipGetLastError());
        }
        LV_HIP(hipMemcpyAsync(s.h_running.p, s.d_running.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        if (s.h_running.p[0] == 0) break;
    }
    LV_HIP(hipMemcpyAsync(s.h_res.p, s.d_res.p, K * sizeof(lv_surf_align_result), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    if (s.h_running.p[0] != 0) { set_error("lv_surf_align: %u hypotheses did not finish", s.h_running.p[0]); return LV_EHIP; }
    std::memcpy(results, s.h_res.p, K * sizeof(lv_surf_align_result));
    surf_align_best(results, K, best);
    return LV_OK;
}

}  // namespace lv
