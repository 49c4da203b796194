// lv_ndt.hip — NDT scan registration (include/limovelo_hip.h "NDT registration"; the rule's code is lv_ndt.hpp).
//
// Plain stream launches, no captured graphs, no grid-wide barriers or spins, no float atomics.
//   ndt_moments_kernel   one lane per source point (a map id tested with pt_alive as lv_elevation.hip does, or a staged caller
//                        point): ndt_point, then integer atomics into n, S1 and S2 of its voxel.  Integer sums commute: the
//                        moments do not depend on the order of the points or of the lanes.
//   ndt_gauss_kernel     one lane per voxel: ndt_gaussian into MEAN, COV and ICOV; the voxel counts are folded per wavefront.
//   ndt_eval_kernel      one workgroup of 256 lanes per (chunk of NDT_CHUNK source points, hypothesis): lane l takes the points
//                        l, l + 256, ... of the chunk in ascending order into 28 f64 accumulators and a count; the wavefronts fold
//                        by an xor-butterfly (a + b == b + a: every lane holds the same bits), the four of them add in order, and
//                        the workgroup writes one partial of NDT_PART doubles.  The chunk is a constant of the header: the sums
//                        do not depend on the chip.
//   ndt_turn_kernel      one workgroup per hypothesis: its four wavefronts stage the partials in LDS, 64 chunks at a time; the first
//                        wavefront adds them, lane a < 29 its entry in chunk order, then lane 0 runs ndt_turn (acceptance,
//                        lambda, the damped 6 x 6 solve, the trial pose).  A hypothesis that finishes
//                        lowers the count of running ones (an integer atomic); the host enqueues NDT_ITER_CHUNK iterations
//                        between two looks at that count, and the workgroups of a finished hypothesis return at once.
#include "lv_ndt.hpp"

#include <algorithm>
#include <cstring>

#include "lv_host.hpp"

namespace lv {

namespace {

constexpr int NB = 256;   // lanes per workgroup of the evaluation
constexpr int NT = 256;   // lanes per workgroup of the turn
constexpr int NT_TILE = 64;   // partials staged in LDS at a time

template <bool MAP>
__device__ __forceinline__ bool ndt_source(const void* __restrict__ src, uint32_t i, float p[3]) {
    if (MAP) {
        const float4 q = static_cast<const float4*>(src)[i];
        if (!pt_alive(q)) return false;
        p[0] = q.x;
        p[1] = q.y;
        p[2] = q.z;
    } else {
        const float* q = static_cast<const float*>(src) + 3 * (size_t)i;
        p[0] = q[0];
        p[1] = q[1];
        p[2] = q[2];
    }
    return true;
}

// stats[0] += used points, stats[1] += ignored points
template <bool MAP>
__global__ __launch_bounds__(256) void ndt_moments_kernel(const void* __restrict__ src, uint32_t n, NdtGrid g, uint32_t* __restrict__ cnt,
                                                          unsigned long long* __restrict__ S1, unsigned long long* __restrict__ S2,
                                                          unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t used = 0, ign = 0;
    float p[3];
    if (i < n && ndt_source<MAP>(src, i, p)) {
        uint32_t cell;
        int32_t c[3], r[3];
        if (ndt_point(g, p, cell, c, r)) {
            used = 1;
            atomicAdd(cnt + cell, 1u);
            int k = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicAdd(S1 + (size_t)cell * 3 + a, (unsigned long long)r[a]);
#pragma unroll
                for (int b = a; b < 3; ++b, ++k) atomicAdd(S2 + (size_t)cell * 6 + k, (unsigned long long)(r[a] * r[b]));
            }
        } else {
            ign = 1;
        }
    }
    wave_add_to(stats + 0, used);
    wave_add_to(stats + 1, ign);
}

// stats[2] = used voxels, stats[3] = occupied voxels below min_points (both zeroed before the launch)
__global__ __launch_bounds__(256) void ndt_gauss_kernel(NdtGrid g, uint32_t n_cells, const uint32_t* __restrict__ cnt,
                                                        const unsigned long long* __restrict__ S1, const unsigned long long* __restrict__ S2,
                                                        double* __restrict__ mean, double* __restrict__ cov, double* __restrict__ icov,
                                                        unsigned long long* stats) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t used = 0, sparse = 0;
    if (cell < n_cells) {
        int c[3];
        grid_ijk(g, cell, c[0], c[1], c[2]);
        const uint32_t n = cnt[cell];
        long long s1[3], s2[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) s1[k] = (long long)S1[(size_t)cell * 3 + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) s2[k] = (long long)S2[(size_t)cell * 6 + k];
        double m[3], C[6], O[6];
        used = ndt_gaussian(g, c, n, s1, s2, m, C, O) ? 1u : 0u;
        sparse = (!used && n > 0) ? 1u : 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) mean[(size_t)cell * 3 + k] = m[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            cov[(size_t)cell * 6 + k] = C[k];
            icov[(size_t)cell * 6 + k] = O[k];
        }
    }
    wave_add_to(stats + 2, used);
    wave_add_to(stats + 3, sparse);
}

// grid (chunks, K).  part: NDT_PART doubles per (hypothesis, chunk)
__global__ __launch_bounds__(NB) void ndt_eval_kernel(NdtView v, const float* __restrict__ src, uint32_t n_src, uint32_t n_chunks,
                                                      const lv_ndt_result* __restrict__ res, const NdtHyp* __restrict__ hyp, int search, double hd,
                                                      double* __restrict__ part) {
    __shared__ double sh[NB / 64][NDT_ACC + 1];
    const uint32_t h = blockIdx.y, chunk = blockIdx.x;
    if (res[h].status != NDT_RUNNING) return;   // (uniform over the workgroup)
    const lv_graph_pose x = hyp[h].trial;
    double R[9];
    gr_rot(x.q, R);
    double acc[NDT_ACC];
#pragma unroll
    for (int a = 0; a < NDT_ACC; ++a) acc[a] = 0.0;
    uint32_t cnt = 0;
    const uint32_t end = min(n_src, (chunk + 1) * NDT_CHUNK);
    for (uint32_t i = chunk * NDT_CHUNK + threadIdx.x; i < end; i += NB) {
        const float p[3] = {src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]};
        cnt += ndt_point_terms(v, R, x.t, p, search, hd, acc) ? 1u : 0u;
    }
#pragma unroll
    for (int a = 0; a < NDT_ACC; ++a) acc[a] = wave_sum(acc[a]);
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < NDT_ACC; ++a) sh[threadIdx.x >> 6][a] = acc[a];
        sh[threadIdx.x >> 6][NDT_ACC] = (double)cnt;   // (at most NDT_CHUNK: exact)
    }
    __syncthreads();
    if (threadIdx.x <= NDT_ACC) {
        double t = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NB / 64; ++w) t = t + sh[w][threadIdx.x];
        part[((size_t)h * n_chunks + chunk) * NDT_PART + threadIdx.x] = t;
    }
}

// One workgroup per hypothesis.  All four wavefronts stage the partials in LDS, NT_TILE chunks at a time (coalesced, the loads of a
// tile in flight together: one lane adding straight from global memory waits for every load in turn); the first wavefront then
// adds each entry in chunk order and its lane 0 runs the turn.
__global__ __launch_bounds__(NT) void ndt_turn_kernel(lv_ndt_align_params prm, int first, const double* __restrict__ part, uint32_t n_chunks,
                                                      lv_ndt_result* __restrict__ res, NdtHyp* __restrict__ hyp, uint32_t* running) {
    __shared__ double tile[NT_TILE][NDT_PART];
    __shared__ double tot[NDT_PART];
    const uint32_t h = blockIdx.x;
    if (res[h].status != NDT_RUNNING) return;   // (uniform over the workgroup)
    const double* p = part + (size_t)h * n_chunks * NDT_PART;
    const uint32_t a = threadIdx.x % NDT_PART, row = threadIdx.x / NDT_PART;
    double t = 0.0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += NT_TILE) {
        const uint32_t m = min((uint32_t)NT_TILE, n_chunks - c0);
        for (uint32_t c = row; c < m; c += NT / NDT_PART) tile[c][a] = p[(size_t)(c0 + c) * NDT_PART + a];
        __syncthreads();
        if (threadIdx.x <= NDT_ACC)
            for (uint32_t c = 0; c < m; ++c) t = t + tile[c][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x <= NDT_ACC) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        lv_ndt_result r = res[h];
        NdtHyp y = hyp[h];
        const bool done = ndt_turn(prm, first != 0, tot, (uint32_t)tot[NDT_ACC], r, y);
        res[h] = r;
        hyp[h] = y;
        if (done) atomicSub(running, 1u);
    }
}

}  // namespace

void NdtStore::release() {
    release_all(d_n, d_S1, d_S2, d_mean, d_cov, d_icov, stats, pts, src, d_res, h_res, d_hyp, h_hyp, d_part, d_running, h_running);
    *this = NdtStore();
}

// p: the parameters of a build; NULL: an add to the target held
int NdtStore::build(hipStream_t stream, const lv_ndt_params* p, const float4* map_orig, uint32_t n_ids, const void* points, size_t stride, size_t n,
                    uint64_t out[4]) {
    const bool from = points == nullptr, fresh = p != nullptr;
    const NdtGrid g = fresh ? ndt_grid_of(*p) : grid;
    const size_t nc = grid_cells(g);
    int rc = pts.reserve(stream, from ? 0 : n);   // (synchronises the stream)
    if (fresh) {
        built = false;   // (before a buffer goes, and until the kernels are through)
        if (!rc) rc = d_n.need(nc);
        if (!rc) rc = d_S1.need(nc * 3);
        if (!rc) rc = d_S2.need(nc * 6);
        if (!rc) rc = d_mean.need(nc * 3);
        if (!rc) rc = d_cov.need(nc * 6);
        if (!rc) rc = d_icov.need(nc * 6);
    }
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    if (!from) {
        pts.append(points, stride, n);
        rc = pts.upload(stream);
        if (rc) return rc;
    }
    if (fresh) {
        LV_HIP(hipMemsetAsync(d_n.p, 0, nc * sizeof(uint32_t), stream));
        LV_HIP(hipMemsetAsync(d_S1.p, 0, nc * 3 * sizeof(unsigned long long), stream));
        LV_HIP(hipMemsetAsync(d_S2.p, 0, nc * 6 * sizeof(unsigned long long), stream));
    }
    const uint32_t ns = from ? n_ids : (uint32_t)n;
    if (ns) {
        if (from) hipLaunchKernelGGL(ndt_moments_kernel<true>, dim3(blocks_of(ns)), dim3(256), 0, stream, map_orig, ns, g, d_n.p, d_S1.p, d_S2.p, stats.d.p);
        else hipLaunchKernelGGL(ndt_moments_kernel<false>, dim3(blocks_of(ns)), dim3(256), 0, stream, pts.d.p, ns, g, d_n.p, d_S1.p, d_S2.p, stats.d.p);
        LV_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ndt_gauss_kernel, dim3(blocks_of(nc)), dim3(256), 0, stream, g, (uint32_t)nc, d_n.p, d_S1.p, d_S2.p, d_mean.p, d_cov.p, d_icov.p,
                       stats.d.p);
    LV_HIP(hipGetLastError());
    uint64_t st[4];
    rc = stats.read(stream, st);
    if (rc) return rc;
    if (fresh) {
        info = lv_ndt_target_info{};
        info.params = *p;
        grid = g;
        n_cells = nc;
        n_given = 0;
    }
    info.built = 1;
    info.from_map = from ? 1 : 0;
    info.n_used += st[0];
    info.n_ignored += st[1];
    info.used_voxels = st[2];
    info.sparse_voxels = st[3];
    n_given += ns;
    if (out)
        for (int k = 0; k < 4; ++k) out[k] = st[k];
    built = true;
    return LV_OK;
}

int NdtStore::fetch(hipStream_t stream, int layer, void* out) {
    const void* from = nullptr;
    switch (layer) {
        case LV_NDT_COUNT: from = d_n.p; break;
        case LV_NDT_S1: from = d_S1.p; break;
        case LV_NDT_S2: from = d_S2.p; break;
        case LV_NDT_MEAN: from = d_mean.p; break;
        case LV_NDT_COV: from = d_cov.p; break;
        default: from = d_icov.p; break;
    }
    LV_HIP(hipMemcpyAsync(out, from, n_cells * ndt_layer_width(layer) * ndt_layer_elem(layer), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int NdtStore::align(hipStream_t stream, const lv_ndt_align_params& prm, const void* points, size_t stride, size_t n_src, const lv_graph_pose* guesses,
                    size_t K, lv_ndt_result* results, int32_t best[2]) {
    if (K == 0) {
        best[0] = best[1] = -1;
        return LV_OK;
    }
    const uint32_t n_chunks = blocks_of(n_src, NDT_CHUNK);
    int rc = src.reserve(stream, n_src, 3 * 4096);   // (synchronises the stream: the pinned records below are free)
    if (!rc) rc = d_res.need_pow2(K, 64);
    if (!rc) rc = h_res.need_pow2(K, 64);
    if (!rc) rc = d_hyp.need_pow2(K, 64);
    if (!rc) rc = h_hyp.need_pow2(K, 64);
    if (!rc) rc = d_part.need_pow2(std::max<size_t>((size_t)K * n_chunks * NDT_PART, 1), 64 * NDT_PART);
    if (!rc) rc = d_running.need(1);
    if (!rc) rc = h_running.need(2);
    if (rc) return rc;
    // the records as the loop starts them
    for (size_t k = 0; k < K; ++k) {
        lv_ndt_result r{};
        r.pose = guesses[k];
        r.lambda = prm.lambda_init;
        r.status = n_src ? NDT_RUNNING : LV_NDT_NO_OVERLAP;
        h_res.p[k] = r;
        NdtHyp y{};
        y.trial = guesses[k];   // the first evaluation stands at the guess
        h_hyp.p[k] = y;
    }
    if (n_src == 0) {   // nothing to evaluate: every guess comes back as it is
        std::memcpy(results, h_res.p, K * sizeof(lv_ndt_result));
        ndt_best(results, K, best);
        return LV_OK;
    }
    src.append(points, stride, n_src);
    rc = src.upload(stream);
    if (rc) return rc;
    h_running.p[1] = (uint32_t)K;
    LV_HIP(hipMemcpyAsync(d_res.p, h_res.p, K * sizeof(lv_ndt_result), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_running.p, h_running.p + 1, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_hyp.p, h_hyp.p, K * sizeof(NdtHyp), hipMemcpyHostToDevice, stream));
    const NdtView view{grid, d_mean.p, d_icov.p};
    const double hd = -0.5 * prm.d2;
    const dim3 eg(n_chunks, (uint32_t)K);
    for (int it = 0; it <= prm.max_iterations;) {
        const int end = std::min(prm.max_iterations + 1, it + NDT_ITER_CHUNK);
        for (; it < end; ++it) {
            hipLaunchKernelGGL(ndt_eval_kernel, eg, dim3(NB), 0, stream, view, src.d.p, (uint32_t)n_src, n_chunks, d_res.p, d_hyp.p, prm.search, hd,
                               d_part.p);
            LV_HIP(hipGetLastError());
            hipLaunchKernelGGL(ndt_turn_kernel, dim3((uint32_t)K), dim3(NT), 0, stream, prm, it == 0 ? 1 : 0, d_part.p, n_chunks, d_res.p, d_hyp.p,
                               d_running.p);
            LV_HIP(hipGetLastError());
        }
        LV_HIP(hipMemcpyAsync(h_running.p, d_running.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        if (h_running.p[0] == 0) break;
    }
    LV_HIP(hipMemcpyAsync(h_res.p, d_res.p, K * sizeof(lv_ndt_result), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    if (h_running.p[0] != 0) { set_error("lv_ndt_align: %u hypotheses did not finish", h_running.p[0]); return LV_EHIP; }
    std::memcpy(results, h_res.p, K * sizeof(lv_ndt_result));
    ndt_best(results, K, best);
    return LV_OK;
}

}  // namespace lv
