// lv_ndt.hip — NDT scan registration (include/limovelo_hip.h "NDT registration"; the rule's code is lv_ndt.hpp).
//
// Plain stream launches, no captured graphs, no grid-wide barriers or spins, no float atomics.
//   ndt_moments_kernel   one lane per source point (a map id tested with pt_alive as lv_elevation.hip does, or a staged caller
//                        point): ndt_point, then integer atomics into n, S1 and S2 of its voxel.  Integer sums commute: the
//                        moments do not depend on the order of the points or of the lanes.
//   ndt_gauss_kernel     one lane per voxel: ndt_gaussian into MEAN, COV and ICOV; the voxel counts are folded per wavefront.
//   ndt_eval_kernel, ndt_turn_kernel   the evaluation and the turn of lv_ndt_align: the bodies are lv_align.hpp's (align_eval,
//                        align_turn_body) over NdtRule, the host driver is its align_run.
#include "lv_ndt.hpp"

#include "lv_host.hpp"

namespace lv {

namespace {

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

// grid (chunks, K).  part: ALIGN_PART doubles per (hypothesis, chunk)
__global__ __launch_bounds__(ALIGN_NB) void ndt_eval_kernel(NdtRule q, const float* __restrict__ src, uint32_t n_src, uint32_t n_chunks,
                                                            const lv_ndt_result* __restrict__ res, const AlignHyp* __restrict__ hyp,
                                                            double* __restrict__ part) {
    align_eval(q, src, n_src, n_chunks, res, hyp, part);
}

// one workgroup per hypothesis
__global__ __launch_bounds__(ALIGN_NT) void ndt_turn_kernel(NdtRule q, int first, const double* __restrict__ part, uint32_t n_chunks,
                                                            lv_ndt_result* __restrict__ res, AlignHyp* __restrict__ hyp, uint32_t* running) {
    align_turn_body(q, first, part, n_chunks, res, hyp, running);
}

}  // namespace

void NdtStore::release() {
    release_all(d_n, d_S1, d_S2, d_mean, d_cov, d_icov, stats, pts, loop);
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
    const NdtRule q = ndt_rule_of(prm, NdtView{grid, d_mean.p, d_icov.p});
    return align_run(stream, loop, q, ndt_eval_kernel, ndt_turn_kernel, points, stride, n_src, guesses, K, results, best, "lv_ndt_align");
}

}  // namespace lv
