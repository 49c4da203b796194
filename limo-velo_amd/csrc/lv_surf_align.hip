// lv_surf_align.hip — registration against the TSDF surface (include/limovelo_hip.h "Surface registration"; the rule's code is
// lv_surf_align.hpp).
//
// Plain stream launches, no captured graphs, no grid-wide barriers or spins, no float atomics.  The kernels read S and W of the
// live volume and write the scratch of TsdfStore::align (a SurfAlignStage) alone.
//   surf_sample_kernel      one lane per point: surf_sample at (double)p.
//   surf_align_eval_kernel, surf_align_turn_kernel   the evaluation and the turn of lv_surf_align: the bodies are lv_align.hpp's
//                           (align_eval, align_turn_body) over SurfAlignRule, the host driver is its align_run.  Per source point the 8
//                           gathers of W and of S and the trilinear algebra; a lane takes the points l and l + 256 of its chunk.
#include "lv_surf_align.hpp"

#include "lv_host.hpp"

namespace lv {

namespace {

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

// grid (chunks, K).  part: ALIGN_PART doubles per (hypothesis, chunk)
__global__ __launch_bounds__(ALIGN_NB) void surf_align_eval_kernel(SurfAlignRule q, const float* __restrict__ src, uint32_t n_src, uint32_t n_chunks,
                                                                   const lv_surf_align_result* __restrict__ res, const AlignHyp* __restrict__ hyp,
                                                                   double* __restrict__ part) {
    align_eval(q, src, n_src, n_chunks, res, hyp, part);
}

// one workgroup per hypothesis
__global__ __launch_bounds__(ALIGN_NT) void surf_align_turn_kernel(SurfAlignRule q, int first, const double* __restrict__ part, uint32_t n_chunks,
                                                                   lv_surf_align_result* __restrict__ res, AlignHyp* __restrict__ hyp,
                                                                   uint32_t* running) {
    align_turn_body(q, first, part, n_chunks, res, hyp, running);
}

}  // namespace

int TsdfStore::surf_sample(hipStream_t stream, int min_weight, const void* pts, size_t stride, size_t n, double* out, uint8_t* status) {
    if (n == 0) return LV_OK;
    int rc = align.loop.src.reserve(stream, n);   // (synchronises the stream)
    if (!rc && out) rc = align.d_out.need(4 * n);
    if (!rc && status) rc = align.d_status.need(n);
    if (rc) return rc;
    align.loop.src.append(pts, stride, n);
    rc = align.loop.src.upload(stream);
    if (rc) return rc;
    const SurfView view = surf_view_of(grid, min_weight, d_S.p, d_W.p);
    hipLaunchKernelGGL(surf_sample_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, view, align.loop.src.d.p, (uint32_t)n, out ? align.d_out.p : nullptr,
                       status ? align.d_status.p : nullptr);
    LV_HIP(hipGetLastError());
    if (out) LV_HIP(hipMemcpyAsync(out, align.d_out.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (status) LV_HIP(hipMemcpyAsync(status, align.d_status.p, n, hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int TsdfStore::surf_align(hipStream_t stream, const lv_surf_align_params& prm, const void* points, size_t stride, size_t n_src,
                          const lv_graph_pose* guesses, size_t K, lv_surf_align_result* results, int32_t best[2]) {
    const SurfAlignRule q = surf_align_rule_of(prm, surf_view_of(grid, prm.min_weight, d_S.p, d_W.p), (uint32_t)n_src);
    return align_run(stream, align.loop, q, surf_align_eval_kernel, surf_align_turn_kernel, points, stride, n_src, guesses, K, results, best,
                     "lv_surf_align");
}

}  // namespace lv
