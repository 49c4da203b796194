// lv_align.hpp — the Levenberg-Marquardt loop that NDT registration (lv_ndt.hpp) and surface registration (lv_surf_align.hpp)
// share: K hypotheses, each on its own, over sums of 28 f64 terms taken in one written order (include/limovelo_hip.h "NDT
// registration", "Surface registration": the order is part of both contracts).
//
// A method is a RULE, a plain struct passed by value to the templates below (NdtRule, SurfAlignRule).  It holds
//   using Result                      lv_ndt_result / lv_surf_align_result: the same layout, the objective under another name
//   AlignLoop loop                    the scalars of the loop
//   point_terms(R, t, p, acc)         what source point p adds to acc (ALIGN_ACC sums) at the pose (R, t); true: it counts in n_in
//   objective(tot, n_in)              the objective of an evaluation from its sums
//   objective_of(res)                 the member of Result that holds it
//   accept(new, old)                  whether a trial's objective is taken; better(a, b) whether result a beats result b
// A further registration target needs its point_terms and such a struct, nothing else.
//
// The first part is plain __host__ __device__ code: the constants, the order of the 21 entries of H, the damped solve, one turn of
// the loop, the loop on the host (align_evaluate, align_one: what the emus of tests/emu and the host programs of scripts run),
// `best` and the argument rules.  The second part (hipcc only) is the two kernel bodies and the host driver:
//   align_eval   one workgroup of 256 lanes per (chunk of ALIGN_CHUNK source points, hypothesis): lane l takes the points l, l + 256,
//                ... of the chunk in ascending order into 28 f64 accumulators and a count in registers; the wavefronts fold by an
//                xor-butterfly (a + b == b + a: every lane holds the same bits), the four of them add in order through LDS, and the
//                workgroup writes one partial of ALIGN_PART doubles.  The chunk is a constant: the sums do not depend on the chip.
//   align_turn_body  one workgroup per hypothesis: its four wavefronts stage the partials in LDS, 64 chunks at a time; the first
//                wavefront adds them, lane a < 29 its entry in chunk order, then lane 0 runs align_turn.  A hypothesis that
//                finishes lowers the count of running ones (an integer atomic).
//   align_run    enqueues ALIGN_ITER_CHUNK evaluations and turns between two looks at that count; the workgroups of a finished
//                hypothesis return at once.
// The quaternion algebra, the retraction and the 6 x 6 Cholesky are lv_graph.hpp's.
#pragma once

#include <algorithm>

#include "../../include/limovelo_hip.h"
#include "lv_buffers.hpp"
#include "lv_graph.hpp"
#include "lv_grid.hpp"

namespace lv {

static_assert(LV_NDT_CHUNK == LV_SURF_ALIGN_CHUNK, "one chunk for every method: the sums are the same");
static_assert(LV_NDT_CONVERGED == LV_SURF_ALIGN_CONVERGED, "one loop: the status values agree");
static_assert(LV_NDT_MAX_ITERATIONS == LV_SURF_ALIGN_MAX_ITERATIONS, "one loop: the status values agree");
static_assert(LV_NDT_NO_OVERLAP == LV_SURF_ALIGN_NO_OVERLAP, "one loop: the status values agree");

constexpr uint32_t ALIGN_CHUNK = LV_NDT_CHUNK;   // source points per workgroup of the evaluation
constexpr int ALIGN_ACC = 28;                    // 21 of H, 6 of g, the method's sum (S, E)
constexpr int ALIGN_PART = 32;                   // doubles per workgroup partial: ALIGN_ACC, n_in, padding
constexpr int ALIGN_ITER_CHUNK = 8;              // iterations enqueued between two looks at the count of running hypotheses
constexpr int ALIGN_NB = 256;                    // lanes per workgroup of the evaluation
constexpr int ALIGN_NT = 256;                    // lanes per workgroup of the turn
constexpr int ALIGN_NT_TILE = 64;                // partials staged in LDS at a time
constexpr int32_t ALIGN_RUNNING = -1;            // a status of the loop, never returned
constexpr int32_t ALIGN_CONVERGED = LV_NDT_CONVERGED, ALIGN_MAX_ITERATIONS = LV_NDT_MAX_ITERATIONS, ALIGN_NO_OVERLAP = LV_NDT_NO_OVERLAP;

// the index of (a, b), a <= b, in the 21 entries of a 6 x 6 upper triangle
LV_OCC_HD constexpr int align_tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// d of (H + lambda diag H) d = -g (H: 21 entries, g: 6); returns the max-norm of d
LV_OCC_HD double align_solve(const double* H21, const double* g, double lambda, double* d) {
    double M[36], Mi[36];
    gr_info(H21, M);
    for (int a = 0; a < 6; ++a) M[a * 7] = M[a * 7] + lambda * M[a * 7];
    graph_block_inverse(M, Mi);
    double m = 0.0;
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s = s + Mi[a * 6 + k] * g[k];
        d[a] = -s;
        const double v = fabs(d[a]);
        m = v > m ? v : m;                       // (a NaN is caught by the finiteness test of the step, below)
        if (!(v - v == 0.0)) m = INFINITY;
    }
    return m;
}

// The scalars of the loop.  least_guess: the n_in below which a guess is NO_OVERLAP; least_trial: the n_in below which a trial is
// rejected.  NDT's pair is (1, 0): it puts no condition on a trial, and a trial with n_in = 0 and S = 0 IS accepted once the
// current score has underflowed to 0.  The surface's is (min_points, min_points).
struct AlignLoop {
    int32_t max_iterations;
    uint32_t least_guess, least_trial;
    uint32_t pad;
    double step_tol, lambda_init, lambda_min, lambda_max;
};

// What the loop keeps per hypothesis beside its result (whose pose, objective, info and n_in are the CURRENT ones)
struct AlignHyp {
    lv_graph_pose trial;   // where the next evaluation stands
    double g[6];           // the gradient at the current pose
    double step;           // max-norm of the increment that gave `trial`
    uint32_t iterations;   // accepted + rejected
    uint32_t pad;
};

// the records as the loop starts them: the first evaluation stands at the guess
template <class Result>
inline void align_start(const AlignLoop& loop, const lv_graph_pose& guess, int32_t status, Result& res, AlignHyp& h) {
    res = Result{};
    res.pose = guess;
    res.lambda = loop.lambda_init;
    res.status = status;
    h = AlignHyp{};
    h.trial = guess;
}

// One turn of the loop for one hypothesis, after an evaluation at h.trial gave tot (ALIGN_ACC sums) and n_in.  first: the
// evaluation stood at the guess.  Returns true when the hypothesis has just finished (res.status left ALIGN_RUNNING).
template <class Rule>
LV_OCC_HD bool align_turn(const Rule& q, bool first, const double* tot, uint32_t n_in, typename Rule::Result& res, AlignHyp& h) {
    const AlignLoop& prm = q.loop;
    const double obj = q.objective(tot, n_in);
    bool take = first;
    if (first) {
        if (n_in < prm.least_guess) {
            res.status = ALIGN_NO_OVERLAP;
            return true;
        }
    } else {
        const double step = h.step;
        if (step - step == 0.0 && n_in >= prm.least_trial && Rule::accept(obj, Rule::objective_of(res))) {
            take = true;
            res.accepted = res.accepted + 1;
            res.last_step = step;
            res.lambda = res.lambda / 3.0 > prm.lambda_min ? res.lambda / 3.0 : prm.lambda_min;
        } else {
            res.rejected = res.rejected + 1;
            res.lambda = 4.0 * res.lambda < prm.lambda_max ? 4.0 * res.lambda : prm.lambda_max;
        }
        h.iterations = h.iterations + 1;
    }
    if (take) {
        if (!first) res.pose = h.trial;
        for (int k = 0; k < 21; ++k) res.info[k] = tot[k];
        for (int k = 0; k < 6; ++k) h.g[k] = tot[21 + k];
        Rule::objective_of(res) = obj;
        res.n_in = n_in;
        if (!first && h.step <= prm.step_tol) {
            res.status = ALIGN_CONVERGED;
            return true;
        }
    }
    if (h.iterations >= (uint32_t)prm.max_iterations) {
        res.status = ALIGN_MAX_ITERATIONS;
        return true;
    }
    double d[6];
    h.step = align_solve(res.info, h.g, res.lambda, d);
    if (h.step - h.step == 0.0) graph_retract(res.pose, d, &h.trial);
    else h.trial = res.pose;   // (rejected at the next turn)
    return false;
}

// One evaluation on the host: the n points of src (packed x, y, z) in ascending order into one accumulator; returns n_in
template <class Rule>
inline uint32_t align_evaluate(const Rule& q, const float* src, size_t n, const lv_graph_pose& x, double* acc) {
    double R[9];
    gr_rot(x.q, R);
    for (int a = 0; a < ALIGN_ACC; ++a) acc[a] = 0.0;
    uint32_t n_in = 0;
    for (size_t i = 0; i < n; ++i) n_in += q.point_terms(R, x.t, src + 3 * i, acc) ? 1u : 0u;
    return n_in;
}

// The loop on the host for one hypothesis: evaluate(pose, tot) fills the ALIGN_ACC sums at a pose and returns n_in.  At most
// max_iterations + 1 turns, as align_run enqueues them: a result still ALIGN_RUNNING means the loop did not end when it must.
template <class Rule, class Eval>
inline typename Rule::Result align_one(const Rule& q, Eval&& evaluate, const lv_graph_pose& guess) {
    typename Rule::Result r;
    AlignHyp h;
    align_start(q.loop, guess, ALIGN_RUNNING, r, h);
    for (int it = 0; it <= q.loop.max_iterations && r.status == ALIGN_RUNNING; ++it) {
        double tot[ALIGN_ACC];
        const uint32_t n_in = evaluate(h.trial, tot);
        align_turn(q, it == 0, tot, n_in, r, h);
    }
    return r;
}

// best[2] of K results: the best objective among those that are not NO_OVERLAP, the smaller index winning a tie, and its n_in
template <class Rule>
inline void align_best(const typename Rule::Result* res, size_t K, int32_t best[2]) {
    best[0] = best[1] = -1;
    for (size_t k = 0; k < K; ++k) {
        if (res[k].status == ALIGN_NO_OVERLAP) continue;
        if (best[0] < 0 || Rule::better(res[k], res[best[0]])) {
            best[0] = (int32_t)k;
            best[1] = (int32_t)res[k].n_in;
        }
    }
}

// ---- the argument rules the methods share (NULL when they hold, otherwise what is wrong); each method keeps its own order
inline const char* align_check_iterations(int32_t max_iterations) {
    return max_iterations < 0 || max_iterations > 1000 ? "max_iterations: 0..1000" : nullptr;
}
inline const char* align_check_loop(double step_tol, double lambda_init, double lambda_min, double lambda_max) {
    const auto fin = [](double v) { return v - v == 0.0; };
    if (!(step_tol >= 0.0 && fin(step_tol))) return "step_tol: finite and >= 0";
    if (!(lambda_min > 0.0 && lambda_min <= lambda_init && lambda_init <= lambda_max && fin(lambda_max)))
        return "0 < lambda_min <= lambda_init <= lambda_max < inf";
    return nullptr;
}
// everything of an align call (who: its name) but its parameters; the message is set
inline int align_check_args(const char* who, const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses, size_t K, const void* results,
                            const int32_t* best) {
    using namespace graph_detail;
    if (!best) { set_error("%s: null best", who); return LV_EINVAL; }
    if (K > LV_NDT_MAX_GUESSES) { set_error("%s: K = %zu above 4096", who, K); return LV_EINVAL; }
    if (n_src > LV_NDT_MAX_SOURCE) { set_error("%s: n_src = %zu above 2^20", who, n_src); return LV_EINVAL; }
    if ((uint64_t)K * (uint64_t)n_src > ((uint64_t)1 << 30)) { set_error("%s: K * n_src above 2^30", who); return LV_EINVAL; }
    if (n_src && (!src || stride < 12)) { set_error("%s: bad source array (stride %zu)", who, stride); return LV_EINVAL; }
    if (K && !guesses) { set_error("%s: null guesses", who); return LV_EINVAL; }
    if (K && !results) { set_error("%s: null results", who); return LV_EINVAL; }
    for (size_t k = 0; k < K; ++k) {
        if (!finite_all(guesses[k].t, 3)) { set_error("%s: guess %zu: t: a non-finite number", who, k); return LV_EINVAL; }
        if (!finite_all(guesses[k].q, 4)) { set_error("%s: guess %zu: q: a non-finite number", who, k); return LV_EINVAL; }
        if (!unit_quat(guesses[k].q)) { set_error("%s: guess %zu: q: norm off 1 by more than 1e-6", who, k); return LV_EINVAL; }
    }
    return LV_OK;
}

// ---- the scratch of one method's align call.  Nothing is allocated before the first call.
template <class Result>
struct AlignStage {
    PointStage src;
    DevBuf<Result> d_res;
    PinBuf<Result> h_res;
    DevBuf<AlignHyp> d_hyp;
    PinBuf<AlignHyp> h_hyp;
    DevBuf<double> d_part;               // ALIGN_PART per (hypothesis, chunk)
    DevBuf<uint32_t> d_running;
    PinBuf<uint32_t> h_running;
    void release() { release_all(src, d_res, h_res, d_hyp, h_hyp, d_part, d_running, h_running); }
};

#ifdef __HIPCC__

// The body of a method's evaluation kernel: grid (chunks, K), ALIGN_NB lanes.  part: ALIGN_PART doubles per (hypothesis, chunk)
template <class Rule>
__device__ __forceinline__ void align_eval(const Rule& q, const float* __restrict__ src, uint32_t n_src, uint32_t n_chunks,
                                           const typename Rule::Result* __restrict__ res, const AlignHyp* __restrict__ hyp,
                                           double* __restrict__ part) {
    __shared__ double sh[ALIGN_NB / 64][ALIGN_ACC + 1];
    const uint32_t h = blockIdx.y, chunk = blockIdx.x;
    if (res[h].status != ALIGN_RUNNING) return;   // (uniform over the workgroup)
    const lv_graph_pose x = hyp[h].trial;
    double R[9];
    gr_rot(x.q, R);
    double acc[ALIGN_ACC];
#pragma unroll
    for (int a = 0; a < ALIGN_ACC; ++a) acc[a] = 0.0;
    uint32_t cnt = 0;
    const uint32_t end = min(n_src, (chunk + 1) * ALIGN_CHUNK);
    for (uint32_t i = chunk * ALIGN_CHUNK + threadIdx.x; i < end; i += ALIGN_NB) {
        const float p[3] = {src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]};
        cnt += q.point_terms(R, x.t, p, acc) ? 1u : 0u;
    }
#pragma unroll
    for (int a = 0; a < ALIGN_ACC; ++a) acc[a] = wave_sum(acc[a]);
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < ALIGN_ACC; ++a) sh[threadIdx.x >> 6][a] = acc[a];
        sh[threadIdx.x >> 6][ALIGN_ACC] = (double)cnt;   // (at most ALIGN_CHUNK: exact)
    }
    __syncthreads();
    if (threadIdx.x <= ALIGN_ACC) {
        double t = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < ALIGN_NB / 64; ++w) t = t + sh[w][threadIdx.x];
        part[((size_t)h * n_chunks + chunk) * ALIGN_PART + threadIdx.x] = t;
    }
}

// The body of a method's turn kernel: one workgroup of ALIGN_NT lanes per hypothesis.  All four wavefronts stage the partials in
// LDS, ALIGN_NT_TILE chunks at a time (coalesced, the loads of a tile in flight together: one lane adding straight from global
// memory waits for every load in turn); the first wavefront then adds each entry in chunk order and its lane 0 runs the turn.
template <class Rule>
__device__ __forceinline__ void align_turn_body(const Rule& q, int first, const double* __restrict__ part, uint32_t n_chunks,
                                                typename Rule::Result* __restrict__ res, AlignHyp* __restrict__ hyp, uint32_t* running) {
    __shared__ double tile[ALIGN_NT_TILE][ALIGN_PART];
    __shared__ double tot[ALIGN_PART];
    const uint32_t h = blockIdx.x;
    if (res[h].status != ALIGN_RUNNING) return;   // (uniform over the workgroup)
    const double* p = part + (size_t)h * n_chunks * ALIGN_PART;
    const uint32_t a = threadIdx.x % ALIGN_PART, row = threadIdx.x / ALIGN_PART;
    double t = 0.0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += ALIGN_NT_TILE) {
        const uint32_t m = min((uint32_t)ALIGN_NT_TILE, n_chunks - c0);
        for (uint32_t c = row; c < m; c += ALIGN_NT / ALIGN_PART) tile[c][a] = p[(size_t)(c0 + c) * ALIGN_PART + a];
        __syncthreads();
        if (threadIdx.x <= ALIGN_ACC)
            for (uint32_t c = 0; c < m; ++c) t = t + tile[c][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x <= ALIGN_ACC) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        typename Rule::Result r = res[h];
        AlignHyp y = hyp[h];
        const bool done = align_turn(q, first != 0, tot, (uint32_t)tot[ALIGN_ACC], r, y);
        res[h] = r;
        hyp[h] = y;
        if (done) atomicSub(running, 1u);
    }
}

// what a method's two kernels take: one line each into align_eval and align_turn_body
template <class Rule>
using AlignEvalKernel = void (*)(Rule, const float*, uint32_t, uint32_t, const typename Rule::Result*, const AlignHyp*, double*);
template <class Rule>
using AlignTurnKernel = void (*)(Rule, int, const double*, uint32_t, typename Rule::Result*, AlignHyp*, uint32_t*);

// The host driver: K hypotheses from `guesses` over n_src source points through the method's kernels.  who: the call's name in
// a message.  Waits for the stream.
template <class Rule>
int align_run(hipStream_t stream, AlignStage<typename Rule::Result>& s, const Rule& q, AlignEvalKernel<Rule> eval, AlignTurnKernel<Rule> turn,
              const void* points, size_t stride, size_t n_src, const lv_graph_pose* guesses, size_t K, typename Rule::Result* results,
              int32_t best[2], const char* who) {
    using Result = typename Rule::Result;
    if (K == 0) {
        best[0] = best[1] = -1;
        return LV_OK;
    }
    const uint32_t n_chunks = blocks_of(n_src, ALIGN_CHUNK);
    int rc = s.src.reserve(stream, n_src, 3 * 4096);   // (synchronises the stream: the pinned records below are free)
    if (!rc) rc = s.d_res.need_pow2(K, 64);
    if (!rc) rc = s.h_res.need_pow2(K, 64);
    if (!rc) rc = s.d_hyp.need_pow2(K, 64);
    if (!rc) rc = s.h_hyp.need_pow2(K, 64);
    if (!rc) rc = s.d_part.need_pow2(std::max<size_t>((size_t)K * n_chunks * ALIGN_PART, 1), 64 * ALIGN_PART);
    if (!rc) rc = s.d_running.need(1);
    if (!rc) rc = s.h_running.need(2);
    if (rc) return rc;
    for (size_t k = 0; k < K; ++k) align_start(q.loop, guesses[k], n_src ? ALIGN_RUNNING : ALIGN_NO_OVERLAP, s.h_res.p[k], s.h_hyp.p[k]);
    if (n_src == 0) {   // nothing to evaluate: every guess comes back as it is
        std::memcpy(results, s.h_res.p, K * sizeof(Result));
        align_best<Rule>(results, K, best);
        return LV_OK;
    }
    s.src.append(points, stride, n_src);
    rc = s.src.upload(stream);
    if (rc) return rc;
    s.h_running.p[1] = (uint32_t)K;
    LV_HIP(hipMemcpyAsync(s.d_res.p, s.h_res.p, K * sizeof(Result), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(s.d_running.p, s.h_running.p + 1, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(s.d_hyp.p, s.h_hyp.p, K * sizeof(AlignHyp), hipMemcpyHostToDevice, stream));
    const dim3 eg(n_chunks, (uint32_t)K);
    for (int it = 0; it <= q.loop.max_iterations;) {
        const int end = std::min(q.loop.max_iterations + 1, it + ALIGN_ITER_CHUNK);
        for (; it < end; ++it) {
            hipLaunchKernelGGL(eval, eg, dim3(ALIGN_NB), 0, stream, q, s.src.d.p, (uint32_t)n_src, n_chunks, s.d_res.p, s.d_hyp.p, s.d_part.p);
            LV_HIP(hipGetLastError());
            hipLaunchKernelGGL(turn, dim3((uint32_t)K), dim3(ALIGN_NT), 0, stream, q, it == 0 ? 1 : 0, s.d_part.p, n_chunks, s.d_res.p, s.d_hyp.p,
                               s.d_running.p);
            LV_HIP(hipGetLastError());
        }
        LV_HIP(hipMemcpyAsync(s.h_running.p, s.d_running.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        if (s.h_running.p[0] == 0) break;
    }
    LV_HIP(hipMemcpyAsync(s.h_res.p, s.d_res.p, K * sizeof(Result), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    if (s.h_running.p[0] != 0) { set_error("%s: %u hypotheses did not finish", who, s.h_running.p[0]); return LV_EHIP; }
    std::memcpy(results, s.h_res.p, K * sizeof(Result));
    align_best<Rule>(results, K, best);
    return LV_OK;
}

#endif   // __HIPCC__

}  // namespace lv
