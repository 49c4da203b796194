// lv_batch.hip — multi-hypothesis measurement passes and iterated updates of the current scan (lv_iterate_batch /
// lv_update_batch): M poses evaluated or refined in a number of launches that does not depend on M (prelocalisation in a
// prior map: the reference's work in progress, README.md:64-67,117; per hypothesis the update of Localizator.cpp:132).
//
// One pass of a chunk of hypotheses is three plain launches, the three-kernel route of lv_update with a hypothesis dimension:
//   batch_search_kernel  grid (scan tiles of 32 points, hypotheses): the tile to the world frame with the hypothesis' pose
//                        constants, the exact k-NN of knn_search (8 lanes per point) -> one hand-over record per point and
//                        hypothesis, the layout of search_kernel (qrec_slots(K) float4 planes);
//   batch_fit_kernel     grid (fit_grid_size(n) + 1, hypotheses): fit_row and the fixed-order contraction of fit_reduce_kernel
//                        -> the hypothesis' block partials; workgroup 0 of each column runs the record-independent half of the
//                        coming solve (batch_prep, solve_prep's algebra);
//   batch_solve_kernel   one workgroup per hypothesis: folds its partials in solve_kernel's order and runs solve_kernel's
//                        algebra (gain, boxplus, convergence, the next pass' pose constants; the posterior covariance on the
//                        pass that ends it).
// lv_iterate_batch: search + fit, then batch_fold_kernel (reduce_final_kernel's fold) per hypothesis.  Every kernel of a
// hypothesis whose update has ended (done) returns at once; nothing waits on another workgroup.  The hypotheses' states live
// in compact BatchHyp records; the context's KfDev, mailbox, capture buffers and resident filter are not touched.
//
// The solve and its prep are restated here over BatchHyp (same building blocks of lv_solve_dev.hpp, same operations in the
// same order, same FMA contraction) rather than moved out of lv_solve.hip: extracting solve_kernel's body into a shared
// inline function changed its register allocation, and the update's kernels must stay as they are.
#define LV_MATCH_DEVICE_ONLY
#include "lv_match.hip"   // knn_search, fit_row, plane_qr_solve, out_pair (its kernels and host code are not compiled here)

#include <cstring>

namespace lv {

// The per-hypothesis state.  The head (x .. sums) is what the host reads back; P_post follows it.
struct BatchHyp {
    double x[NX];
    int t, iter, done, passes;
    int fallback_queries, pad_[3];
    double sums[SUMS_LEN];        // record of the hypothesis' latest pass
    double P_post[NS * NS];
    double x_prop[NX];
    double P_prop[NS * NS];
    double prep_dxnew[NS];
    double prep_P[NS * NS];
    double prep_A1[12 * 12];
    double degen_eig[6];
    PoseConsts pose;
};

constexpr int BS_S = 8;                 // lanes per scan point (the general-K build and pass_kernel use 8)
constexpr int BS_GS = 256 / BS_S;       // scan points per search workgroup
constexpr int B_FOLD_THREADS = 576;     // solve_kernel's geometry (lv_solve.hip: FOLD_THREADS, FOLD_PARTS, FOLD_DEPTH)
constexpr int B_FOLD_PARTS = B_FOLD_THREADS / SUMS_LEN;
constexpr int B_FOLD_DEPTH = 44;

// search_kernel (non-capturing, not the first launch of an update) with the pose and `done` of hypothesis blockIdx.y.
// sink: knn_search's counters (a KfDev of the batch's own).
template <int K>
__global__ __launch_bounds__(256) void batch_search_kernel(MapView map, const float4* __restrict__ scan, uint32_t n,
                                                           const BatchHyp* __restrict__ hyps, float4* __restrict__ qrec,
                                                           uint32_t qstride, double max_dist_sq, KfDev* __restrict__ sink) {
    constexpr int S = BS_S, GS = BS_GS, STAGE = S * 8;
    __shared__ Xyz s_stage[GS][STAGE];
    __shared__ uint32_t s_pref[4][64], s_start[4][64];
    const BatchHyp* hy = hyps + blockIdx.y;
    if (hy->done) return;
    qrec += (size_t)blockIdx.y * qrec_slots(K) * qstride;
    const int tid = threadIdx.x;
    const int gq = tid / S, gl = tid % S;
    const uint32_t q = blockIdx.x * (uint32_t)GS + (uint32_t)gq;
    const bool live = q < n;
    kkey k[K];
#pragma unroll
    for (int j = 0; j < K; ++j) k[j] = none_key();
    uint32_t bstart = 0;
    int src = -1;
    const float4 sp = scan[live ? q : n - 1];
    float qx, qy, qz;
    rt_apply(hy->pose.Tc, sp.x, sp.y, sp.z, qx, qy, qz);   // Mapper.cpp:51
    knn_search<S, false>(map, sink, qx, qy, qz, gl, k, bstart, src, nullptr, false, live, s_stage[gq], max_dist_sq, s_pref[tid >> 6],
                         s_start[tid >> 6]);
    int found = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) found += key_real(k[j]) ? 1 : 0;
    if (!live) return;
    // the record of search_kernel: slots 0..K-1 the neighbours {x, y, z, id}, slot K the world point and scan index, then the
    // K distance bits followed by `found`, four words to a slot
#pragma unroll
    for (int slot0 = 0; slot0 < qrec_slots(K); slot0 += S) {
        const int slot = slot0 + gl;
        if (slot >= qrec_slots(K)) break;
        float4 v;
        if (slot < K) {
            kkey kk = k[0];
#pragma unroll
            for (int j = 1; j < K; ++j) kk = (slot == j) ? k[j] : kk;
            v = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
            if (key_real(kk)) {
                const uint32_t pos = key_lo(kk);
                if (src == 0 && pos < (uint32_t)STAGE) {
                    const Xyz w = s_stage[gq][pos];
                    v = make_float4(w.x, w.y, w.z, __uint_as_float(0xFFFFFFFFu));
                } else if (src >= 0) {
                    const Xyz w = reinterpret_cast<const Xyz*>(map.bxyz[src])[(size_t)bstart + pos];
                    v = make_float4(w.x, w.y, w.z, __uint_as_float(map.bidx[src][(size_t)bstart + pos]));
                } else {
                    v = map.orig[pos];
                    v.w = __uint_as_float(pos);
                }
            }
        } else if (slot == K) {
            v = make_float4(qx, qy, qz, sp.w);
        } else {
            float wv[4];
#pragma unroll
            for (int cw = 0; cw < 4; ++cw) {
                const int w = (slot - K - 1) * 4 + cw;
                float val = w == K ? __int_as_float(found) : 0.f;
#pragma unroll
                for (int j = 0; j < K; ++j) val = (w == j) ? __uint_as_float(key_hi(k[j])) : val;
                wv[cw] = val;
            }
            v = make_float4(wv[0], wv[1], wv[2], wv[3]);
        }
        qrec[(size_t)slot * qstride + q] = v;
    }
}

template <int NW, int NT>
__device__ void batch_prep(BatchHyp* __restrict__ kf, double R_inv);

// fit_reduce_kernel (non-capturing) for hypothesis blockIdx.y: nfit = gridDim.x - 1 plane-fitting workgroups, the same
// point-to-workgroup map and contraction order, so the hypothesis' partials equal the three-kernel route's
constexpr int B_FIT_POINTS = 256;
template <bool EXT, int K>
__global__ __launch_bounds__(B_FIT_POINTS) void batch_fit_kernel(const float4* __restrict__ qrec, uint32_t qstride, uint32_t n,
                                                                 BatchHyp* __restrict__ hyps, MatchParams prm, double* __restrict__ partials) {
    constexpr int G = B_FIT_POINTS;
    constexpr int NWAVE = G / 64;
    constexpr int W = EXT ? 12 : 6;
    constexpr int ROW_W = W + 2;
    constexpr int NOUT = W * (W + 1) / 2 + W + 2;
    constexpr int NACC = (NOUT + 63) / 64;
    __shared__ double s_rows[G][ROW_W];
    __shared__ double s_out[NWAVE][2][SUMS_LEN];
    BatchHyp* hy = hyps + blockIdx.y;
    if (hy->done) return;
    if (blockIdx.x == 0) {
        batch_prep<W, G>(hy, prm.R_inv);
        return;
    }
    const uint32_t nfit = gridDim.x - 1u, bid = blockIdx.x - 1u;
    qrec += (size_t)blockIdx.y * qrec_slots(K) * qstride;
    partials += ((size_t)blockIdx.y * nfit + bid) * SUMS_LEN;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const PoseConsts& pc = hy->pose;
    const DebugOut dbg{};
    int oa[NACC], ob[NACC], orec[NACC];
    double acc[NACC];
    constexpr bool HALVES = NOUT <= 32;
    const int olane = HALVES ? (lane & 31) : lane;
    const int prow0 = HALVES ? (lane >> 5) * 32 : 0;
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        oa[a] = ob[a] = orec[a] = 0;
        acc[a] = 0.0;
        if (olane + a * 64 < NOUT) out_pair<W>(olane + a * 64, oa[a], ob[a], orec[a]);
    }
    for (int t = tid; t < 2 * NWAVE * SUMS_LEN; t += G) (&s_out[0][0][0])[t] = 0.0;
    const uint32_t vb = (bid % 8u) * (nfit / 8u) + bid / 8u;
    const uint32_t per_iter = (uint32_t)G * nfit;
    const uint32_t iters = (n + per_iter - 1) / per_iter;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t q = (it * nfit + vb) * (uint32_t)G + (uint32_t)tid;
        float P[K][3];
        uint32_t nidx[K], dbits[K];
        float qx = 0.f, qy = 0.f, qz = 0.f;
        uint32_t oq = 0;
        int found = -1;
#pragma unroll
        for (int j = 0; j < K; ++j) { P[j][0] = P[j][1] = P[j][2] = 0.f; nidx[j] = 0xFFFFFFFFu; dbits[j] = 0x7f800000u; }
        if (q < n) {
            float4 r[qrec_slots(K)];
#pragma unroll
            for (int sl = 0; sl < qrec_slots(K); ++sl) r[sl] = qrec[(size_t)sl * qstride + q];
#pragma unroll
            for (int j = 0; j < K; ++j) { P[j][0] = r[j].x; P[j][1] = r[j].y; P[j][2] = r[j].z; nidx[j] = __float_as_uint(r[j].w); }
            qx = r[K].x; qy = r[K].y; qz = r[K].z; oq = __float_as_uint(r[K].w);
            const auto dword = [&](int w) { const float4 v = r[K + 1 + w / 4]; return (w & 3) == 0 ? v.x : (w & 3) == 1 ? v.y : (w & 3) == 2 ? v.z : v.w; };
#pragma unroll
            for (int j = 0; j < K; ++j) dbits[j] = __float_as_uint(dword(j));
            found = __float_as_int(dword(K));
        }
        fit_row<W, EXT, false>(pc, prm, dbg, found, P, nidx, dbits, qx, qy, qz, oq, s_rows[tid]);
        __syncthreads();
        const double (*rows)[ROW_W] = s_rows + wave * 64;
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            if (olane + a * 64 < NOUT) {
                double sacc = acc[a];
#pragma unroll 8
                for (int p = 0; p < (HALVES ? 32 : 64); ++p) sacc += rows[prow0 + p][oa[a]] * rows[prow0 + p][ob[a]];
                acc[a] = sacc;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < NACC; ++a)
        if (olane + a * 64 < NOUT) s_out[wave][HALVES ? (lane >> 5) : 0][orec[a]] = acc[a];
    __syncthreads();
    if (tid < SUMS_LEN) {
        double s = s_out[0][0][tid] + s_out[0][1][tid];
#pragma unroll
        for (int w = 1; w < NWAVE; ++w) s += s_out[w][0][tid] + s_out[w][1][tid];
        partials[tid] = s;
    }
}

// ---- the solve over BatchHyp: the filter algebra of lv_solve.hip, compiled as it is there ----------------------------------
#pragma clang fp contract(fast)

// solve_prep (lv_solve_dev.hpp) over a hypothesis record
template <int NW, int NT>
__device__ void batch_prep(BatchHyp* __restrict__ kf, double R_inv) {
    __shared__ double pP[NS][LD], pB[NS][LD], pJ[NS][LD];
    __shared__ double pW[2][12][13];
    __shared__ double px[NX], pxp[NX], pdx[NS];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < NS * NS; e += NT) pB[e / NS][e % NS] = kf->P_prop[e];
    if (tid < NX) { px[tid] = kf->x[tid]; pxp[tid] = kf->x_prop[tid]; }
    set_identity<NT>(pJ, tid);
    __syncthreads();
    if (wave < 3 && lane == 0) manifold_block(wave, 0, px, pxp, nullptr, pdx, pJ);
    if (wave == 3 && lane < 15) {
        const int dof = lane < 3 ? lane : lane + 6;
        const int si = vect_state_index(dof);
        pdx[dof] = px[si] - pxp[si];
    }
    __syncthreads();
    if (tid < NS) {
        double s = 0.0;
        const int b = (tid >= 3 && tid < 6) ? 3 : (tid >= 6 && tid < 9) ? 6 : (tid >= 21) ? 21 : -1;
        if (b < 0) s = pdx[tid];
        else if (b == 21) s = pJ[tid][21] * pdx[21] + pJ[tid][22] * pdx[22];
        else s = dot3d(pJ[tid][b], pdx[b], pJ[tid][b + 1], pdx[b + 1], pJ[tid][b + 2], pdx[b + 2]);
        kf->prep_dxnew[tid] = s;
    }
    congruence<NT>(pP, pJ, pB, tid);
    __syncthreads();
    for (int e = tid; e < NS * NS; e += NT) kf->prep_P[e] = pP[e / NS][e % NS];
    if (tid < NW * NW) pW[0][tid / NW][tid % NW] = pP[tid / NW][tid % NW] * R_inv;
    __syncthreads();
    int cur = 0;
    gj_spd<NW>(pW, cur, tid);
    if (tid < NW * NW) kf->prep_A1[tid] = pW[cur][tid / NW][tid % NW];
}

// fold_issue / fold_stage / fold_total of lv_solve.hip: thread (o, part) sums records part, part + 6, ... in four interleaved
// running sums; the six part sums are combined pairwise
__device__ __forceinline__ void batch_fold(const double* __restrict__ recs, int nrec, double (*s_part)[SUMS_LEN], double* out, int tid) {
    if (nrec <= B_FOLD_PARTS * B_FOLD_DEPTH) {
        double fv[B_FOLD_DEPTH];
        const int fo = tid % SUMS_LEN, fpart = tid / SUMS_LEN;
#pragma unroll
        for (int i = 0; i < B_FOLD_DEPTH; ++i) {
            const int g = fpart + B_FOLD_PARTS * i;
            fv[i] = g < nrec ? recs[(size_t)g * SUMS_LEN + fo] : 0.0;
        }
        double a0 = fv[0], a1 = fv[1], a2 = fv[2], a3 = fv[3];
#pragma unroll
        for (int i = 4; i + 3 < B_FOLD_DEPTH; i += 4) { a0 += fv[i]; a1 += fv[i + 1]; a2 += fv[i + 2]; a3 += fv[i + 3]; }
        s_part[tid / SUMS_LEN][tid % SUMS_LEN] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (tid < SUMS_LEN)
            out[tid] = ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) + (s_part[4][tid] + s_part[5][tid]);
    } else if (tid < SUMS_LEN) {
        double s = 0.0;
        for (int g = 0; g < nrec; ++g) s += recs[(size_t)g * SUMS_LEN + tid];
        out[tid] = s;
    }
}

// lv_iterate_batch: the hypothesis' record from its partials (reduce_final_kernel's fold)
__global__ __launch_bounds__(B_FOLD_THREADS) void batch_fold_kernel(BatchHyp* __restrict__ hyps, const double* __restrict__ partials, int nrec) {
    __shared__ double s_part[B_FOLD_PARTS][SUMS_LEN];
    batch_fold(partials + (size_t)blockIdx.x * nrec * SUMS_LEN, nrec, s_part, hyps[blockIdx.x].sums, threadIdx.x);
}

// solve_kernel (lv_solve.hip) for hypothesis blockIdx.x, without its mailbox, trace, sums log and clocks
template <int NW>
__global__ __launch_bounds__(B_FOLD_THREADS) void batch_solve_kernel(BatchHyp* __restrict__ hyps, const double* __restrict__ partials, int nrec,
                                                                     SolveParams prm) {
    __shared__ double sP[NS][LD], sA[NS][LD], sB[NS][LD], sJ[NS][LD];
    __shared__ double sW[2][12][13], sT[12][12];
    __shared__ double sX[NS][12], sKx[NS][12], sHTH[12][12], sHTh[12];
    __shared__ double sG[NS][12];
    __shared__ double sv[12];
    __shared__ double sdxnew[NS], sdxo[NS], sx[NX], sxp[NX], srec[SUMS_LEN];
    __shared__ double s_part[B_FOLD_PARTS][SUMS_LEN];
    __shared__ double sRot[4][9];
    __shared__ PoseConsts s_pose;
    __shared__ float s_ptmp[8];
    __shared__ int s_last, s_conv;
    BatchHyp* kf = hyps + blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    if (kf->done) return;
    partials += (size_t)blockIdx.x * nrec * SUMS_LEN;
    if (tid >= 128 && tid < 128 + NX) { sx[tid - 128] = kf->x[tid - 128]; sxp[tid - 128] = kf->x_prop[tid - 128]; }
    if (tid < NS * NS) sP[tid / NS][tid % NS] = kf->prep_P[tid];
    if (tid < NS) sdxnew[tid] = kf->prep_dxnew[tid];
    if (tid >= 192 && tid < 192 + NW * NW) sG[(tid - 192) / NW][(tid - 192) % NW] = kf->prep_A1[tid - 192];
    const int pass = kf->passes;
    const int kf_t = kf->t, kf_iter = kf->iter;
    batch_fold(partials, nrec, s_part, srec, tid);
    if (tid == 200) s_conv = 1;
    __syncthreads();
    if (tid < SUMS_LEN) kf->sums[tid] = srec[tid];
    if (tid < 144) {
        const int a = tid / 12, b = tid % 12;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        sHTH[a][b] = srec[lo * 12 - lo * (lo - 1) / 2 + (hi - lo)];
    }
    if (tid >= 192 && tid < 204) sHTh[tid - 192] = srec[78 + tid - 192];
    const double n_valid = srec[90];
    if (n_valid == 0.0) {   // h_share_model: dyn_share.valid = false -> `continue`
        if (tid == 0) {
            kf->passes = pass + 1;
            kf->iter = kf_iter + 1;
            if (kf_iter + 1 >= prm.maximum_iter) kf->done = 1;
        }
        return;
    }
    __syncthreads();
    if (prm.degeneracy_mode) {
        if (tid == 0) degeneracy_stage(sHTH, sHTh, prm.degeneracy_mode, prm.degeneracy_threshold, kf->degen_eig);
        __syncthreads();
    }
    if (tid < NS * NS) sA[tid / NS][tid % NS] = sP[tid / NS][tid % NS] * prm.R_inv;
    int cur = 0;
    if (tid < NW * NW) {
        const int i = tid / NW, j = tid % NW;
        sW[cur][i][j] = sG[i][j] + sHTH[i][j];
    }
    if (tid >= 64 && tid < 64 + NW) {
        const int i = tid - 64;
        double s = sHTh[i];
        for (int j = 0; j < NW; ++j) s += sHTH[i][j] * sdxnew[j];
        sv[i] = s;
    }
    __syncthreads();
    gj_spd<NW>(sW, cur, tid);
    if (tid < NW * NW) {
        const int i = tid / NW, c = tid % NW;
        double s = 0.0;
        for (int j = 0; j < NW; ++j) s += sG[i][j] * sW[cur][j][c];
        sT[i][c] = s;
    }
    __syncthreads();
    if (tid < NS * NW) {
        const int i = tid / NW, c = tid % NW;
        double v;
        if (i < NW) {
            v = sW[cur][i][c];
        } else {
            double s = 0.0;
            for (int j = 0; j < NW; ++j) s += sA[i][j] * sT[j][c];
            v = s;
        }
        sX[i][c] = v;
    }
    __syncthreads();
    if (tid < NS) {
        double s = 0.0;
        for (int j = 0; j < NW; ++j) s += sX[tid][j] * sv[j];
        const double d = s - sdxnew[tid];
        sdxo[tid] = d;
        if (fabs(d) > prm.limits[tid]) s_conv = 0;
    }
    __syncthreads();
    if (wave < 3 && lane == 0) boxplus_block(wave, sx, sdxo);
    if (wave == 3 && lane < 15) {
        const int dof = lane < 3 ? lane : lane + 6;
        sx[vect_state_index(dof)] += sdxo[dof];
    }
    if (tid == 256) {
        int t = kf_t;
        if (s_conv) t++;
        kf->t = t;
        s_last = (t > 1 || kf_iter == prm.maximum_iter - 1) ? 1 : 0;
    }
    __syncthreads();
    const int last = s_last;
    if (tid < NX) kf->x[tid] = sx[tid];
    if (!last && tid >= 320 && tid < 324) {
        const int w = tid - 320;
        const int q = (w & 1) ? 7 : 3;
        const double sg = (w & 2) ? -1.0 : 1.0;
        const double qq[4] = {sg * sx[q], sg * sx[q + 1], sg * sx[q + 2], sx[q + 3]};
        quat_to_rot(qq, &sRot[w][0]);
    }
    __syncthreads();
    if (tid == 0) {
        kf->passes = pass + 1;
        kf->iter = kf_iter + 1;
        if (last) kf->done = 1;
    }
    if (!last) {
        if (tid >= 64 && tid < 128) pose_consts_stage_a(tid - 64, sx, sRot, &s_pose, s_ptmp);
        __syncthreads();
        if (tid >= 64 && tid < 128) pose_consts_stage_b(tid - 64, sRot, &s_pose, s_ptmp);
        __syncthreads();
        constexpr int NW32 = (int)(sizeof(PoseConsts) / 4);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&s_pose);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&kf->pose);
        if (tid < NW32) dst[tid] = src[tid];
        return;
    }
    // terminal pass: L_ = J2 P_ J2^T, K_x rows projected, P_ <- P_ J2^T, P = L_ - K_x[:, :NW] P_[0:NW, :]
    __syncthreads();
    set_identity<B_FOLD_THREADS>(sJ, tid);
    __syncthreads();
    if (wave < 3 && lane == 0) manifold_block(wave, 1, sx, sxp, sdxo, nullptr, sJ);
    __syncthreads();
    congruence<B_FOLD_THREADS>(sB, sJ, sP, tid);
    mm<B_FOLD_THREADS>(sA, sP, sJ, true, tid);
    __syncthreads();
    if (tid < NS * NW) {
        const int i = tid / NW, c = tid % NW;
        double t = 0.0;
        for (int j = 0; j < NW; ++j) t += sX[i][j] * sHTH[j][c];
        sKx[i][c] = t;
    }
    __syncthreads();
    if (tid < NS * NW) {
        const int i = tid / NW, c = tid % NW;
        double s = 0;
        for (int r = 0; r < NS; ++r) s += sJ[i][r] * sKx[r][c];
        sX[i][c] = s;
    }
    __syncthreads();
    if (tid < NS * NS) {
        const int i = tid / NS, j = tid % NS;
        double s = 0;
        for (int c = 0; c < NW; ++c) s += sX[i][c] * sA[c][j];
        kf->P_post[tid] = sB[i][j] - s;
    }
}

#pragma clang fp contract(off)

// ---- host ----------------------------------------------------------------------------------------------------------------
namespace {

template <int K>
void launch_batch_pass(hipStream_t s, const MapView& map, const float4* scan, uint32_t n, BatchHyp* hyps, uint32_t mc, float4* qrec,
                       uint32_t qstride, double* part, int nfit, const MatchParams& mp, KfDev* sink) {
    const uint32_t tiles = (n + BS_GS - 1) / BS_GS;
    hipLaunchKernelGGL((batch_search_kernel<K>), dim3(tiles, mc), dim3(256), 0, s, map, scan, n, hyps, qrec, qstride, mp.max_dist_plane_sq, sink);
    if (mp.estimate_extrinsics)
        hipLaunchKernelGGL((batch_fit_kernel<true, K>), dim3(nfit + 1, mc), dim3(B_FIT_POINTS), 0, s, qrec, qstride, n, hyps, mp, part);
    else
        hipLaunchKernelGGL((batch_fit_kernel<false, K>), dim3(nfit + 1, mc), dim3(B_FIT_POINTS), 0, s, qrec, qstride, n, hyps, mp, part);
}

}  // namespace

size_t BatchStore::chunk_size(uint32_t n, int num_match) const {
    // hand-over records: qrec_slots(K) x 16 bytes per point and hypothesis (128 B for K = 5)
    const size_t per_hyp = (size_t)qrec_slots(num_match) * sizeof(float4) * n;
    size_t c = BATCH_RECORD_BUDGET / (per_hyp ? per_hyp : 1);
    if (c < 1) c = 1;
    if (c > 65535) c = 65535;   // (grid y)
    if (chunk_hyp > 0 && (size_t)chunk_hyp < c) c = (size_t)chunk_hyp;
    return c;
}

int BatchStore::run(const lv_params& prm, int max_blocks, const MapView& map, const float4* scan, uint32_t n, hipStream_t stream,
                    const lv_state* xs, size_t m, const double* P, bool solve, lv_state* x_out, double* P_out, int* passes, double* recs) {
    const int K = prm.NUM_MATCH_POINTS;
    if (K < 3 || K > 8) { set_error("NUM_MATCH_POINTS must be 3..8 (got %d)", K); return LV_EINVAL; }
    const size_t chunk = chunk_size(n, K);
    const int nfit = fit_grid_size(n, max_blocks);
    const size_t mc_max = chunk < m ? chunk : m;
    int rc = d_hyp.need(m);
    if (!rc) rc = d_qrec.need(mc_max * qrec_slots(K) * (size_t)n);
    if (!rc) rc = d_part.need(mc_max * (size_t)nfit * SUMS_LEN);
    if (!rc && !d_sink) {
        rc = d_sink.need(1);
        if (!rc) LV_HIP(hipMemsetAsync(d_sink, 0, sizeof(KfDev), stream));
    }
    // (every call ends with a wait on the stream: nothing reads the pinned records when they grow)
    if (!rc) rc = h_hyp.need(m);
    if (rc) return rc;
    // every hypothesis starts as lv_update's first pass does: x_prop = x, P_prop = P_post = P, the pass constants from the host
    for (size_t i = 0; i < m; ++i) {
        BatchHyp& h = h_hyp[i];
        std::memset(&h, 0, sizeof(h));
        std::memcpy(h.x, &xs[i], sizeof(h.x));
        std::memcpy(h.x_prop, &xs[i], sizeof(h.x_prop));
        if (P) {
            std::memcpy(h.P_prop, P, sizeof(h.P_prop));
            std::memcpy(h.P_post, P, sizeof(h.P_post));
        }
        h.t = 0;
        h.iter = -1;   // upstream loop starts at i = -1
        compute_pose_consts(h.x, &h.pose);
    }
    LV_HIP(hipMemcpyAsync(d_hyp, h_hyp, m * sizeof(BatchHyp), hipMemcpyHostToDevice, stream));
    MatchParams mp{};
    mp.R_inv = 1.0 / prm.LiDAR_noise;
    mp.max_dist_plane_sq = prm.MAX_DIST_PLANE * prm.MAX_DIST_PLANE;
    mp.planes_threshold = prm.PLANES_THRESHOLD;
    mp.estimate_extrinsics = prm.estimate_extrinsics;
    SolveParams sp{};
    sp.R = prm.LiDAR_noise;
    sp.R_inv = 1.0 / prm.LiDAR_noise;
    for (int i = 0; i < NS; ++i) sp.limits[i] = prm.LIMITS[i];
    sp.maximum_iter = prm.MAX_NUM_ITERS;
    sp.estimate_extrinsics = prm.estimate_extrinsics;
    sp.degeneracy_mode = prm.degeneracy_mode;
    sp.degeneracy_threshold = prm.degeneracy_threshold;
    const int npass = solve ? prm.MAX_NUM_ITERS + 1 : 1;
    const uint32_t qstride = n;
    for (size_t c0 = 0; c0 < m; c0 += chunk) {
        const uint32_t mc = (uint32_t)((m - c0) < chunk ? (m - c0) : chunk);
        BatchHyp* hy = d_hyp + c0;
        for (int p = 0; p < npass; ++p) {
            switch (K) {
#define LV_K(K_) case K_: launch_batch_pass<K_>(stream, map, scan, n, hy, mc, d_qrec, qstride, d_part, nfit, mp, d_sink); break
                LV_K(3); LV_K(4); LV_K(5); LV_K(6); LV_K(7); LV_K(8);
#undef LV_K
            }
            if (!solve)
                hipLaunchKernelGGL(batch_fold_kernel, dim3(mc), dim3(B_FOLD_THREADS), 0, stream, hy, d_part, nfit);
            else if (prm.estimate_extrinsics)
                hipLaunchKernelGGL((batch_solve_kernel<12>), dim3(mc), dim3(B_FOLD_THREADS), 0, stream, hy, d_part, nfit, sp);
            else
                hipLaunchKernelGGL((batch_solve_kernel<6>), dim3(mc), dim3(B_FOLD_THREADS), 0, stream, hy, d_part, nfit, sp);
            LV_HIP(hipGetLastError());
        }
    }
    // the head of every record (x .. sums), and P_post when asked for: one wait
    const size_t head = P_out ? offsetof(BatchHyp, x_prop) : offsetof(BatchHyp, P_post);
    LV_HIP(hipMemcpy2DAsync(h_hyp, sizeof(BatchHyp), d_hyp, sizeof(BatchHyp), head, m, hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < m; ++i) {
        const BatchHyp& h = h_hyp[i];
        if (x_out) std::memcpy(&x_out[i], h.x, sizeof(h.x));
        if (P_out) std::memcpy(P_out + i * NS * NS, h.P_post, sizeof(h.P_post));
        if (passes) passes[i] = h.passes;
        if (recs) std::memcpy(recs + i * SUMS_LEN, h.sums, sizeof(h.sums));
    }
    return LV_OK;
}

void BatchStore::release() {   // (chunk_hyp, an option of the context, stays)
    d_hyp.release();
    d_qrec.release();
    d_part.release();
    d_sink.release();
    h_hyp.release();
}

}  // namespace lv
