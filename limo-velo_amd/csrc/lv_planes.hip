// lv_planes.hip — lv_map_planes: RANSAC planes of the device map, one after the other (include/limovelo_hip.h "Plane
// segmentation"; the arithmetic and the rules: lv_planes.hpp).  Per round r:
//
//   planes_flag_kernel       one lane per id: 1 at an included living id no plane has taken yet; a hipcub exclusive scan of the flags
//   planes_compact_kernel    and a scatter make the round's candidates (x, y, z, id) in map order.  The host reads n.
//   planes_hyp_kernel        one lane per hypothesis: three hashed draws, the plane in f64 (pl_hypothesis), its count zeroed.
//   planes_score_kernel      THE HOT PATH, K x n inlier tests.  One lane per hypothesis: its plane (6 floats) and its count stay in
//                            registers; a workgroup of PL_CHUNK lanes stages PL_TILE candidates in the LDS and every lane reads them
//                            all at the same address (a broadcast: no bank conflict), 3 subtractions, 3 multiplications, 2
//                            additions, a compare and a count per test.  No ballot, shuffle or atomic in the loop; one integer
//                            atomicAdd per lane and tile.  Grid: (candidate tiles) x (hypothesis chunks).
//   argmax                   on the host, from the K counts: the most inliers, ties to the smaller h (an invalid hypothesis counts 0).
//   planes_refit_kernel      over the winner's inliers: the quantised offsets from the anchor summed in int64, PL_SUMS sums per
//                            workgroup in a slot of its own (4096 candidates per workgroup: 2^44 * 2^12 < 2^63).  The host folds
//                            the slots in 128 bits, solves the 3 x 3 (sym3_eig) and has the final plane.
//   planes_classify_kernel   one lane per candidate: an inlier of the final plane takes the label r at its living rank and leaves
//                            the candidates; one atomicAdd per wavefront counts them.
// Every count is an integer sum and every test one lane's f32 arithmetic: the result does not depend on the launch geometry or on
// the order in which workgroups run.
#include "lv_planes.hpp"

#include "lv_query_dev.hpp"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

namespace lv {

namespace {

constexpr int32_t PL_OUT = -2;    // d_state: dead or excluded
constexpr int32_t PL_FREE = -1;   // d_state: a candidate still

// the final (or winning) plane as the refit and classify kernels take it
struct PlaneArg {
    float nx, ny, nz, ax, ay, az, distance;
};

__global__ __launch_bounds__(256) void planes_init_kernel(const float4* __restrict__ orig, uint32_t n_ids, const uint32_t* __restrict__ rank,
                                                          const uint8_t* __restrict__ mask, int32_t* __restrict__ state,
                                                          int32_t* __restrict__ labels) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const bool alive = pt_alive(orig[id]);
    const uint32_t rk = alive ? rank_of(rank, id) : 0u;
    state[id] = (alive && (!mask || mask[rk] != 0)) ? PL_FREE : PL_OUT;
    if (alive && labels) labels[rk] = -1;
}

__global__ __launch_bounds__(256) void planes_flag_kernel(const int32_t* __restrict__ state, uint32_t n_ids, uint32_t* __restrict__ flag) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n_ids) flag[id] = state[id] == PL_FREE ? 1u : 0u;
}

__global__ __launch_bounds__(256) void planes_compact_kernel(const float4* __restrict__ orig, uint32_t n_ids, const uint32_t* __restrict__ flag,
                                                             const uint32_t* __restrict__ pos, float4* __restrict__ cand) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids || !flag[id]) return;
    const float4 p = orig[id];
    cand[pos[id]] = make_float4(p.x, p.y, p.z, __uint_as_float(id));
}

__global__ __launch_bounds__(256) void planes_hyp_kernel(const float4* __restrict__ cand, uint32_t n, PlaneRule q, uint32_t round,
                                                         float4* __restrict__ hyp, uint32_t* __restrict__ count) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h == 0u) count[q.iterations] = 0u;   // (the classify kernel's counter)
    if (h >= q.iterations) return;
    const uint32_t i0 = pl_draw(q.seed, round, h, 0u, n), i1 = pl_draw(q.seed, round, h, 1u, n), i2 = pl_draw(q.seed, round, h, 2u, n);
    const float4 a = cand[i0], b = cand[i1], c = cand[i2];
    const float p0[3] = {a.x, a.y, a.z}, p1[3] = {b.x, b.y, b.z}, p2[3] = {c.x, c.y, c.z};
    float nrm[3];
    bool valid = i0 != i1 && i0 != i2 && i1 != i2;
    valid = pl_hypothesis(p0, p1, p2, q.constraint, q.axis[0], q.axis[1], q.axis[2], q.cos_max, q.sin_max, nrm) && valid;
    hyp[2u * h] = make_float4(nrm[0], nrm[1], nrm[2], valid ? 1.f : 0.f);
    hyp[2u * h + 1u] = make_float4(a.x, a.y, a.z, 0.f);
    count[h] = 0u;
}

__global__ __launch_bounds__(PL_CHUNK) void planes_score_kernel(const float4* __restrict__ cand, uint32_t n, const float4* __restrict__ hyp,
                                                                uint32_t K, float distance, uint32_t* __restrict__ count) {
    __shared__ float4 s_tile[PL_TILE];
    const uint32_t base = blockIdx.x * (uint32_t)PL_TILE;
    const uint32_t cnt = min((uint32_t)PL_TILE, n - base);   // (the grid has no empty tile: base < n)
    for (uint32_t i = threadIdx.x; i < cnt; i += (uint32_t)PL_CHUNK) s_tile[i] = cand[base + i];
    const uint32_t h = blockIdx.y * (uint32_t)PL_CHUNK + threadIdx.x;
    const bool mine = h < K;
    const float4 N = mine ? hyp[2u * h] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 A = mine ? hyp[2u * h + 1u] : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    uint32_t c = 0u;
#pragma unroll 8
    for (uint32_t i = 0; i < cnt; ++i) {
        const float4 p = s_tile[i];
        c += pl_inlier(N.x, N.y, N.z, A.x, A.y, A.z, p.x, p.y, p.z, distance) ? 1u : 0u;
    }
    if (mine && N.w != 0.f && c != 0u) atomicAdd(count + h, c);
}

__global__ __launch_bounds__(256) void planes_refit_kernel(const float4* __restrict__ cand, uint32_t n, PlaneArg P, long long* __restrict__ slot) {
    __shared__ long long s_part[4][PL_SUMS];
    const uint32_t base = blockIdx.x * (uint32_t)(256 * PL_FIT_PER);
    long long s[PL_SUMS];
#pragma unroll
    for (int k = 0; k < PL_SUMS; ++k) s[k] = 0;
#pragma unroll 4
    for (int j = 0; j < PL_FIT_PER; ++j) {
        const uint32_t i = base + (uint32_t)j * 256u + threadIdx.x;
        if (i >= n) continue;
        const float4 p = cand[i];
        if (!pl_inlier(P.nx, P.ny, P.nz, P.ax, P.ay, P.az, p.x, p.y, p.z, P.distance)) continue;
        int32_t gx, gy, gz;
        const bool okx = pl_quant(p.x, P.ax, &gx), oky = pl_quant(p.y, P.ay, &gy), okz = pl_quant(p.z, P.az, &gz);
        if (okx && oky && okz) pl_accumulate(s, gx, gy, gz);
    }
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < PL_SUMS; ++k) {
        long long v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_part[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)PL_SUMS)
        slot[(size_t)blockIdx.x * PL_SUMS + threadIdx.x] = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void planes_classify_kernel(const float4* __restrict__ cand, uint32_t n, PlaneArg P, int32_t label,
                                                              const uint32_t* __restrict__ rank, int32_t* __restrict__ state,
                                                              int32_t* __restrict__ labels, uint32_t* __restrict__ members) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false;
    if (i < n) {
        const float4 p = cand[i];
        in = pl_inlier(P.nx, P.ny, P.nz, P.ax, P.ay, P.az, p.x, p.y, p.z, P.distance);
        if (in) {
            const uint32_t id = __float_as_uint(p.w);
            state[id] = label;
            if (labels) labels[rank_of(rank, id)] = label;
        }
    }
    const unsigned long long hit = __ballot(in);
    if (hit != 0ull && (int)(threadIdx.x & 63u) == __ffsll((long long)hit) - 1) atomicAdd(members, (uint32_t)__popcll(hit));
}

}  // namespace

int PlaneStore::ensure(size_t n_ids, size_t m, uint32_t iterations) {
    int rc = d_state.need(n_ids);
    if (!rc) rc = d_flag.need(n_ids);
    if (!rc) rc = d_pos.need(n_ids + 1);
    if (!rc) rc = d_cand.need(m);
    if (!rc) rc = d_hyp.need(2 * (size_t)iterations);
    if (!rc) rc = d_count.need((size_t)iterations + 1);
    if (!rc) rc = d_slot.need((size_t)blocks_of(m, 256 * PL_FIT_PER) * PL_SUMS);
    if (!rc) rc = d_labels.need(m);
    if (!rc) rc = d_mask.need(m);
    if (!rc) rc = h_count.need((size_t)iterations + 2);
    if (!rc) rc = h_slot.need((size_t)blocks_of(m, 256 * PL_FIT_PER) * PL_SUMS);
    return rc;
}

void PlaneStore::release() {
    d_state.release(); d_flag.release(); d_pos.release(); d_cand.release(); d_hyp.release(); d_count.release(); d_slot.release();
    d_labels.release(); d_mask.release(); d_tmp.release(); h_count.release(); h_slot.release();
}

int planes_extract(const MapStore& map, hipStream_t stream, PlaneStore& st, const PlaneRule& q, const uint32_t* rank, const uint8_t* mask,
                   bool want_labels, lv_plane* planes, size_t* n_planes) {
    *n_planes = 0;
    const uint32_t ids = map.n_ids;
    if (ids == 0) return LV_OK;
    if (ids > PLANE_MAX_IDS) { set_error("map of %u ids: plane segmentation takes at most %u", ids, PLANE_MAX_IDS); return LV_EINVAL; }
    const uint32_t K = q.iterations;
    int32_t* labels = want_labels ? st.d_labels.p : nullptr;
    hipLaunchKernelGGL(planes_init_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, rank, mask, st.d_state, labels);
    LV_HIP(hipGetLastError());
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, st.d_flag.p, st.d_pos.p, (int)ids, stream));
    int rc = st.d_tmp.need(bytes ? bytes : 1);
    if (rc) return rc;
    for (uint32_t r = 0; r < q.max_planes; ++r) {
        // the candidates of the round, in map order
        hipLaunchKernelGGL(planes_flag_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, st.d_state, ids, st.d_flag);
        LV_HIP(hipGetLastError());
        LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(st.d_tmp.p, bytes, st.d_flag.p, st.d_pos.p, (int)ids, stream));
        hipLaunchKernelGGL(scan_total_kernel<uint32_t>, dim3(1), dim3(64), 0, stream, st.d_pos, st.d_flag, ids, st.d_pos + ids);
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(st.h_count + K + 1, st.d_pos + ids, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        const uint32_t n = st.h_count[K + 1];
        if (n < 3u || n < q.min_inliers) break;
        hipLaunchKernelGGL(planes_compact_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, st.d_flag, st.d_pos, st.d_cand);
        LV_HIP(hipGetLastError());
        // the hypotheses and their counts
        hipLaunchKernelGGL(planes_hyp_kernel, dim3(blocks_of(K, 256)), dim3(256), 0, stream, st.d_cand, n, q, r, st.d_hyp, st.d_count);
        LV_HIP(hipGetLastError());
        hipLaunchKernelGGL(planes_score_kernel, dim3(blocks_of(n, PL_TILE), blocks_of(K, PL_CHUNK)), dim3(PL_CHUNK), 0, stream, st.d_cand, n, st.d_hyp, K,
                           q.distance, st.d_count);
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(st.h_count, st.d_count, K * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        uint32_t best = 0, best_h = 0;
        for (uint32_t h = 0; h < K; ++h)
            if (st.h_count[h] > best) { best = st.h_count[h]; best_h = h; }
        if (best < q.min_inliers) break;   // (an invalid hypothesis counts 0 and min_inliers >= 3: no valid one ends here too)
        float4 hp[2];   // the winner's plane
        LV_HIP(hipMemcpyAsync(hp, st.d_hyp + 2 * (size_t)best_h, sizeof(hp), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        lv_plane out;
        std::memset(&out, 0, sizeof(out));
        out.normal[0] = hp[0].x; out.normal[1] = hp[0].y; out.normal[2] = hp[0].z;
        out.anchor[0] = hp[1].x; out.anchor[1] = hp[1].y; out.anchor[2] = hp[1].z;
        out.rms = std::nan("");
        out.support = best;
        out.hypothesis = best_h;
        out.candidates = n;
        if (q.refine) {
            const uint32_t nb = blocks_of(n, 256 * PL_FIT_PER);
            const PlaneArg W = {out.normal[0], out.normal[1], out.normal[2], out.anchor[0], out.anchor[1], out.anchor[2], q.distance};
            hipLaunchKernelGGL(planes_refit_kernel, dim3(nb), dim3(256), 0, stream, st.d_cand, n, W, st.d_slot);
            LV_HIP(hipGetLastError());
            LV_HIP(hipMemcpyAsync(st.h_slot, st.d_slot, (size_t)nb * PL_SUMS * sizeof(long long), hipMemcpyDeviceToHost, stream));
            LV_HIP(hipStreamSynchronize(stream));
            double m6[6], s1[3];
            const uint64_t n_fit = pl_fold(st.h_slot, nb, m6, s1);
            out.n_fit = (uint32_t)n_fit;
            if (pl_refit(n_fit, m6, s1, q.constraint, q.axis, out.normal, out.anchor, &out.rms)) out.flags |= 1u;
        }
        out.d = pl_offset(out.normal, out.anchor);
        const PlaneArg F = {out.normal[0], out.normal[1], out.normal[2], out.anchor[0], out.anchor[1], out.anchor[2], q.distance};
        hipLaunchKernelGGL(planes_classify_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, stream, st.d_cand, n, F, (int32_t)r, rank, st.d_state, labels,
                           st.d_count + K);
        LV_HIP(hipGetLastError());
        LV_HIP(hipMemcpyAsync(st.h_count + K, st.d_count + K, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        out.inliers = st.h_count[K];
        planes[(*n_planes)++] = out;
    }
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
