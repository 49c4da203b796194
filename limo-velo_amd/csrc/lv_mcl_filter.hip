// lv_mcl_filter.hip — the resident localisation filter (include/limovelo_hip.h "Resident localisation filter"; the rule's code is
// lv_mcl_filter.hpp).
//
// On the context's stream:
//   mclf_move_kernel     one lane per particle: a 16-byte load, mclf_move (nine mix chains, one sincos), a 16-byte store.
//   mclf_weigh_kernel<G> mcl_kernel's grouping (lv_mcl.hip) on the resident poses: G lanes per particle, the table in LDS once per
//                        workgroup, the workgroups stride over the particles.  Lane 0 of a group stores n_in and the accumulated
//                        score; the workgroup sends one 64-bit atomicMin for the scan's least key and one for the least eligible
//                        acc.  Both keys order totally, so neither depends on how the device reduces.
//   mclf_weights_kernel  one workgroup per block of MCLF_BLOCK particles, one lane per particle, the weight table in LDS: w, the
//                        inclusive sums of w inside the block (a shuffle scan per wavefront, the wavefronts' totals through LDS),
//                        the block's sum, and W, sum w^2, the five S sums and the two counts folded per workgroup (wave_sum, then
//                        LDS) into ONE 64-bit integer atomicAdd per sum and workgroup.  Integer sums do not depend on the order.
//   mclf_scan_kernel     one workgroup: the inclusive sums of the up to 4096 block sums, in place, 16 per lane.
//   mclf_gather_kernel   one lane per new particle: its target, a binary search over the block sums and then inside the block
//                        (mclf_ancestor), a 16-byte copy from the one pose buffer into the other, acc = 0.
// lv_occ_mcl_filter_resample copies the statistics back after mclf_weights_kernel (its one wait) and decides on the host; the scan
// and the gather run only when it resamples.  Plain stores and vector atomics only.
#include "lv_mcl_filter.hpp"

#include <cstring>

#include "lv_common.hpp"
#include "lv_mcl_lanes.hpp"

namespace lv {

namespace {

__device__ __forceinline__ void load_pose(const float* poses, uint32_t i, float (&pose)[4]) {
    const float4 v = reinterpret_cast<const float4*>(poses)[i];
    pose[0] = v.x;
    pose[1] = v.y;
    pose[2] = v.z;
    pose[3] = v.w;
}

__global__ __launch_bounds__(256) void mclf_move_kernel(float* __restrict__ poses, uint32_t K, uint64_t base, float d0, float d1, float d2, float s0,
                                                        float s1, float s2) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= K) return;
    float pose[4];
    load_pose(poses, i, pose);
    const float delta[3] = {d0, d1, d2}, sigma[3] = {s0, s1, s2};
    mclf_move(pose, base, i, delta, sigma);
    reinterpret_cast<float4*>(poses)[i] = make_float4(pose[0], pose[1], pose[2], pose[3]);
}

// in: the table (MCL_MAX_TABLE words), then the beams [B][3].  stats: the statistics block (MCLF_KEY and MCLF_SMIN are all ones).
template <int G>
__global__ __launch_bounds__(256) void mclf_weigh_kernel(MclView f, lv_mcl_params r, const uint32_t* __restrict__ table, uint32_t n_table,
                                                         const float* __restrict__ beams, int B, const float* __restrict__ poses, uint32_t K,
                                                         unsigned long long* __restrict__ acc, uint32_t* __restrict__ n_in,
                                                         unsigned long long* __restrict__ stats) {
    __shared__ uint32_t sh_table[MCL_MAX_TABLE];
    __shared__ unsigned long long sh_key[4][2];
    for (uint32_t t = threadIdx.x; t < n_table; t += 256u) sh_table[t] = table[t];
    __syncthreads();
    constexpr uint32_t PER = 256u / (uint32_t)G;   // particles per workgroup and pass
    MclLanes<G> lanes;
    lanes.g = (int)(threadIdx.x % (uint32_t)G);
    unsigned long long least = MCL_NO_SCORE, least_acc = MCL_NO_SCORE;
    // (the trip count is the same in every lane of the workgroup: the folds inside run in step)
    for (uint32_t base = blockIdx.x * PER; base < K; base += gridDim.x * PER) {
        const uint32_t q = base + threadIdx.x / (uint32_t)G;
        const bool live = q < K;
        float pose[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) load_pose(poses, q, pose);
        uint64_t s;
        uint32_t n;
        mcl_particle(f, r, pose, beams, B, sh_table, n_table, live, lanes, s, n);
        if (live && lanes.g == 0) {
            n_in[q] = n;
            const unsigned long long a = (unsigned long long)mclf_accumulate((uint64_t)acc[q], s);
            acc[q] = a;
            const unsigned long long k = (unsigned long long)mcl_key(s, q);
            if (k < least) least = k;
            if (a < least_acc) least_acc = a;
        }
    }
    least = wave_min(least);
    least_acc = wave_min(least_acc);
    if ((threadIdx.x & 63u) == 0) {
        sh_key[threadIdx.x >> 6][0] = least;
        sh_key[threadIdx.x >> 6][1] = least_acc;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long v = sh_key[0][threadIdx.x];
        for (int w = 1; w < 4; ++w)
            if (sh_key[w][threadIdx.x] < v) v = sh_key[w][threadIdx.x];
        if (v != MCL_NO_SCORE) atomicMin(&stats[MCLF_KEY + threadIdx.x], v);
    }
}

// The inclusive sums of v over the workgroup's 256 lanes in lane order; total: the workgroup's sum.  sh: 4 words, free again after
// the caller's next barrier.
template <class T>
__device__ __forceinline__ T block_scan(T v, T* sh, T& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, (unsigned int)o);
        if (lane >= (uint32_t)o) v += u;
    }
    if (lane == 63u) sh[wave] = v;
    __syncthreads();
    T before = 0;
    total = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const T s = sh[k];
        if (k < wave) before += s;
        total += s;
    }
    return v + before;
}

__global__ __launch_bounds__(256) void mclf_weights_kernel(const float* __restrict__ poses, const unsigned long long* __restrict__ acc, uint32_t K,
                                                           const uint32_t* __restrict__ wtable, uint32_t n_w, int shift, float o0, float o1, float o2,
                                                           float resolution, uint32_t* __restrict__ w_out, uint32_t* __restrict__ cin,
                                                           unsigned long long* __restrict__ cb, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t sh_w[MCLF_MAX_W];
    __shared__ uint32_t sh_scan[4];
    __shared__ unsigned long long sh_fold[4][MCLF_SUMS];
    for (uint32_t t = threadIdx.x; t < n_w; t += 256u) sh_w[t] = wtable[t];
    __syncthreads();
    const uint32_t i = blockIdx.x * MCLF_BLOCK + threadIdx.x;
    const uint64_t s_min = (uint64_t)stats[MCLF_SMIN];
    unsigned long long v[MCLF_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t w = 0;
    if (i < K) {
        float pose[4];
        load_pose(poses, i, pose);
        const uint64_t a = (uint64_t)acc[i];
        w = mclf_weight(a, s_min, shift, sh_w, n_w);
        const float origin[3] = {o0, o1, o2};
        int64_t q[5];
        const bool clamped = mclf_terms(origin, resolution, pose, q);
        v[MCLF_W] = w;
        v[MCLF_W2] = (unsigned long long)w * w;
        for (int a5 = 0; a5 < 5; ++a5) v[MCLF_S + a5] = (unsigned long long)((int64_t)w * q[a5]);
        v[MCLF_ELIGIBLE] = a != MCL_NO_SCORE ? 1u : 0u;
        v[MCLF_CLAMPED] = clamped ? 1u : 0u;
        w_out[i] = w;
    }
    uint32_t total;
    const uint32_t c = block_scan(w, sh_scan, total);
    if (i < K) cin[i] = c;
    if (threadIdx.x == 0) cb[blockIdx.x] = total;
    for (int k = 0; k < MCLF_SUMS; ++k) {
        const unsigned long long s = wave_sum(v[k]);
        if ((threadIdx.x & 63u) == 0) sh_fold[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)MCLF_SUMS) {
        const unsigned long long s = sh_fold[0][threadIdx.x] + sh_fold[1][threadIdx.x] + sh_fold[2][threadIdx.x] + sh_fold[3][threadIdx.x];
        if (s) atomicAdd(&stats[threadIdx.x], s);
    }
}

// cb [nb <= 4096]: the block sums become their inclusive sums.  The least eligible acc of the particles to come is 0.
__global__ __launch_bounds__(256) void mclf_scan_kernel(unsigned long long* __restrict__ cb, uint32_t nb, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long sh_scan[4];
    constexpr uint32_t PER = (uint32_t)(MCL_MAX_K / MCLF_BLOCK / 256u);   // 16
    unsigned long long v[PER];
    unsigned long long run = 0;
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t at = threadIdx.x * PER + k;
        run += at < nb ? cb[at] : 0ull;
        v[k] = run;
    }
    unsigned long long total;
    const unsigned long long before = block_scan(run, sh_scan, total) - run;
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t at = threadIdx.x * PER + k;
        if (at < nb) cb[at] = v[k] + before;
    }
    if (threadIdx.x == 0) stats[MCLF_SMIN] = 0ull;
}

__global__ __launch_bounds__(256) void mclf_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, uint32_t K, unsigned long long W,
                                                          unsigned long long r, const unsigned long long* __restrict__ cb, uint32_t nb,
                                                          const uint32_t* __restrict__ cin, unsigned long long* __restrict__ acc,
                                                          uint32_t* __restrict__ anc) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= K) return;
    const uint32_t a = mclf_ancestor(cb, nb, cin, K, mclf_target(j, W, r, K));   // (in 0 .. K - 1 whatever the sums hold)
    reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[a];
    acc[j] = 0ull;
    anc[j] = a;
}

template <int G>
void weigh_launch(hipStream_t stream, const MclView& f, const lv_mcl_params& r, const uint32_t* table, uint32_t n_table, const float* beams, int B,
                  const float* poses, uint32_t K, unsigned long long* acc, uint32_t* n_in, unsigned long long* stats) {
    const uint32_t blocks = grid_stride_blocks((size_t)K * (size_t)G);
    hipLaunchKernelGGL(mclf_weigh_kernel<G>, dim3(blocks), dim3(256), 0, stream, f, r, table, n_table, beams, B, poses, K, acc, n_in, stats);
}

}  // namespace

void MclFilterStore::release() {
    release_all(d_pose[0], d_pose[1], d_acc, d_n_in, d_w, d_cin, d_cb, d_anc, d_stats, h_stats, h_in, d_in);
    *this = MclFilterStore();
}

int MclFilterStore::set_poses(hipStream_t stream, const float* poses, size_t k, uint64_t sd) {
    LV_HIP(hipStreamSynchronize(stream));   // (nothing in flight reads what may be freed)
    set = false;
    int rc = need_all(4 * k, d_pose[0], d_pose[1]);
    if (!rc) rc = need_all(k, d_acc, d_n_in, d_w, d_cin, d_anc);
    if (!rc) rc = d_cb.need(blocks_of(k, MCLF_BLOCK));
    if (!rc) rc = d_stats.need(MCLF_WORDS);
    if (!rc) rc = h_stats.need(MCLF_WORDS);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(d_pose[0].p, poses, 4 * k * sizeof(float), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetAsync(d_acc.p, 0, k * sizeof(unsigned long long), stream));
    LV_HIP(hipMemsetAsync(d_n_in.p, 0, k * sizeof(uint32_t), stream));
    LV_HIP(hipMemsetAsync(d_stats.p, 0, MCLF_WORDS * sizeof(unsigned long long), stream));   // (the least acc is 0)
    LV_HIP(hipStreamSynchronize(stream));   // (the caller's poses are read)
    set = true;
    K = k;
    seed = sd;
    epoch = 0;
    since = 0;
    cur = 0;
    return LV_OK;
}

int MclFilterStore::move(hipStream_t stream, const float* delta, const float* sigma) {
    hipLaunchKernelGGL(mclf_move_kernel, dim3(blocks_of(K)), dim3(256), 0, stream, d_pose[cur].p, (uint32_t)K, mclf_base(seed, epoch), delta[0], delta[1],
                       delta[2], sigma[0], sigma[1], sigma[2]);
    LV_HIP(hipGetLastError());
    ++epoch;
    return LV_OK;
}

static MclView view_of(const DistStore& dist) {
    MclView f{};
    f.field = GridDims{dist.grid.nx, dist.grid.ny, dist.grid.nz};
    std::memcpy(f.origin, dist.origin, sizeof(f.origin));
    f.resolution = dist.grid.resolution;
    f.planar = dist.prm.planar != 0;
    f.s2 = dist.d_s2.p;
    return f;
}

int MclFilterStore::weigh(hipStream_t stream, const DistStore& dist, const lv_mcl_params& p, const float* beams, size_t B, const uint32_t* table,
                          size_t n_table, int64_t* best) {
    LV_HIP(hipStreamSynchronize(stream));   // (the pinned buffers are free: lv_buffers.hpp, THE RULE)
    const size_t n_words = MCL_MAX_TABLE + 3 * B;
    int rc = h_in.need(n_words);
    if (!rc) rc = d_in.need(n_words);
    if (rc) return rc;
    std::memset(h_in.p, 0, MCL_MAX_TABLE * sizeof(uint32_t));
    std::memcpy(h_in.p, table, n_table * sizeof(uint32_t));
    std::memcpy(h_in.p + MCL_MAX_TABLE, beams, 3 * B * sizeof(float));
    LV_HIP(hipMemcpyAsync(d_in.p, h_in.p, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetAsync(d_stats.p + MCLF_KEY, 0xFF, 2 * sizeof(unsigned long long), stream));   // (MCLF_KEY, MCLF_SMIN: all ones)

    const MclView f = view_of(dist);
    const uint32_t* d_table = d_in.p;
    const float* d_beams = reinterpret_cast<const float*>(d_in.p + MCL_MAX_TABLE);
    const float* d_poses = d_pose[cur].p;
    const uint32_t nt = (uint32_t)n_table, k = (uint32_t)K;
    const int nb = (int)B;
    switch (mcl_group(B)) {
        case 1: weigh_launch<1>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
        case 2: weigh_launch<2>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
        case 4: weigh_launch<4>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
        case 8: weigh_launch<8>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
        case 16: weigh_launch<16>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
        case 32: weigh_launch<32>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
        default: weigh_launch<64>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_acc.p, d_n_in.p, d_stats.p); break;
    }
    LV_HIP(hipGetLastError());
    ++since;
    if (best) {
        LV_HIP(hipMemcpyAsync(h_stats.p + MCLF_KEY, d_stats.p + MCLF_KEY, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        mcl_best_of((uint64_t)h_stats.p[MCLF_KEY], best);
    }
    return LV_OK;
}

int MclFilterStore::resample(hipStream_t stream, const DistStore& dist, const lv_mcl_resample_params& p, const uint32_t* wtable, size_t n_w,
                             lv_mcl_filter_stats* stats, uint32_t* ancestors) {
    LV_HIP(hipStreamSynchronize(stream));   // (the pinned buffers are free)
    int rc = h_in.need(MCL_MAX_TABLE);
    if (!rc) rc = d_in.need(MCL_MAX_TABLE);
    if (rc) return rc;
    std::memcpy(h_in.p, wtable, n_w * sizeof(uint32_t));
    LV_HIP(hipMemcpyAsync(d_in.p, h_in.p, n_w * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemsetAsync(d_stats.p, 0, MCLF_SUMS * sizeof(unsigned long long), stream));
    const uint32_t k = (uint32_t)K, nb = blocks_of(K, MCLF_BLOCK);
    hipLaunchKernelGGL(mclf_weights_kernel, dim3(nb), dim3(256), 0, stream, d_pose[cur].p, d_acc.p, k, d_in.p, (uint32_t)n_w, p.shift, dist.origin[0],
                       dist.origin[1], dist.origin[2], dist.grid.resolution, d_w.p, d_cin.p, d_cb.p, d_stats.p);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(h_stats.p, d_stats.p, MCLF_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    const uint64_t W = (uint64_t)h_stats.p[MCLF_W], sum_w2 = (uint64_t)h_stats.p[MCLF_W2];
    const bool go = mclf_decide(p.mode, W, sum_w2, (uint64_t)K, p.below_num, p.below_den);
    if (go) {
        const uint64_t r = mclf_draw(mclf_base(seed, epoch)) % W;
        hipLaunchKernelGGL(mclf_scan_kernel, dim3(1), dim3(256), 0, stream, d_cb.p, nb, d_stats.p);
        hipLaunchKernelGGL(mclf_gather_kernel, dim3(blocks_of(K)), dim3(256), 0, stream, d_pose[cur].p, d_pose[cur ^ 1].p, k, (unsigned long long)W,
                           (unsigned long long)r, d_cb.p, nb, d_cin.p, d_acc.p, d_anc.p);
        LV_HIP(hipGetLastError());
        if (ancestors) {
            LV_HIP(hipMemcpyAsync(ancestors, d_anc.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            LV_HIP(hipStreamSynchronize(stream));
        }
        cur ^= 1;
        since = 0;
    }
    ++epoch;
    *stats = lv_mcl_filter_stats{};
    stats->W = W;
    stats->sum_w2 = sum_w2;
    stats->n_eligible = (uint32_t)h_stats.p[MCLF_ELIGIBLE];
    stats->n_clamped = (uint32_t)h_stats.p[MCLF_CLAMPED];
    stats->s_min = stats->n_eligible ? (int64_t)h_stats.p[MCLF_SMIN] : -1;
    for (int a = 0; a < 5; ++a) stats->S[a] = (int64_t)h_stats.p[MCLF_S + a];
    stats->resampled = go ? 1 : 0;
    stats->epoch = epoch;
    stats->since_resample = since;
    std::memcpy(stats->origin, dist.origin, sizeof(stats->origin));
    stats->resolution = dist.grid.resolution;
    return LV_OK;
}

int MclFilterStore::get(hipStream_t stream, float* poses, uint64_t* acc, uint32_t* n_in) {
    if (poses) LV_HIP(hipMemcpyAsync(poses, d_pose[cur].p, 4 * K * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (acc) LV_HIP(hipMemcpyAsync(acc, d_acc.p, K * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (n_in) LV_HIP(hipMemcpyAsync(n_in, d_n_in.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
