// lv_mcl.hip — Monte Carlo localisation on the distance field (include/limovelo_hip.h "Localisation"; the rule's code is
// lv_mcl.hpp).
//
// On the context's stream:
//   mcl_kernel<G>   a group of G lanes per particle, G the power of two >= B and at most 64: 256 / G particles per workgroup and
//                   pass.  The workgroups stride over the particles (at most GRID_STRIDE_BLOCKS of them), so the table is copied
//                   into LDS once per workgroup, not once per 256 / G particles.  Every lane of a group runs mcl_particle on the
//                   same particle: it reads the pose by one 16-byte load and computes the sine and cosine itself; lane g takes the
//                   beams g, g + G, ... (the lanes of a group read consecutive beams, and every group reads the same ones), looks
//                   the end point's cell up in the field (a gather of int32) and the cost up in LDS.  The group's 64-bit sum and
//                   its count are group_fold<G> (wave_sum when G = 64).  Lane 0 of a group stores score and n_in and keeps the
//                   least key (score << 20 | index) of its particles; the workgroup's least key goes out in one 64-bit atomicMin.
//                   The key orders (score, index) totally, so `best` does not depend on how the device reduces.
// The call's key is set to all ones from the pinned word before the kernel runs.
#include "lv_mcl.hpp"

#include <cstring>

#include "lv_common.hpp"
#include "lv_mcl_lanes.hpp"

namespace lv {

namespace {

// in: the table (MCL_MAX_TABLE words), the beams [B][3], the poses [K][4] (16-byte aligned: MclStore::run pads the beams).
// key: the call's least key.
template <int G>
__global__ __launch_bounds__(256) void mcl_kernel(MclView f, lv_mcl_params r, const uint32_t* __restrict__ table, uint32_t n_table,
                                                  const float* __restrict__ beams, int B, const float* __restrict__ poses, uint32_t K,
                                                  unsigned long long* __restrict__ score, uint32_t* __restrict__ n_in,
                                                  unsigned long long* __restrict__ key) {
    __shared__ uint32_t sh_table[MCL_MAX_TABLE];
    __shared__ unsigned long long sh_key[4];
    for (uint32_t t = threadIdx.x; t < n_table; t += 256u) sh_table[t] = table[t];
    __syncthreads();
    constexpr uint32_t PER = 256u / (uint32_t)G;   // particles per workgroup and pass
    MclLanes<G> lanes;
    lanes.g = (int)(threadIdx.x % (uint32_t)G);
    unsigned long long least = MCL_NO_SCORE;
    // (the trip count is the same in every lane of the workgroup: the folds inside run in step)
    for (uint32_t base = blockIdx.x * PER; base < K; base += gridDim.x * PER) {
        const uint32_t q = base + threadIdx.x / (uint32_t)G;
        const bool live = q < K;
        float pose[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            const float4 v = reinterpret_cast<const float4*>(poses)[q];
            pose[0] = v.x;
            pose[1] = v.y;
            pose[2] = v.z;
            pose[3] = v.w;
        }
        uint64_t s;
        uint32_t n;
        mcl_particle(f, r, pose, beams, B, sh_table, n_table, live, lanes, s, n);
        if (live && lanes.g == 0) {
            score[q] = (unsigned long long)s;
            n_in[q] = n;
            const unsigned long long k = (unsigned long long)mcl_key(s, q);
            if (k < least) least = k;
        }
    }
    least = wave_min(least);
    if ((threadIdx.x & 63u) == 0) sh_key[threadIdx.x >> 6] = least;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sh_key[w] < least) least = sh_key[w];
        if (least != MCL_NO_SCORE) atomicMin(key, least);
    }
}

template <int G>
void mcl_launch(hipStream_t stream, const MclView& f, const lv_mcl_params& r, const uint32_t* table, uint32_t n_table, const float* beams, int B,
                const float* poses, uint32_t K, unsigned long long* score, uint32_t* n_in, unsigned long long* key) {
    const uint32_t blocks = grid_stride_blocks((size_t)K * (size_t)G);
    hipLaunchKernelGGL(mcl_kernel<G>, dim3(blocks), dim3(256), 0, stream, f, r, table, n_table, beams, B, poses, K, score, n_in, key);
}

}  // namespace

void MclStore::release() {
    h_in.release(); d_in.release(); d_score.release(); d_n_in.release(); h_best.release();
    *this = MclStore();
}

int MclStore::run(hipStream_t stream, const DistStore& dist, const lv_mcl_params& p, const float* poses, size_t K, const float* beams, size_t B,
                  const uint32_t* table, size_t n_table, uint64_t* score, uint32_t* n_in, int64_t* best) {
    if (K == 0) {
        if (best) best[0] = best[1] = -1;
        return LV_OK;
    }
    LV_HIP(hipStreamSynchronize(stream));   // (the pinned buffers are free: lv_buffers.hpp, THE RULE)
    const size_t n_beams = (3 * B + 3) & ~(size_t)3;   // padded: the poses start on a 16-byte boundary
    const size_t at_beams = MCL_MAX_TABLE, at_poses = at_beams + n_beams, n_words = at_poses + 4 * K;
    int rc = h_in.need(n_words);
    if (!rc) rc = d_in.need(n_words);
    if (!rc) rc = d_score.need(K + 1);
    if (!rc) rc = d_n_in.need(K);
    if (!rc) rc = h_best.need(2);
    if (rc) return rc;
    std::memset(h_in.p, 0, at_poses * sizeof(uint32_t));
    std::memcpy(h_in.p, table, n_table * sizeof(uint32_t));
    std::memcpy(h_in.p + at_beams, beams, 3 * B * sizeof(float));
    std::memcpy(h_in.p + at_poses, poses, 4 * K * sizeof(float));
    h_best.p[0] = MCL_NO_SCORE;
    LV_HIP(hipMemcpyAsync(d_in.p, h_in.p, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    LV_HIP(hipMemcpyAsync(d_score.p + K, h_best.p, sizeof(unsigned long long), hipMemcpyHostToDevice, stream));

    MclView f{};
    f.field = GridDims{dist.grid.nx, dist.grid.ny, dist.grid.nz};
    std::memcpy(f.origin, dist.origin, sizeof(f.origin));
    f.resolution = dist.grid.resolution;
    f.planar = dist.prm.planar != 0;
    f.s2 = dist.d_s2.p;
    const uint32_t* d_table = d_in.p;
    const float* d_beams = reinterpret_cast<const float*>(d_in.p + at_beams);
    const float* d_poses = reinterpret_cast<const float*>(d_in.p + at_poses);
    const uint32_t nt = (uint32_t)n_table, k = (uint32_t)K;
    const int nb = (int)B;
    unsigned long long* d_key = d_score.p + K;
    switch (mcl_group(B)) {
        case 1: mcl_launch<1>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
        case 2: mcl_launch<2>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
        case 4: mcl_launch<4>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
        case 8: mcl_launch<8>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
        case 16: mcl_launch<16>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
        case 32: mcl_launch<32>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
        default: mcl_launch<64>(stream, f, p, d_table, nt, d_beams, nb, d_poses, k, d_score.p, d_n_in.p, d_key); break;
    }
    LV_HIP(hipGetLastError());
    if (score) LV_HIP(hipMemcpyAsync(score, d_score.p, K * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (n_in) LV_HIP(hipMemcpyAsync(n_in, d_n_in.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipMemcpyAsync(h_best.p + 1, d_key, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    if (best) mcl_best_of((uint64_t)h_best.p[1], best);
    return LV_OK;
}

}  // namespace lv
