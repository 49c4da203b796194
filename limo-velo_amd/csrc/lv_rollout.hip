// lv_rollout.hip — trajectory rollouts on the plan and the distance field (include/limovelo_hip.h "Rollouts"; the rule's code is
// lv_rollout.hpp).
//
// On the context's stream:
//   rollout_kernel<G>    a group of G lanes per sequence, G the power of two >= max(1, n_fp): 256 / G sequences per workgroup.
//                        Every lane of a group runs rollout_sequence on the same sequence and gets the same pose bits; lane g
//                        holds footprint point g in registers and judges it, and the group's verdict is group_min of the
//                        lanes' (reason, point) keys.  The step loop is a recurrence; a wavefront leaves it once the ballot
//                        says that every group in it has stopped.  Controls are read by one 8-byte load per lane and step
//                        while s <= Tc (staging tiles of steps through LDS was measured and was no faster: DESIGN.md).  Lane 0 of a group stores the poses as it goes, then the record as two 16-byte stores
//                        and the score; the workgroup's least (score, index) goes to d_part[block].
//   rollout_best_kernel  one workgroup folds the workgroups' entries into the call's.  Both folds take the least by
//                        rollout_before, a total order: the result does not depend on how the device reduces.
// The pose rows are filled with the NaN pattern before the kernel runs; it stores rows 0..n_ok only.
#include "lv_rollout.hpp"

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

template <int G>
struct RolloutLanes {
    int g;
    float fx, fy;   // footprint point g
    // one 8-byte load: the pairs of a sequence start on an 8-byte boundary of the input buffer
    __device__ void control(const float* ctrl, int s, float& v, float& w) const {
        const float2 u = reinterpret_cast<const float2*>(ctrl)[s - 1];
        v = u.x;
        w = u.y;
    }
    __device__ bool any(bool alive) const { return __ballot(alive) != 0ull; }
    __device__ uint32_t fold(uint32_t key) const { return group_min<G>(key); }
    __device__ int first() const { return g; }
    __device__ int stride() const { return G; }
    __device__ void point(const float*, int, float& x, float& y) const {
        x = fx;
        y = fy;
    }
    __device__ bool writes() const { return g == 0; }
};

struct RolloutStart {
    float v[3];
};

// the least (score, index) of the workgroup into threads 0's (s, i); sh: one slot per wavefront
__device__ __forceinline__ void rollout_block_best(unsigned long long (&sh_s)[4], uint32_t (&sh_i)[4], unsigned long long& s, uint32_t& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long so = __shfl_xor(s, o);
        const uint32_t io = __shfl_xor(i, o);
        if (rollout_before(so, io, s, i)) {
            s = so;
            i = io;
        }
    }
    if ((threadIdx.x & 63u) == 0) {
        sh_s[threadIdx.x >> 6] = s;
        sh_i[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w)
            if (rollout_before(sh_s[w], sh_i[w], s, i)) {
                s = sh_s[w];
                i = sh_i[w];
            }
}

// in: the footprint (2 * ROLL_MAX_FP floats), then the controls [K][Tc][2].  poses: NULL, or K x (T + 1) x 3 floats.
// part: per workgroup (score, index) as two 64-bit words.
template <int G>
__global__ __launch_bounds__(256) void rollout_kernel(RolloutView f, lv_rollout_params r, int n_fp, RolloutStart start, const float* __restrict__ in,
                                                      uint32_t K, lv_rollout_result* __restrict__ res, unsigned long long* __restrict__ score,
                                                      float* __restrict__ poses, unsigned long long* __restrict__ part) {
    __shared__ unsigned long long sh_s[4];
    __shared__ uint32_t sh_i[4];
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    const uint32_t seq = id / (uint32_t)G;
    const bool live = seq < K;
    RolloutLanes<G> lanes;
    lanes.g = (int)(id % (uint32_t)G);
    lanes.fx = lanes.fy = 0.0f;
    if (lanes.g < n_fp) {
        lanes.fx = in[2 * lanes.g];
        lanes.fy = in[2 * lanes.g + 1];
    }
    const float* ctrl = in + 2 * ROLL_MAX_FP + (size_t)(live ? seq : 0u) * (size_t)r.Tc * 2u;
    float* rows = poses ? poses + (size_t)(live ? seq : 0u) * (size_t)(r.T + 1) * 3u : nullptr;
    lv_rollout_result o;
    rollout_sequence(f, r, n_fp, start.v, ctrl, nullptr, live, lanes, o, rows);
    unsigned long long s = ROLL_NO_SCORE;
    uint32_t i = 0xFFFFFFFFu;
    if (live && lanes.g == 0) {
        s = rollout_score(r, o);
        i = seq;
        int4* q = reinterpret_cast<int4*>(res + seq);
        q[0] = make_int4(o.status, o.steps, o.why, o.cell_end);
        q[1] = make_int4((int)o.p_end, (int)o.p_min, o.s_min, (int)o.cost_sum);
        score[seq] = s;
    }
    rollout_block_best(sh_s, sh_i, s, i);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s;
        part[2 * (size_t)blockIdx.x + 1] = i;
    }
}

// part: n entries, then the call's (one workgroup of 256)
__global__ __launch_bounds__(256) void rollout_best_kernel(unsigned long long* __restrict__ part, uint32_t n) {
    __shared__ unsigned long long sh_s[4];
    __shared__ uint32_t sh_i[4];
    unsigned long long s = ROLL_NO_SCORE;
    uint32_t i = 0xFFFFFFFFu;
    for (uint32_t e = threadIdx.x; e < n; e += 256u) {
        const unsigned long long se = part[2 * (size_t)e];
        const uint32_t ie = (uint32_t)part[2 * (size_t)e + 1];
        if (rollout_before(se, ie, s, i)) {
            s = se;
            i = ie;
        }
    }
    rollout_block_best(sh_s, sh_i, s, i);
    if (threadIdx.x == 0) {
        part[2 * (size_t)n] = s;
        part[2 * (size_t)n + 1] = s == ROLL_NO_SCORE ? ~0ull : (unsigned long long)i;
    }
}

template <int G>
void rollout_launch(hipStream_t stream, uint32_t blocks, const RolloutView& f, const lv_rollout_params& r, int n_fp, const RolloutStart& start,
                    const float* in, uint32_t K, lv_rollout_result* res, unsigned long long* score, float* poses, unsigned long long* part) {
    hipLaunchKernelGGL(rollout_kernel<G>, dim3(blocks), dim3(256), 0, stream, f, r, n_fp, start, in, K, res, score, poses, part);
}

}  // namespace

void RolloutStore::release() {
    h_in.release(); d_in.release(); d_res.release(); d_score.release(); d_poses.release(); d_part.release(); h_best.release();
    *this = RolloutStore();
}

int RolloutStore::run(hipStream_t stream, const PlanStore& plan, const DistStore& dist, const lv_rollout_params& p, const float start[3],
                      const float* controls, size_t K, const float* footprint, size_t n_fp, lv_rollout_result* results, float* poses,
                      uint64_t* score, int64_t* best) {
    if (K == 0) {
        if (best) best[0] = best[1] = -1;
        return LV_OK;
    }
    LV_HIP(hipStreamSynchronize(stream));   // (the pinned buffers are free: lv_buffers.hpp, THE RULE)
    const int G = rollout_group(n_fp);
    const size_t n_ctrl = K * (size_t)p.Tc * 2, n_in = 2 * ROLL_MAX_FP + n_ctrl, n_rows = K * (size_t)(p.T + 1) * 3;
    const uint32_t blocks = blocks_of(K * (size_t)G);
    int rc = h_in.need(n_in);
    if (!rc) rc = d_in.need(n_in);
    if (!rc) rc = d_res.need(K);
    if (!rc) rc = d_score.need(K);
    if (!rc) rc = d_part.need(2 * ((size_t)blocks + 1));
    if (!rc) rc = h_best.need(2);
    if (!rc && poses) rc = d_poses.need(n_rows);
    if (rc) return rc;
    std::memset(h_in.p, 0, 2 * ROLL_MAX_FP * sizeof(float));
    if (n_fp) std::memcpy(h_in.p, footprint, 2 * n_fp * sizeof(float));
    std::memcpy(h_in.p + 2 * ROLL_MAX_FP, controls, n_ctrl * sizeof(float));
    LV_HIP(hipMemcpyAsync(d_in.p, h_in.p, n_in * sizeof(float), hipMemcpyHostToDevice, stream));
    if (poses) LV_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_poses.p), (int)ROLL_NAN_BITS, n_rows, stream));

    RolloutView f{};
    f.plan = plan.grid;
    f.cost = plan.d_cost.p;
    f.pot = plan.d_pot.p;
    if (n_fp) {
        f.field = GridDims{dist.grid.nx, dist.grid.ny, 1};
        std::memcpy(f.f_origin, dist.origin, sizeof(f.f_origin));
        f.f_resolution = dist.grid.resolution;
        f.s2 = dist.d_s2.p;
    }
    RolloutStart s0{{start[0], start[1], start[2]}};
    float* d_rows = poses ? d_poses.p : nullptr;
    const int nf = (int)n_fp;
    switch (G) {
        case 1: rollout_launch<1>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
        case 2: rollout_launch<2>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
        case 4: rollout_launch<4>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
        case 8: rollout_launch<8>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
        case 16: rollout_launch<16>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
        case 32: rollout_launch<32>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
        default: rollout_launch<64>(stream, blocks, f, p, nf, s0, d_in.p, (uint32_t)K, d_res.p, d_score.p, d_rows, d_part.p); break;
    }
    LV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rollout_best_kernel, dim3(1), dim3(256), 0, stream, d_part.p, blocks);
    LV_HIP(hipGetLastError());
    if (results) LV_HIP(hipMemcpyAsync(results, d_res.p, K * sizeof(lv_rollout_result), hipMemcpyDeviceToHost, stream));
    if (score) LV_HIP(hipMemcpyAsync(score, d_score.p, K * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (poses) LV_HIP(hipMemcpyAsync(poses, d_poses.p, n_rows * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipMemcpyAsync(h_best.p, d_part.p + 2 * (size_t)blocks, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    if (best) {
        best[0] = (int64_t)h_best.p[1];
        best[1] = (int64_t)h_best.p[0];
    }
    return LV_OK;
}

}  // namespace lv
