// lv_mcl_filter.hpp — the resident localisation filter: a particle set that stays on the device from one cycle to the next, with the
// motion update, the measurement update, the weights, the estimate's sums and the systematic resampling (lv_occ_mcl_filter_*,
// include/limovelo_hip.h "Resident localisation filter"; kernels and host side in lv_mcl_filter.hip).
//
// The first part is the rule as plain __host__ __device__ code: the draws, a particle's move, the accumulation, a particle's weight,
// its terms of the estimate's sums, the decision, the ancestor of a new particle, and the checks.  The kernels of lv_mcl_filter.hip
// run exactly these functions; tests/emu/mcl_filter_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and
// tests/test_mcl_filter_host.py holds them to tests/mcl_filter_ref.py.  Every f32 operation stands alone (-ffp-contract=off), the
// sine and cosine are lv_sincos.hpp's polynomial, and everything after a quantisation is integer arithmetic, so every output is a
// pure function of the arguments: the same bits whatever the schedule.
#pragma once

#include "lv_mcl.hpp"

namespace lv {

constexpr size_t MCLF_MAX_W = 4096;                  // weight-table entries: 16 KiB of LDS
constexpr uint32_t MCLF_MAX_WEIGHT = 1u << 20;       // of a weight-table entry: W <= 2^40, sum w^2 <= 2^60
constexpr uint32_t MCLF_MAX_SINCE = 1u << 20;        // weigh calls since the last resampling, exclusive: acc stays below 2^60
constexpr uint32_t MCLF_MAX_EPOCH = 0xFFFFFFFFu;
constexpr uint32_t MCLF_MAX_BELOW = 65536;
constexpr uint32_t MCLF_BLOCK = 256;                 // particles per block of the prefix sums: at most 4096 blocks
constexpr float MCLF_Q_CLAMP = 4194304.0f;           // 2^22 sub-units: a sum of w * q stays below 2^62
constexpr float MCLF_PI = 3.14159274f, MCLF_TWO_PI = 6.28318548f;

// ---- the draws
// splitmix64's finaliser with its additive constant (lv_planes.hpp's pl_mix, restated: that header compiles apart)
LV_OCC_HD uint64_t mclf_mix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// what every draw of one epoch starts from
LV_OCC_HD uint64_t mclf_base(uint64_t seed, uint32_t epoch) { return mclf_mix(mclf_mix(seed) ^ (uint64_t)epoch); }
// word j (0..8) of particle i (< 2^20)
LV_OCC_HD uint64_t mclf_word(uint64_t base, uint32_t i, uint32_t j) { return mclf_mix(base ^ (((uint64_t)i << 8) | (uint64_t)j)); }
// the resampling draw of the epoch
LV_OCC_HD uint64_t mclf_draw(uint64_t base) { return mclf_mix(base ^ 0xFFFFFFFFFFFFFFFFull); }
// Standard normal n (0..2) of particle i as the integer G = 2 * (the sum of twelve 16-bit fields) - 12 * 65535: |G| < 2^20, and
// z = G * 2^-17 has unit variance (Probabilistic Robotics, table 5.4)
LV_OCC_HD int32_t mclf_normal(uint64_t base, uint32_t i, uint32_t n) {
    uint32_t sum = 0;
    for (uint32_t k = 0; k < 3; ++k) {
        const uint64_t w = mclf_word(base, i, 3u * n + k);
        sum += (uint32_t)(w & 0xFFFFu) + (uint32_t)((w >> 16) & 0xFFFFu) + (uint32_t)((w >> 32) & 0xFFFFu) + (uint32_t)(w >> 48);
    }
    return 2 * (int32_t)sum - 12 * 65535;
}

// ---- move (sample_motion_model_odometry, Probabilistic Robotics, table 5.6).  pose: (x, y, z, th), in place.
LV_OCC_HD void mclf_move(float* pose, uint64_t base, uint32_t i, const float* delta, const float* sigma) {
    const float th = pose[3];
    if (!rollout_usable(th)) return;   // (left untouched: it will score MCL_NO_SCORE)
    const float z0 = (float)mclf_normal(base, i, 0) * 0.00000762939453125f;   // 2^-17
    const float z1 = (float)mclf_normal(base, i, 1) * 0.00000762939453125f;
    const float z2 = (float)mclf_normal(base, i, 2) * 0.00000762939453125f;
    const float r1 = delta[0] - z0 * sigma[0];
    const float tr = delta[1] - z1 * sigma[1];
    const float r2 = delta[2] - z2 * sigma[2];
    const float a = th + r1;
    if (!rollout_usable(a)) {
        pose[3] = a;
        return;
    }
    float sn, cs;
    sincos_f32(a, sn, cs);
    pose[0] = pose[0] + tr * cs;
    pose[1] = pose[1] + tr * sn;
    float t = a + r2;
    if (t >= MCLF_PI) t = t - MCLF_TWO_PI;
    if (t < -MCLF_PI) t = t + MCLF_TWO_PI;
    pose[3] = t;
}

// ---- accumulate: the scores since the last resampling
LV_OCC_HD uint64_t mclf_accumulate(uint64_t acc, uint64_t score) { return (acc == MCL_NO_SCORE || score == MCL_NO_SCORE) ? MCL_NO_SCORE : acc + score; }

// ---- weights.  s_min: the least eligible acc (not read where acc is MCL_NO_SCORE)
LV_OCC_HD uint32_t mclf_weight(uint64_t acc, uint64_t s_min, int shift, const uint32_t* wtable, uint32_t n_w) {
    if (acc == MCL_NO_SCORE) return 0u;
    const uint64_t d = (acc - s_min) >> shift;
    return wtable[d < (uint64_t)(n_w - 1u) ? (uint32_t)d : n_w - 1u];
}

// ---- the estimate's terms of one particle: q[0..2] the quantised x, y, z against the field's origin and resolution, clamped to
// +-2^22 (a non-finite one counts as 0); q[3], q[4] the heading's sine and cosine in units of 2^-20 (0 for an unusable heading).
// true: an axis was clamped or zeroed.
LV_OCC_HD bool mclf_terms(const float* origin, float resolution, const float* pose, int64_t* q) {
    bool clamped = false;
    for (int a = 0; a < 3; ++a) {
        float f = occ_quant_f(pose[a], origin[a], resolution);
        if (!(fabsf(f) < __builtin_huge_valf())) {
            f = 0.0f;
            clamped = true;
        } else if (f > MCLF_Q_CLAMP) {
            f = MCLF_Q_CLAMP;
            clamped = true;
        } else if (f < -MCLF_Q_CLAMP) {
            f = -MCLF_Q_CLAMP;
            clamped = true;
        }
        q[a] = (int64_t)(int32_t)f;
    }
    q[3] = q[4] = 0;
    if (rollout_usable(pose[3])) {
        float sn, cs;
        sincos_f32(pose[3], sn, cs);
        q[3] = (int64_t)(int32_t)rintf(sn * 1048576.0f);
        q[4] = (int64_t)(int32_t)rintf(cs * 1048576.0f);
    }
    return clamped;
}

// ---- the decision (host): exactly W^2 * den < num * K * sum_w2, all below 2^97
inline bool mclf_decide(int mode, uint64_t W, uint64_t sum_w2, uint64_t K, uint32_t num, uint32_t den) {
    if (mode == 0 || W == 0) return false;
    if (mode == 2) return true;
    return (unsigned __int128)W * W * den < (unsigned __int128)sum_w2 * K * num;
}

// ---- resample: systematic, M = K.  The inclusive prefix sums C of w are kept in two levels: cin[i] = the sum of w over i's block
// of MCLF_BLOCK particles up to and including i (below 2^28), cb[b] = the sum over the blocks 0..b.
LV_OCC_HD uint64_t mclf_target(uint64_t j, uint64_t W, uint64_t r, uint64_t K) { return (j * W + r) / K; }   // (below 2^61)

// the smallest i with C_i > t, for t < W = cb[nb - 1]
LV_OCC_HD uint32_t mclf_ancestor(const unsigned long long* cb, uint32_t nb, const uint32_t* cin, uint32_t K, uint64_t t) {
    uint32_t lo = 0, hi = nb - 1u;   // the smallest block b with cb[b] > t
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)cb[mid] > t) hi = mid; else lo = mid + 1u;
    }
    const uint32_t b = lo;
    const uint64_t rest = t - (b ? (uint64_t)cb[b - 1u] : 0u);   // (below the block's sum)
    lo = b * MCLF_BLOCK;
    hi = lo + MCLF_BLOCK - 1u < K - 1u ? lo + MCLF_BLOCK - 1u : K - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)cin[mid] > rest) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

inline void default_mcl_resample_params(lv_mcl_resample_params* p) {
    if (!p) return;
    *p = lv_mcl_resample_params{};
    p->shift = 0;
    p->mode = 1;
    p->below_num = 1;
    p->below_den = 2;
}

// ---- the checks: everything that can be judged without a context.  NULL when it holds, otherwise what is wrong (LV_EINVAL)
inline const char* mclf_check_set(const float* poses, size_t K) {
    if (K < 1 || K > MCL_MAX_K) return "K: 1..2^20";
    if (!poses) return "null poses";
    return nullptr;
}

inline const char* mclf_check_move(const float* delta, const float* sigma) {
    if (!delta) return "null delta";
    if (!sigma) return "null sigma";
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(delta[a]) < __builtin_huge_valf())) return "delta: finite";
    for (int a = 0; a < 3; ++a)
        if (!(sigma[a] >= 0.0f && sigma[a] < __builtin_huge_valf())) return "sigma: finite and >= 0";
    return nullptr;
}

// (K is the store's: K * B is judged by mclf_check_pairs once there are particles)
inline const char* mclf_check_weigh(const lv_mcl_params* p, const float* beams, size_t B, const uint32_t* table, size_t n_table) {
    if (!p) return "null params";
    if (B < 1 || B > MCL_MAX_B) return "B: 1..65536";
    if (n_table < 1 || n_table > MCL_MAX_TABLE) return "n_table: 1..4096";
    if (p->out_cost > MCL_MAX_COST) return "out_cost: 0..2^24";
    if (p->min_inside < 0 || (size_t)p->min_inside > B) return "min_inside: 0..B";
    if (!beams) return "null beams";
    if (!table) return "null table";
    for (size_t t = 0; t < n_table; ++t)
        if (table[t] > MCL_MAX_COST) return "table: every entry 0..2^24";
    return nullptr;
}
inline const char* mclf_check_pairs(size_t K, size_t B) { return K * B > MCL_MAX_PAIRS ? "K * B: at most 2^30" : nullptr; }

inline const char* mclf_check_resample(const lv_mcl_resample_params* p, const uint32_t* wtable, size_t n_w, const void* stats) {
    if (!p) return "null params";
    if (p->shift < 0 || p->shift > 63) return "shift: 0..63";
    if (p->mode < 0 || p->mode > 2) return "mode: 0 (never), 1 (below the threshold) or 2 (always)";
    if (p->below_num < 1 || p->below_num > p->below_den || p->below_den > MCLF_MAX_BELOW) return "below: 1 <= below_num <= below_den <= 65536";
    if (n_w < 1 || n_w > MCLF_MAX_W) return "n_w: 1..4096";
    if (!wtable) return "null wtable";
    for (size_t t = 0; t < n_w; ++t)
        if (wtable[t] > MCLF_MAX_WEIGHT) return "wtable: every entry 0..2^20";
    if (!stats) return "null stats";
    return nullptr;
}

inline const char* mclf_check_get(const void* poses, const void* acc, const void* n_in) {
    return (!poses && !acc && !n_in) ? "poses, acc and n_in are all null" : nullptr;
}

// the states of a store that has particles (LV_ESTATE); NULL: the call may run
inline const char* mclf_state_epoch(uint32_t epoch) {
    return epoch == MCLF_MAX_EPOCH ? "the epoch has reached 2^32 - 1: call lv_occ_mcl_filter_set again" : nullptr;
}
inline const char* mclf_state_since(uint32_t since) {
    return since >= MCLF_MAX_SINCE - 1u ? "2^20 scans since the last resampling: call lv_occ_mcl_filter_resample" : nullptr;
}

// ---- the store.  Nothing is allocated before lv_occ_mcl_filter_set; lv_occ_mcl_filter_clear and lv_destroy free everything.
// The statistics block, as 64-bit words:
enum { MCLF_W = 0, MCLF_W2 = 1, MCLF_S = 2, MCLF_ELIGIBLE = 7, MCLF_CLAMPED = 8, MCLF_SUMS = 9, MCLF_KEY = 9, MCLF_SMIN = 10, MCLF_WORDS = 16 };

struct MclFilterStore {
    bool set = false;
    size_t K = 0;
    uint64_t seed = 0;
    uint32_t epoch = 0;
    uint32_t since = 0;                       // weigh calls since the last resampling
    int cur = 0;                              // which pose buffer holds the particles
    DevBuf<float> d_pose[2];                  // [K] float4 each: the resampling gathers from one into the other
    DevBuf<unsigned long long> d_acc;         // [K]
    DevBuf<uint32_t> d_n_in;                  // [K]
    DevBuf<uint32_t> d_w;                     // [K]
    DevBuf<uint32_t> d_cin;                   // [K] the inclusive sums of w inside a block
    DevBuf<unsigned long long> d_cb;          // [blocks] the block sums, then their inclusive sums
    DevBuf<uint32_t> d_anc;                   // [K]
    DevBuf<unsigned long long> d_stats;       // MCLF_WORDS
    PinBuf<unsigned long long> h_stats;
    PinBuf<uint32_t> h_in;                    // a call's table (MCL_MAX_TABLE words), then the beams
    DevBuf<uint32_t> d_in;

    int set_poses(hipStream_t stream, const float* poses, size_t K, uint64_t seed);
    int move(hipStream_t stream, const float* delta, const float* sigma);
    int weigh(hipStream_t stream, const DistStore& dist, const lv_mcl_params& p, const float* beams, size_t B, const uint32_t* table, size_t n_table,
              int64_t* best);
    int resample(hipStream_t stream, const DistStore& dist, const lv_mcl_resample_params& p, const uint32_t* wtable, size_t n_w,
                 lv_mcl_filter_stats* stats, uint32_t* ancestors);
    int get(hipStream_t stream, float* poses, uint64_t* acc, uint32_t* n_in);
    void release();
};

}  // namespace lv
