// lv_rollout.hpp — trajectory rollouts on the plan and the distance field (lv_occ_rollout, include/limovelo_hip.h "Rollouts"; kernels
// and host side in lv_rollout.hip).
//
// The first part is the rule as plain __host__ __device__ code: which heading is usable, one step of the motion model, the test of
// a pose and of a footprint point, one whole sequence, its score and the order `best` is chosen by.  The kernel of lv_rollout.hip
// runs exactly these functions; tests/emu/occ_rollout_emu.cpp compiles them with g++ through tests/emu/hip/hip_runtime.h and
// tests/test_occ_rollout_host.py holds them to tests/rollout_ref.py.  Every f32 operation stands alone (-ffp-contract=off) and the
// sine and cosine are lv_sincos.hpp's one polynomial, so the three agree on the bits of every pose.
//
// rollout_sequence is written for a GROUP of lanes that serve one sequence: every lane integrates the pose itself (the same
// operations give the same bits, nothing is broadcast), lane g judges the footprint points g, g + stride, ..., and the group's
// verdict is a fold of the lanes' keys.  What a group is comes in through the Lanes argument:
//   bool any(bool alive)             some lane that runs in step with this one is still rolling (the device: its wavefront)
//   uint32_t fold(uint32_t key)      the least key of the group; every lane of the group calls it in every step
//   void control(ctrl, s, v, w)      the sequence's pair of step s <= Tc
//   int first(), int stride()        the footprint points this lane judges
//   void point(fp, q, fx, fy)        footprint point q
//   bool writes()                    this lane stores the group's poses
// The host emulation is a group of one lane.
#pragma once

#include "lv_plan.hpp"
#include "lv_sincos.hpp"

namespace lv {

constexpr int ROLL_MAX_T = 1024;
constexpr size_t ROLL_MAX_K = (size_t)1 << 20;
constexpr size_t ROLL_MAX_FP = 64;
constexpr uint32_t ROLL_MAX_WEIGHT = 65535u;
constexpr size_t ROLL_MAX_PAIRS = (size_t)1 << 24;   // K * Tc, and K * (T + 1) when poses are asked for
constexpr float ROLL_TH_LIMIT = 1048576.0f;       // 2^20: below it sincos_f32's (int)k is defined
constexpr uint32_t ROLL_NAN_BITS = 0x7FC00000u;   // every float of a pose row past n_ok
constexpr uint32_t ROLL_NO_FAIL = 0xFFFFFFFFu;    // a lane's key when none of its footprint points fails
constexpr uint64_t ROLL_NO_SCORE = 0xFFFFFFFFFFFFFFFFull;

// What a rollout reads: the plan's cells, and with a footprint the field's
struct RolloutView {
    PlanGrid plan;          // planar
    const uint8_t* cost;
    const uint32_t* pot;
    GridDims field;         // nz = 1
    float f_origin[3];
    float f_resolution;
    const int32_t* s2;      // NULL with n_fp = 0
};

LV_OCC_HD bool rollout_usable(float th) { return fabsf(th) < ROLL_TH_LIMIT; }   // (NaN fails)

// the plan's cell of (x, y), -1 if it has none
LV_OCC_HD int32_t rollout_cell(const PlanGrid& g, float x, float y) {
    const float p[3] = {x, y, 0.0f};
    int i, j, k;
    return plan_cell_of(g, p, i, j, k) ? (int32_t)grid_at(g, i, j, k) : -1;
}

struct RolloutPose {
    float x, y, th;
    float sn, cs;   // of th; not set while th is not usable
};

LV_OCC_HD void rollout_start(const float start[3], RolloutPose& a) {
    a.x = start[0];
    a.y = start[1];
    a.th = start[2];
    a.sn = a.cs = 0.0f;
    if (rollout_usable(a.th)) sincos_f32(a.th, a.sn, a.cs);
}

// Pose s from pose s - 1 under (v, w): 0 when it passes reasons 1..4, otherwise the first of them that applies.  With 0, b is the
// pose with the sine and cosine of its heading, cell its cell in the plan and cost that cell's byte.
LV_OCC_HD int rollout_step(const RolloutView& f, const RolloutPose& a, float v, float w, float dt, RolloutPose& b, int32_t& cell, uint32_t& cost) {
    if (!rollout_usable(a.th)) return 1;
    const float d = v * dt;
    b.x = a.x + d * a.cs;
    b.y = a.y + d * a.sn;
    b.th = a.th + w * dt;
    if (!rollout_usable(b.th)) return 2;
    cell = rollout_cell(f.plan, b.x, b.y);
    if (cell < 0) return 3;
    cost = f.cost[cell];
    if (cost == 0) return 4;
    sincos_f32(b.th, b.sn, b.cs);
    return 0;
}

// Footprint point (fx, fy) of pose b: 0 when it passes, else 5 or 6
LV_OCC_HD int rollout_point(const RolloutView& f, const RolloutPose& b, float fx, float fy, int32_t fp_clear_s2) {
    const float p[3] = {b.x + (b.cs * fx - b.sn * fy), b.y + (b.sn * fx + b.cs * fy), 0.0f};
    int i, j, k;
    if (!grid_cell_of(f.field, f.f_origin, f.f_resolution, true, p, i, j, k)) return 5;
    return f.s2[grid_at(f.field, i, j, k)] < fp_clear_s2 ? 6 : 0;
}

// a lane's key for a failing point: the lowest reason wins, then the lowest point
LV_OCC_HD uint32_t rollout_key(int reason, int q) { return ((uint32_t)reason << 8) | (uint32_t)q; }

LV_OCC_HD void rollout_put_pose(float* rows, int s, const RolloutPose& a) {
    rows[3 * s + 0] = a.x;
    rows[3 * s + 1] = a.y;
    rows[3 * s + 2] = a.th;
}

// One sequence.  live: false for a lane that has no sequence and only keeps its group's folds company.  ctrl: the sequence's Tc
// pairs; fp: the footprint; rows: the sequence's T + 1 pose rows or NULL (rows past n_ok are not touched).
template <class Lanes>
LV_OCC_HD void rollout_sequence(const RolloutView& f, const lv_rollout_params& r, int n_fp, const float start[3], const float* ctrl, const float* fp,
                                bool live, const Lanes& lanes, lv_rollout_result& out, float* rows) {
    RolloutPose a;
    rollout_start(start, a);
    int32_t steps = 0, why = 0, cell_end = -1, s_min = -1;
    uint32_t p_end = PLAN_UNREACHED, p_min = PLAN_UNREACHED, cost_sum = 0;
    if (live) {
        cell_end = rollout_cell(f.plan, a.x, a.y);
        if (cell_end >= 0) {
            p_end = p_min = f.pot[cell_end];
            s_min = 0;
        }
        if (rows && lanes.writes()) rollout_put_pose(rows, 0, a);
    }
    bool alive = live;
    float v = 0.0f, w = 0.0f;
    for (int s = 1; s <= r.T; ++s) {
        if (!lanes.any(alive)) break;
        RolloutPose b = a;
        int32_t cell = -1;
        uint32_t cost = 0, key = ROLL_NO_FAIL;
        int bad = 0;
        if (alive) {
            if (s <= r.Tc) lanes.control(ctrl, s, v, w);
            bad = rollout_step(f, a, v, w, r.dt, b, cell, cost);
            if (!bad) {
                for (int q = lanes.first(); q < n_fp; q += lanes.stride()) {
                    float fx, fy;
                    lanes.point(fp, q, fx, fy);
                    const int e = rollout_point(f, b, fx, fy, r.fp_clear_s2);
                    if (e && rollout_key(e, q) < key) key = rollout_key(e, q);
                }
            }
        }
        key = lanes.fold(key);
        if (alive) {
            if (!bad && key != ROLL_NO_FAIL) bad = (int)(key >> 8);
            if (bad) {
                why = bad;
                alive = false;
            } else {
                a = b;
                steps = s;
                cost_sum += cost;
                cell_end = cell;
                p_end = f.pot[cell];
                if (s_min < 0 || p_end < p_min) {
                    p_min = p_end;
                    s_min = s;
                }
                if (rows && lanes.writes()) rollout_put_pose(rows, s, a);
            }
        }
    }
    out.status = why ? LV_ROLLOUT_STOPPED : LV_ROLLOUT_CLEAR;
    out.steps = steps;
    out.why = why;
    out.cell_end = cell_end;
    out.p_end = p_end;
    out.p_min = p_min;
    out.s_min = s_min;
    out.cost_sum = cost_sum;
}

// ROLL_NO_SCORE: not eligible
LV_OCC_HD uint64_t rollout_score(const lv_rollout_params& r, const lv_rollout_result& o) {
    const uint32_t p_sel = r.goal_mode ? o.p_min : o.p_end;
    if (o.steps < r.min_steps || p_sel == PLAN_UNREACHED) return ROLL_NO_SCORE;
    return (uint64_t)r.w_cost * o.cost_sum + (uint64_t)r.w_goal * p_sel + (uint64_t)r.w_stop * (uint64_t)(r.T - o.steps);
}

// (score, index) a before b: `best` is the least by this order, so it does not depend on the order of the fold
LV_OCC_HD bool rollout_before(uint64_t sa, uint32_t ia, uint64_t sb, uint32_t ib) { return sa < sb || (sa == sb && ia < ib); }

// The group of one lane (the host emulation, the timing's CPU baseline)
struct RolloutOneLane {
    LV_OCC_HD bool any(bool alive) const { return alive; }
    LV_OCC_HD uint32_t fold(uint32_t key) const { return key; }
    LV_OCC_HD void control(const float* ctrl, int s, float& v, float& w) const {
        v = ctrl[2 * (s - 1)];
        w = ctrl[2 * (s - 1) + 1];
    }
    LV_OCC_HD int first() const { return 0; }
    LV_OCC_HD int stride() const { return 1; }
    LV_OCC_HD void point(const float* fp, int q, float& fx, float& fy) const {
        fx = fp[2 * q];
        fy = fp[2 * q + 1];
    }
    LV_OCC_HD bool writes() const { return true; }
};

inline void default_rollout_params(lv_rollout_params* p) {
    if (!p) return;
    *p = lv_rollout_params{};
    p->T = 32;
    p->Tc = 1;
    p->dt = 0.1f;
    p->fp_clear_s2 = 1;
    p->w_cost = 1;
    p->w_goal = 1;
    p->w_stop = 0;
    p->min_steps = 1;
    p->goal_mode = 0;
}

// Everything that can be judged without a context: NULL when it holds, otherwise what is wrong (lv_occ_rollout: LV_EINVAL)
inline const char* rollout_check(const lv_rollout_params* p, const float* start, const float* controls, size_t K, const float* footprint,
                                 size_t n_fp, const void* results, const void* poses, const void* score, const void* best) {
    if (!p) return "null params";
    if (p->T < 1 || p->T > ROLL_MAX_T) return "T: 1..1024";
    if (p->Tc < 1 || p->Tc > p->T) return "Tc: 1..T";
    if (!(p->dt > 0.0f && p->dt < __builtin_huge_valf())) return "dt: finite and > 0";
    if (n_fp > ROLL_MAX_FP) return "n_fp: 0..64";
    if (n_fp && !footprint) return "null footprint with n_fp > 0";
    if (p->fp_clear_s2 < 1 || p->fp_clear_s2 > PLAN_MAX_CLEAR) return "fp_clear_s2: 1..3 * 1023^2";
    if (p->min_steps < 0 || p->min_steps > p->T) return "min_steps: 0..T";
    if (p->goal_mode != 0 && p->goal_mode != 1) return "goal_mode: 0 or 1";
    if (p->w_cost > ROLL_MAX_WEIGHT || p->w_goal > ROLL_MAX_WEIGHT || p->w_stop > ROLL_MAX_WEIGHT) return "weights: 0..65535";
    if (K > ROLL_MAX_K) return "K: 0..2^20";
    if (K * (size_t)p->Tc > ROLL_MAX_PAIRS) return "K * Tc: at most 2^24 pairs";
    if (poses && K * (size_t)(p->T + 1) > ROLL_MAX_PAIRS) return "K * (T + 1): at most 2^24 pose rows";
    if (!start) return "null start";
    if (K && !controls) return "null controls with K > 0";
    if (!results && !poses && !score && !best) return "results, poses, score and best are all null";
    return nullptr;
}

// the lanes that serve one sequence: the power of two >= max(1, n_fp)
inline int rollout_group(size_t n_fp) {
    int g = 1;
    while ((size_t)g < n_fp) g *= 2;
    return g;
}

// The buffers of a context's rollouts.  Nothing is allocated before the first call.
struct RolloutStore {
    PinBuf<float> h_in;                      // the footprint (2 * ROLL_MAX_FP floats), then the controls
    DevBuf<float> d_in;
    DevBuf<lv_rollout_result> d_res;
    DevBuf<unsigned long long> d_score;
    DevBuf<float> d_poses;                   // not allocated before the first call that asks for poses
    DevBuf<unsigned long long> d_part;       // per workgroup its least (score, index), then the call's
    PinBuf<unsigned long long> h_best;

    int run(hipStream_t stream, const PlanStore& plan, const DistStore& dist, const lv_rollout_params& p, const float start[3],
            const float* controls, size_t K, const float* footprint, size_t n_fp, lv_rollout_result* results, float* poses, uint64_t* score,
            int64_t* best);
    void release();
};

}  // namespace lv
