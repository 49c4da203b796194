// lv_update.hpp — the update driver: what the host does between "an iterated update is wanted" and "its posterior is in the caller's
// hands" (lv_iterate, lv_update, the split API, lv_correct, lv_calculate_H).  lv_ctx holds one UpdateDriver; an entry point of
// lv_api.hip judges its arguments and the context, settles the map and hands over the stream, the map and the scan as an
// UpdateInputs.  The filter and the rank exchange stay in lv_ctx (other entry points use them) and come in by reference.  Split
// design: the header does not include lv_host.hpp (it does not build on the host); the launch declarations live HERE and
// lv_host.hpp includes this header.  tests/emu/update_emu.cpp compiles it with g++ and fake launches (tests/test_update_host.py).
// Rules:
// - Begin: a host prior (x_in / P_in, or the filter's pinned copy) rides in the FIRST launch's arguments when scan and map are not
//   empty; launch_kf_begin runs for a device prior (filt, filt_in_kf as ResidentFilter::prior() says), an empty scan or map, and
//   lv_calculate_H.  ResidentFilter::begin_update comes first.  A failed flush or begin of lv_correct drops the filter.
// - One launch per pass (pass_kernel) applies unless: fused_pass off | capture | phase clocks | degeneracy_mode == 2 |
//   NUM_MATCH_POINTS != 5 | lanes_per_query != 8 | extrinsics with fused_ext off | empty map | empty scan on one rank | rounds
//   above the limit (fused_multi_round 1: none, 0: three, -1: PK_DEFAULT_MAX_ROUNDS) | several ranks not fused_ready() or not
//   fitting.  A gather-only transport has no other form: refused by lv_correct before anything is enqueued or update_seq
//   advances, by lv_update after its begin.
// - Its npass + 1 launches: mode 0 (prior in the arguments) or 2 (in kf), then 1; the closing launch (one workgroup, the last
//   solve) has rounds = 0.  Launch i writes partials / costs buffer i & 1 and reads (i + 1) & 1; cost_in is null on launch 0 and
//   with keeper_by_cost off; ranks exchange after every launch but the last.
// - Three kernels: grid <= solve_direct_records(): the solve folds the block partials (nrec = grid); above: the group records.
//   RCCL, lv_iterate and the split API finalise the rank's record (directly or through the groups); RCCL all-reduces it; nrec = 1.
// - End: a log wanted: one copy of kf's log prefix and a synchronise.  Else the mailbox is polled (no HIP call when the word has
//   arrived and its checksum matches) and the stream synchronised when it is late, unchecked, mismatching (mailbox_resyncs) or
//   polling is off (spin_wait off, profiling, phase clocks, capture).  Only a profiled lv_update records events.
// - KF_FAULT_BIT (a bounded wait inside pass_kernel expired) fails the update that raised it (LV_EHIP) and only that one: the host
//   clears it on the device (the stream is idle by then) and in fallback_base; every use of the word as a counter masks it out.
// - A poisoned peer exchange (a rank gave up on another): what those launches computed is built on stale partials.  lv_update hands
//   back the prior x, P bit for bit, the filter is dropped, every update refuses until lv_comm_destroy.
// - in_update: true from a successful begin to the end and while lv_correct enqueues; any failure clears it.  begin_pending never
//   outlives its call.  grow_records synchronises before it frees (lv_reserve_stream, which used not to, included).
#pragma once
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lv_common.hpp"
#include "lv_device.hpp"
#include "lv_exchange.hpp"
#include "lv_filter.hpp"

namespace lv {

// ---- the launches (lv_match.hip)
// search_kernel writes one 128-byte record per scan point (8 float4 planes of qstride entries; qrec_slots(K) planes with K neighbours);
// fit_reduce_kernel turns them into `grid` block partials (and one extra workgroup runs solve_prep)
// begin != nullptr: the first launch of an update (no begin kernel ran): the state / covariance / pass constants
// travel as kernel arguments and one extra workgroup installs them in kf and the mailbox io
int launch_search(hipStream_t stream, int lanes_per_query, const MapView& map, const float4* scan_sorted, uint32_t n, KfDev* kf,
                  float4* qrec, uint32_t qstride, const uint32_t* tile_order, uint32_t n_tiles, double max_dist_sq, const DebugOut& dbg,
                  const BeginArg* begin, KfHostIO* io, int num_match = KNN);
int launch_fit_reduce(hipStream_t stream, const float4* qrec, uint32_t qstride, uint32_t n, KfDev* kf, const MatchParams& prm,
                      double* partials, int grid, const DebugOut& dbg, int num_match = KNN);   // num_match: NUM_MATCH_POINTS (3..8; 5 = the tuned build)
int fit_grid_size(uint32_t n, int max_blocks);
// lv_solve.hip
int launch_kf_begin(hipStream_t stream, KfDev* kf, KfHostIO* io, const double* x_host, const FilterDev* filt = nullptr, int filt_in_kf = 0);  // io: device pointer of the pinned mailbox;
// x_host != nullptr: x (NX doubles) followed by P_prop (NS*NS doubles) on the host, passed as kernel arguments
int launch_reduce_groups(hipStream_t stream, const double* partials, int nblocks, double* groups, int* ngroups_out, KfDev* kf);
int solve_direct_records();  // most records solve_kernel folds in one round trip
int launch_reduce_final(hipStream_t stream, const double* groups, int ngroups, double* sums, KfDev* kf);
struct SolveParams {
    double R;
    double R_inv;
    double limits[NS];
    int maximum_iter;
    int estimate_extrinsics;
    int seq;   // written to the host mailbox by the pass that finishes the update
    int degeneracy_mode;           // lv_params
    double degeneracy_threshold;
};
int launch_solve(hipStream_t stream, KfDev* kf, KfHostIO* io, const double* recs, int nrec, double* sums_out, const SolveParams& prm);
// lv_match.hip — one launch per pass (pass_kernel): prologue solve of the previous pass in every workgroup + search +
// plane fits + one compact partial per workgroup (lv_pass_dev.hpp)
struct PassLaunch {
    const MapView* map;
    const float4* scan;
    const uint32_t* tile_order;   // 32-point tiles (ScanStore::order_tiles(32)) or nullptr
    uint32_t n;
    KfDev* kf;
    KfHostIO* io;
    const double* recs_in;        // compact partials of the previous launch (mode 1), nrec of them
    double* part_out;
    double* sums_out;
    float4* qrec;                 // optional (debug): the hand-over records also go to memory, 8 planes of qstride entries
    long long* clk;               // optional (instrumentation): 16 stamps per search workgroup
    uint32_t qstride;
    int nrec;
    int mode;                     // 0: the update starts here (state in the BeginArg); 1: solve the previous pass first; 2: state already in kf
    int rounds, launch, nwg;      // nwg searching workgroups; rounds = 0: closing launch (one workgroup, no search);
                                  // launch = index of the launch in the update
    const uint32_t* cost_in;      // per searching workgroup: time of its search + fits in the previous launch (nullptr: none) ...
    uint32_t* cost_out;           // ... and where this launch leaves its own
    bool multi_overlap = true;    // rounds > 1: a round's plane fits beside the next round's search (pass_kernel<.., MULTI>); false: round 3's barrier form
    int steps, dedicated;         // search steps per round (1 or 2); dedicated != 0: one more workgroup only keeps the books
                                  // (otherwise the last searching workgroup does, after its own fits)
    MatchParams mp;
    SolveParams sp;
};
void pass_grid_size(uint32_t n, int max_wg, int* nsearch, int* steps, int* rounds, int* dedicated);
constexpr int PK_DEFAULT_MAX_ROUNDS = 16;   // rounds per workgroup up to which lv_update takes pass_kernel by default (1 M points on 256 CUs)
int pass_clock_words();   // stamp words per workgroup (PassLaunch::clk)
int launch_pass(hipStream_t stream, const PassLaunch& pl, const BeginArg* begin);
// lv_rows.hip
int launch_rows_from_matches(hipStream_t stream, const KfDev* kf, const float* p_world, const float* abcd, const float* dist,
                             uint32_t n, int estimate_extrinsics, double* H, double* h);

// What an update works on: the context's stream, the map as the search sees it, and the current scan in Morton order with its
// search tiles (ScanStore: d_sorted, n, d_tile_order, n_tiles, tile_points)
struct UpdateInputs {
    hipStream_t stream;
    const MapView* map;
    const float4* scan;
    uint32_t n;
    const uint32_t* tile_order;
    uint32_t n_tiles, tile_points;
};

inline void unpack_sums(const double* rec, lv_sums* out) {
    int idx = 0;
    for (int i = 0; i < 12; ++i)
        for (int j = i; j < 12; ++j) out->HTH[i * 12 + j] = out->HTH[j * 12 + i] = rec[idx++];
    for (int i = 0; i < 12; ++i) out->HTh[i] = rec[78 + i];
    out->n_valid = (int64_t)rec[90];
    out->sum_h2 = rec[91];
}

// eigenvalues (cyclic Jacobi, 8 sweeps, unsorted: the order degeneracy_stage of lv_solve_dev.hpp leaves them in) of the 6 x 6
// pose block of the H^T H packed in a 96-double sums record
inline void host_pose_eigenvalues(const double* rec, double eig[6]) {
    double A[6][6];
    int idx = 0;
    for (int i = 0; i < 12; ++i)
        for (int j = i; j < 12; ++j, ++idx)
            if (j < 6) A[i][j] = A[j][i] = rec[idx];
    for (int sweep = 0; sweep < 8; ++sweep)
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p][q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
            }
    for (int i = 0; i < 6; ++i) eig[i] = A[i][i];
}

struct UpdateDriver {
    const lv_params& prm;
    ResidentFilter& filter;   // x, P resident between lv_filter_set / lv_predict / lv_correct / lv_filter_get
    RankExchange& ranks;      // multi-GPU: how the partials of every pass reach every rank
    UpdateDriver(const lv_params& p, ResidentFilter& f, RankExchange& r) : prm(p), filter(f), ranks(r) {}
    KfDev *d_kf = nullptr, *h_kf = nullptr;       // h_kf: pinned mirror (logs / trace downloads)
    KfHostIO *h_io = nullptr, *d_io = nullptr;    // the pinned, host-mapped mailbox (update inputs and results: no copy kernels), its device address
    int update_seq = 0;        // number of the update in flight (the finishing pass echoes it into h_io->seq)
    long mailbox_resyncs = 0;  // updates whose mailbox checksum did not match at first sight (stream synchronised instead)
    int fallback_base = 0;     // device counter value before the update in flight (the device never resets it)
    // ---- the three-kernel pass: block partials, group records (reduce stage 1), the record in use (own or caller-provided)
    double *d_partials = nullptr, *d_groups = nullptr, *d_sums = nullptr, *d_sums_own = nullptr;
    double* h_sums = nullptr;      // pinned
    int ngroups = 0;
    int blocks_per_cu = 4, max_blocks = 0, grid = 1;   // LV_BLOCKS_PER_CU (tuning knob); the most fit blocks; those of this scan
    bool fold_direct = false;      // this pass: solve_kernel reads the block partials directly
    // ---- one launch per pass (pass_kernel, lv_pass_dev.hpp): compact workgroup partials and per-workgroup costs (how long its
    // search + fits took: picks the next bookkeeper), ping-pong by launch parity
    double* d_cpart[2] = {nullptr, nullptr};
    uint32_t* d_wgcost[2] = {nullptr, nullptr};
    int pass_max_wg = 0;           // search workgroups of pass_kernel: all resident at once, one per CU (LV_PASS_WG: another limit)
    // ---- search -> fit hand-over: qrec_slots(K) float4 planes of qstride entries (one record per scan point)
    float4* d_qrec = nullptr;
    uint32_t qstride = 0;
    bool qrec_valid = false;       // d_qrec holds the records of a pass over the CURRENT scan (lv_fetch_neighbors)
    // ---- capture (debug / API-parity) buffers, sized for the current scan
    size_t cap_n = 0;
    DebugOut dbg{};
    bool dbg_valid = false;
    bool begin_pending = false;    // the update's state waits in h_begin for the first search launch (no begin kernel)
    BeginArg h_begin{};
    // ---- the route flags (what each means, its option name and its environment variable: the table of lv_knobs.hpp)
    bool fused_pass = true, fused_ext = true, fast_fit = false, multi_overlap = true, keeper_by_cost = true, tile_lpt = true, spin_wait = true;
    int fused_multi_round = -1;    // 1 = pass_kernel whatever the rounds per workgroup, 0 = up to three, -1 = up to PK_DEFAULT_MAX_ROUNDS
    bool record_dump = false;      // lv_set_record_dump: pass_kernel also writes its hand-over records to d_qrec (lv_fetch_neighbors)
    bool capture = false;          // lv_set_capture: per-point outputs of every pass (the three-kernel pass alone writes them)
    bool in_update = false, last_update_fused = false;
    // ---- profiling
    bool profiling = false, phase_clocks = false;   // lv_set_profiling 1 / 2 (2: per-workgroup phase stamps of the match kernel)
    bool pass_clk = false;         // LV_PASS_CLK=1: phase stamps of pass_kernel's workgroups (lv_get_pass_clocks), allocated by alloc
    long long *d_clk = nullptr, *d_pclk = nullptr;
    int pclk_wg = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    std::vector<hipEvent_t> ev_pass;  // 3 per pass: before the search / pass kernel, after it, after the rest of the pass
    std::vector<hipEvent_t> ev_coll;  // 2 per pass: around the pass' collective (multi-GPU forms, profiled updates)
    bool coll_timed = false;          // the last profiled update recorded events around its collectives
    lv_timing timing{};
    // ---- buffers
    template <class T> static int zeroed(T** p, size_t bytes) { LV_HIP(hipMalloc(p, bytes)); LV_HIP(hipMemset(*p, 0, bytes)); return LV_OK; }
    int alloc(int n_cus) {
        // (the stamp buffer is strided by pass_max_wg + 1 workgroup slots: the grid limit is fixed first; MAX_PASSES + 1 launches)
        if (pass_max_wg <= 0) pass_max_wg = n_cus;
        if (pass_clk)
            if (int rc = zeroed(&d_pclk, (size_t)(MAX_PASSES + 1) * (pass_max_wg + 1) * pass_clock_words() * sizeof(long long))) return rc;
        max_blocks = std::max(64, n_cus * (blocks_per_cu > 0 ? blocks_per_cu : 4));
        if (int rc = zeroed(&d_kf, sizeof(KfDev))) return rc;
        LV_HIP(hipHostMalloc((void**)&h_kf, sizeof(KfDev), hipHostMallocDefault));
        std::memset(h_kf, 0, sizeof(KfDev));
        LV_HIP(hipHostMalloc((void**)&h_io, sizeof(KfHostIO), hipHostMallocMapped));
        std::memset(h_io, 0, sizeof(KfHostIO));
        LV_HIP(hipHostGetDevicePointer((void**)&d_io, h_io, 0));
        LV_HIP(hipMalloc(&d_partials, (size_t)(max_blocks + 8) * SUMS_LEN * sizeof(double)));
        LV_HIP(hipMalloc(&d_groups, (size_t)(max_blocks / 32 + 2) * SUMS_LEN * sizeof(double)));
        for (int i = 0; i < 2; ++i) {
            if (int rc = zeroed(&d_cpart[i], (size_t)(pass_max_wg + 8) * SUMS_LEN * sizeof(double))) return rc;
            if (int rc = zeroed(&d_wgcost[i], (size_t)(pass_max_wg + 8) * sizeof(uint32_t))) return rc;
        }
        if (int rc = zeroed(&d_sums_own, SUMS_LEN * sizeof(double))) return rc;
        d_sums = d_sums_own;
        LV_HIP(hipHostMalloc((void**)&h_sums, SUMS_LEN * sizeof(double), hipHostMallocDefault));
        LV_HIP(hipEventCreate(&ev_begin));
        LV_HIP(hipEventCreate(&ev_end));
        ev_pass.assign((size_t)(prm.MAX_NUM_ITERS + 1) * 3, nullptr);
        for (auto& ev : ev_pass) LV_HIP(hipEventCreate(&ev));
        ev_coll.assign((size_t)(prm.MAX_NUM_ITERS + 1) * 2, nullptr);
        for (auto& ev : ev_coll) LV_HIP(hipEventCreate(&ev));
        return LV_OK;
    }
    void release() {   // (also of a driver whose alloc failed part of the way)
        free_capture();
        for (void* h : {(void*)h_kf, (void*)h_io, (void*)h_sums}) if (h) hipHostFree(h);
        hipFree(d_cpart[0]); hipFree(d_cpart[1]); hipFree(d_pclk); hipFree(d_wgcost[0]); hipFree(d_wgcost[1]);
        hipFree(d_qrec); hipFree(d_clk); hipFree(d_kf); hipFree(d_partials); hipFree(d_groups); hipFree(d_sums_own);
        for (auto* v : {&ev_pass, &ev_coll}) for (auto ev : *v) if (ev) hipEventDestroy(ev);
        for (auto ev : {ev_begin, ev_end}) if (ev) hipEventDestroy(ev);
    }
    // room for n hand-over records: 4096, doubled until it fits; qstride is 0 between a failed allocation and the next try
    int grow_records(hipStream_t s, size_t n) {
        if ((uint32_t)n <= qstride) return LV_OK;
        uint32_t cap = qstride ? qstride : 4096;
        while (cap < (uint32_t)n) cap *= 2;
        LV_HIP(hipStreamSynchronize(s));   // (a pass over the old buffer may still be in flight)
        hipFree(d_qrec);
        d_qrec = nullptr, qstride = 0;
        LV_HIP(hipMalloc(&d_qrec, (size_t)cap * qrec_slots(prm.NUM_MATCH_POINTS) * sizeof(float4)));
        qstride = cap;
        return LV_OK;
    }
    void free_capture() {
        hipFree(dbg.knn_idx); hipFree(dbg.knn_d2); hipFree(dbg.valid); hipFree(dbg.p_world);
        hipFree(dbg.abcd); hipFree(dbg.dist); hipFree(dbg.rows); hipFree(dbg.h);
        dbg = DebugOut{}, cap_n = 0, dbg_valid = false, qrec_valid = false;
    }
    int ensure_capture(size_t n) {
        if (n <= cap_n && dbg.knn_idx) return LV_OK;
        free_capture();
        const size_t cap = n ? n : 1, K = (size_t)prm.NUM_MATCH_POINTS;
        LV_HIP(hipMalloc(&dbg.knn_idx, cap * K * sizeof(uint32_t)));
        LV_HIP(hipMalloc(&dbg.knn_d2, cap * K * sizeof(float)));
        LV_HIP(hipMalloc(&dbg.valid, cap));
        LV_HIP(hipMalloc(&dbg.p_world, cap * 3 * sizeof(float)));
        LV_HIP(hipMalloc(&dbg.abcd, cap * 4 * sizeof(float)));
        LV_HIP(hipMalloc(&dbg.dist, cap * sizeof(float)));
        LV_HIP(hipMalloc(&dbg.rows, cap * 12 * sizeof(double)));
        LV_HIP(hipMalloc(&dbg.h, cap * sizeof(double)));
        cap_n = cap;
        return LV_OK;
    }
    void new_scan() { dbg_valid = false, qrec_valid = false; }   // what was captured or handed over belongs to the scan before
    // ---- the launch parameters out of lv_params
    MatchParams match_params() const {
        // R_inv, max_dist_plane_sq, planes_threshold, estimate_extrinsics, fast_fit (pass_kernel alone knows it: update_fused)
        return {1.0 / prm.LiDAR_noise, prm.MAX_DIST_PLANE * prm.MAX_DIST_PLANE, prm.PLANES_THRESHOLD, prm.estimate_extrinsics, 0};
    }
    SolveParams solve_params() const {
        SolveParams sp;
        sp.R = prm.LiDAR_noise, sp.R_inv = 1.0 / prm.LiDAR_noise;
        for (int i = 0; i < NS; ++i) sp.limits[i] = prm.LIMITS[i];
        sp.maximum_iter = prm.MAX_NUM_ITERS, sp.estimate_extrinsics = prm.estimate_extrinsics, sp.seq = update_seq;
        sp.degeneracy_mode = prm.degeneracy_mode, sp.degeneracy_threshold = prm.degeneracy_threshold;
        return sp;
    }
    // ---- the begin.  x_host: x / P_prop ride in the first launch's arguments (or kf_begin_kernel's); else kf_begin_kernel
    // installs prior.dev in kf
    int begin_device(const UpdateInputs& in, const double* x_host, bool defer, const ResidentFilter::Prior& prior = {}) {
        if (int rf = filter.begin_update(in.stream, d_kf, prior.dev != nullptr)) return rf;
        begin_pending = false;
        if (capture) LV_HIP(hipMemsetAsync(d_kf->level_hist, 0, sizeof(int) * 8, in.stream));   // instrumentation of capturing passes
        if (defer && x_host && in.n > 0 && in.map->m > 0) {
            // the first search launch installs everything (x_host: x followed by P_prop, KfHostIO layout)
            std::memcpy(h_begin.x, x_host, sizeof(h_begin.x));
            std::memcpy(h_begin.P, x_host + NX, sizeof(h_begin.P));
            compute_pose_consts(h_begin.x, &h_begin.pose);
            begin_pending = true;
        } else if (int rc = launch_kf_begin(in.stream, d_kf, d_io, x_host, prior.dev, prior.dev_in_kf)) return rc;
        grid = fit_grid_size(in.n, max_blocks);
        if (int rc = grow_records(in.stream, in.n)) { begin_pending = false; return rc; }
        return LV_OK;
    }
    int begin(const UpdateInputs& in, const lv_state* x, const double* P, bool defer = true) {   // an update by value
        std::memcpy(h_io->x_in, x, sizeof(double) * NX);
        if (P) std::memcpy(h_io->P_in, P, sizeof(double) * NS * NS);
        else for (int i = 0; i < NS * NS; ++i) h_io->P_in[i] = (i / NS == i % NS) ? 1.0 : 0.0;
        update_seq = (update_seq + 1) & 0x3fffffff;
        return begin_device(in, h_io->x_in, defer);   // x_in and P_in (contiguous) ride in the kernel arguments
    }
    // ---- the three-kernel pass.  finalize: the rank's record is wanted in d_sums; ev_mid: a profiled pass records it behind the search
    int pass_reduce(const UpdateInputs& in, bool finalize, hipEvent_t ev_mid = nullptr) {
        const MatchParams mp = match_params();
        DebugOut out{};
        if (capture) {
            if (int rc = ensure_capture(in.n)) return rc;
            out = dbg;
            dbg_valid = false;   // (until the launches that fill the buffers are enqueued)
        }
        if (phase_clocks) {
            if (!d_clk) LV_HIP(hipMalloc(&d_clk, (size_t)(max_blocks + 8) * 16 * sizeof(long long)));
            out.clk = d_clk, out.clk_blocks = grid;
        }
        int rc = LV_OK;
        qrec_valid = in.n > 0;
        if (in.n > 0) {
            rc = launch_search(in.stream, prm.lanes_per_query, *in.map, in.scan, in.n, d_kf, d_qrec, qstride, tile_lpt ? in.tile_order : nullptr,
                               in.n_tiles, mp.max_dist_plane_sq, out, begin_pending ? &h_begin : nullptr, d_io, prm.NUM_MATCH_POINTS);
            begin_pending = false;
        }
        if (rc) return rc;
        if (ev_mid) LV_HIP(hipEventRecord(ev_mid, in.stream));
        rc = launch_fit_reduce(in.stream, d_qrec, qstride, in.n, d_kf, mp, d_partials, grid, out, prm.NUM_MATCH_POINTS);
        if (rc) return rc;
        if (capture) dbg_valid = true;
        // few enough block partials (a 64k-point scan leaves 256): solve_kernel folds them itself in one memory
        // round trip; otherwise stage 1 of the reduction runs as its own kernel
        fold_direct = !finalize && grid <= solve_direct_records();
        if (fold_direct) return LV_OK;
        if (finalize && grid <= solve_direct_records())   // the rank's record straight from its block partials
            return launch_reduce_final(in.stream, d_partials, grid, d_sums, d_kf);
        if ((rc = launch_reduce_groups(in.stream, d_partials, grid, d_groups, &ngroups, d_kf))) return rc;
        if (finalize) return launch_reduce_final(in.stream, d_groups, ngroups, d_sums, d_kf);
        return LV_OK;
    }
    int pass_solve(hipStream_t s, bool from_groups) {
        const SolveParams sp = solve_params();
        if (from_groups && fold_direct) return launch_solve(s, d_kf, d_io, d_partials, grid, d_sums, sp);
        if (from_groups) return launch_solve(s, d_kf, d_io, d_groups, ngroups, d_sums, sp);
        return launch_solve(s, d_kf, d_io, d_sums, 1, nullptr, sp);
    }
    // one measurement pass + solve as lv_update / lv_correct run it.  With a communicator (multi-GPU): the rank's record is
    // all-reduced in place on the stream and every rank solves from the identical record.  timed >= 0: the index of a profiled pass
    int pass_full(const UpdateInputs& in, int timed = -1) {
        // (a rank without points still runs the pass: its partials are zeros and solve_prep must run)
        const bool reduced = ranks.transport == RankExchange::Transport::Rccl;
        if (int rc = pass_reduce(in, reduced, timed >= 0 ? ev_pass[3 * timed + 1] : nullptr)) return rc;
        if (reduced) {
            if (timed >= 0) LV_HIP(hipEventRecord(ev_coll[2 * timed], in.stream));
            if (int rc = ranks.allreduce(in.stream, d_sums)) return rc;
            if (timed >= 0) { LV_HIP(hipEventRecord(ev_coll[2 * timed + 1], in.stream)); coll_timed = true; }
        }
        return pass_solve(in.stream, !reduced);
    }
    // ---- one launch per pass
    // doubles per compact workgroup partial (PassDims<W>::OW, lv_pass_dev.hpp): 32 for the 6-column rows, 96 with extrinsics
    size_t partial_width() const { return prm.estimate_extrinsics ? 96u : 32u; }
    // the scan size that fixes pass_kernel's geometry: the local scan, or with a communicator the largest shard over the ranks
    // (every rank launches the same grid; workgroups without a tile contribute zero partials)
    uint32_t geometry_points(const UpdateInputs& in) const { return ranks.multi_rank() ? (uint32_t)ranks.shard_max : in.n; }
    bool fused_applies(const UpdateInputs& in) const {   // (the table at the top)
        // (multi-round scans run pass_kernel<.., MULTI>; measured r04 per update: 131 072 points 191.8 us, 196 608 249.1, 262 144
        // 304.9 against 329.3 with three kernels; estimate_extrinsics takes the overlapped form as well since round 5)
        if (ranks.multi_rank() ? !ranks.fused_ready(in.n) : in.n == 0) return false;   // (a rank without points still runs every launch)
        int nwg = 0, rounds = 0, steps = 0, dedicated = 0;
        pass_grid_size(geometry_points(in), pass_max_wg, &nwg, &steps, &rounds, &dedicated);
        const int max_rounds = fused_multi_round > 0 ? INT_MAX : fused_multi_round == 0 ? 3 : PK_DEFAULT_MAX_ROUNDS;
        if (rounds > max_rounds) return false;
        if (ranks.multi_rank() && !ranks.fits((size_t)nwg * partial_width())) return false;
        // (degeneracy_mode 1 only REPORTS eigenvalues: derived on the host from the logged sums, degeneracy_values)
        return fused_pass && !capture && !phase_clocks && prm.degeneracy_mode <= 1 && prm.NUM_MATCH_POINTS == KNN &&
               prm.lanes_per_query == 8 && (prm.estimate_extrinsics == 0 || fused_ext) && in.map->m > 0;
    }
    // the whole iterated update as npass + 1 launches, after begin_device()
    int update_fused(const UpdateInputs& in, bool timed) {
        const int npass = prm.MAX_NUM_ITERS + 1;
        PassLaunch pl{};
        pl.map = in.map, pl.scan = in.scan, pl.n = in.n, pl.kf = d_kf, pl.io = d_io, pl.sums_out = d_sums;
        pl.tile_order = (tile_lpt && in.tile_points == 32u && in.n_tiles == (in.n + 31u) / 32u) ? in.tile_order : nullptr;
        pl.mp = match_params(), pl.mp.fast_fit = fast_fit && !prm.estimate_extrinsics;
        pl.sp = solve_params(), pl.sp.degeneracy_mode = 0;   // (mode 1 is derived on the host, mode 2 does not take this form)
        int nwg = 0, rounds = 0, steps = 0, dedicated = 0;
        pass_grid_size(geometry_points(in), pass_max_wg, &nwg, &steps, &rounds, &dedicated);
        const bool gathered = ranks.multi_rank();              // multi-GPU: the partials of all ranks, gathered after every launch
        const size_t slot = (size_t)nwg * partial_width();     // doubles per rank in the gather buffers (compact records)
        pl.multi_overlap = multi_overlap, pl.qrec = record_dump ? d_qrec : nullptr, pl.qstride = qstride;
        pl.nwg = nwg, pl.steps = steps, pl.dedicated = dedicated, pl.nrec = ranks.nrec(nwg);
        pclk_wg = nwg + dedicated;   // (the last slot is the bookkeeping workgroup either way)
        qrec_valid = record_dump, last_update_fused = true;
        for (int i = 0; i <= npass; ++i) {
            const bool closing = i == npass, stamp = timed && !closing;
            pl.mode = i == 0 ? (begin_pending ? 0 : 2) : 1;
            pl.recs_in = gathered ? ranks.d_gather[(i + 1) & 1] : d_cpart[(i + 1) & 1];
            pl.part_out = gathered ? ranks.part_out(i & 1, slot) : d_cpart[i & 1];
            pl.cost_in = (i > 0 && keeper_by_cost) ? d_wgcost[(i + 1) & 1] : nullptr;
            pl.cost_out = d_wgcost[i & 1];
            pl.rounds = closing ? 0 : rounds, pl.launch = i;
            pl.clk = d_pclk ? d_pclk + (size_t)i * (pass_max_wg + 1) * pass_clock_words() : nullptr;
            if (stamp) LV_HIP(hipEventRecord(ev_pass[3 * i + 0], in.stream));
            const int rc = launch_pass(in.stream, pl, (i == 0 && begin_pending) ? &h_begin : nullptr);
            begin_pending = false;
            if (rc) return rc;
            if (stamp) LV_HIP(hipEventRecord(ev_pass[3 * i + 1], in.stream));   // (the pass kernel alone)
            if (gathered && !closing) {
                if (timed) LV_HIP(hipEventRecord(ev_coll[2 * i], in.stream));
                if (int re = ranks.exchange(in.stream, i, slot)) return re;
                if (timed) LV_HIP(hipEventRecord(ev_coll[2 * i + 1], in.stream));
            }
            if (stamp) LV_HIP(hipEventRecord(ev_pass[3 * i + 2], in.stream));
        }
        coll_timed = gathered && timed;
        return LV_OK;
    }
    // ---- the passes of lv_update (timed: a profiled update brackets them with events) and lv_correct, after the begin
    enum class Route { Fused, ThreeKernel, Refused };   // Refused: a gather-only transport and a scan that does not take the one-launch form
    Route route(const UpdateInputs& in) const { return fused_applies(in) ? Route::Fused : ranks.gather_only() ? Route::Refused : Route::ThreeKernel; }
    int run_passes(const UpdateInputs& in, Route r, bool timed) {
        last_update_fused = false;
        coll_timed = false;
        const int rc = [&]() -> int {
            if (timed) LV_HIP(hipEventRecord(ev_begin, in.stream));
            if (r == Route::Refused) return ranks.refuse_unfused();
            if (r == Route::Fused) {
                if (int rf = update_fused(in, timed)) return rf;
            } else {
                for (int i = 0; i <= prm.MAX_NUM_ITERS; ++i) {
                    if (timed) LV_HIP(hipEventRecord(ev_pass[3 * i + 0], in.stream));
                    if (int rp = pass_full(in, timed ? i : -1)) return rp;
                    if (timed) LV_HIP(hipEventRecord(ev_pass[3 * i + 2], in.stream));
                }
            }
            if (timed) LV_HIP(hipEventRecord(ev_end, in.stream));
            return LV_OK;
        }();
        begin_pending = false;
        if (rc) in_update = false;   // (the one place a failure between the begin and the end clears it)
        return rc;
    }
    // ---- failures that outlive a call (the rules at the top)
    int report_fault(hipStream_t s, int raw) {
        const int cnt = fallback_count(raw);
        LV_HIP(hipStreamSynchronize(s));
        LV_HIP(hipMemcpy(&d_kf->fallback_queries, &cnt, sizeof(int), hipMemcpyHostToDevice));
        h_io->fallback_queries = cnt, fallback_base = cnt;
        set_error("a bounded wait inside pass_kernel expired: this update's results are invalid (the flag has been cleared; the context stays usable)");
        return LV_EHIP;
    }
    static int fallback_count(int raw) { return raw & (int)~KF_FAULT_BIT; }
    void count_fallbacks(int raw) { timing.fallback_queries = fallback_count(raw) - fallback_base, fallback_base = fallback_count(raw); }
    int poisoned() {
        if (!ranks.failed()) return LV_OK;
        filter.drop(), in_update = false;
        set_error("peer-mapped gather: a rank of the node did not publish its partials in time (or reported a failed exchange): the update "
                  "was not adopted; lv_comm_destroy, then lv_filter_set / a new exchange");
        return LV_ESTATE;
    }
    // mailbox_wait's `enabled` (lv_filter.hpp): not where something else waits on the stream anyway
    bool spin_ok() const { return spin_wait && !profiling && !phase_clocks && !capture; }
    int busy(const char* call) const { return in_update ? (set_error("%s inside an update", call), LV_ESTATE) : LV_OK; }
    // ---- the entry points
    int iterate(const UpdateInputs& in, const lv_state* x, lv_sums* out) {
        std::memset(out, 0, sizeof(*out));
        if (in.map->m == 0 || in.n == 0) { dbg_valid = false; return LV_OK; }  // Mapper.cpp:42 — empty Matches
        const bool cap = capture;
        capture = true;  // lv_iterate is the API-parity path: always captures per-point outputs
        int rc = begin(in, x, nullptr);
        if (!rc) rc = pass_reduce(in, true);
        capture = cap;
        begin_pending = false;
        if (rc) return rc;
        LV_HIP(hipMemcpyAsync(h_sums, d_sums, SUMS_LEN * sizeof(double), hipMemcpyDeviceToHost, in.stream));
        LV_HIP(hipMemcpyAsync(&h_kf->fallback_queries, &d_kf->fallback_queries, sizeof(int), hipMemcpyDeviceToHost, in.stream));
        LV_HIP(hipStreamSynchronize(in.stream));
        unpack_sums(h_sums, out);
        count_fallbacks(h_kf->fallback_queries);
        return LV_OK;
    }
    int update_begin(const UpdateInputs& in, const lv_state* x, const double* P) {
        const int rc = begin(in, x, P);
        in_update = rc == LV_OK;
        return rc;
    }
    int split_reduce(const UpdateInputs& in) {
        return in_update ? pass_reduce(in, true) : (set_error("lv_pass_reduce outside lv_update_begin/end"), LV_ESTATE);
    }
    int split_solve(hipStream_t s) {
        return in_update ? pass_solve(s, false) : (set_error("lv_pass_solve outside lv_update_begin/end"), LV_ESTATE);
    }
    int update_end(hipStream_t s, lv_state* x, double* P, int* passes, bool want_log = false) {   // want_log: download the trace / per-pass sums
        if (!in_update) { set_error("lv_update_end without lv_update_begin"); return LV_ESTATE; }
        in_update = false;
        begin_pending = false;
        // results were stored into the pinned mailbox by kf_begin_kernel / solve_kernel; the device copy of the logs
        // is only downloaded when the caller asked for them
        if (want_log) {
            LV_HIP(hipMemcpyAsync(h_kf, d_kf, offsetof(KfDev, pose), hipMemcpyDeviceToHost, s));
            LV_HIP(hipStreamSynchronize(s));
        } else if (!mailbox_wait(h_io, update_seq, spin_ok(), &mailbox_resyncs)) {
            LV_HIP(hipStreamSynchronize(s));
        }
        const KfHostIO* io = h_io;
        if ((unsigned)io->fallback_queries & KF_FAULT_BIT) return report_fault(s, io->fallback_queries);
        count_fallbacks(io->fallback_queries);
        if (x) std::memcpy(x, io->x, sizeof(double) * NX);
        if (P) std::memcpy(P, io->P_post, sizeof(double) * NS * NS);
        if (passes) *passes = io->passes;
        h_kf->passes = io->passes;
        timing.last_passes = h_kf->passes;
        if (prm.degeneracy_mode && prm.print_degeneracy_values) {   // print_degeneracy_values (config/params.yaml:53)
            double eig[MAX_PASSES * 6];
            int np = 0;
            if (degeneracy_values(s, eig, MAX_PASSES, &np) == LV_OK)
                for (int i = 0; i < np; ++i)
                    fprintf(stderr, "degeneracy eigenvalues (pass %d): %.6g %.6g %.6g %.6g %.6g %.6g\n", i, eig[6 * i], eig[6 * i + 1],
                            eig[6 * i + 2], eig[6 * i + 3], eig[6 * i + 4], eig[6 * i + 5]);
        }
        return LV_OK;
    }
    int update(const UpdateInputs& in, lv_state* x, double* P, int* passes, lv_sums* per_pass, double* trace) {
        if (passes) *passes = 0;
        filter.latest = ResidentFilter::Source::ByValue;
        if (in.map->m == 0) {  // Localizator::correct returns without a map (Localizator.cpp:24)
            // ... but the state the caller propagated is the one the first map is built with (main.cpp:92,102 -> lv_map_add_scan)
            if (int rp = filter.flush(in.stream, d_kf)) return rp;   // (a resident filter that still lives in kf moves out before kf->x is overwritten)
            if (int rm = filter.materialise(in.stream, d_kf)) return rm;
            LV_HIP(hipStreamSynchronize(in.stream));   // (x_in of an earlier update may still be in flight)
            std::memcpy(h_io->x_in, x, sizeof(double) * NX);
            LV_HIP(hipMemcpyAsync(d_kf->x, h_io->x_in, sizeof(double) * NX, hipMemcpyHostToDevice, in.stream));
            return LV_OK;
        }
        const int npass = prm.MAX_NUM_ITERS + 1;
        if (int rq = poisoned()) return rq;
        const bool peer = ranks.transport == RankExchange::Transport::PeerMapped;   // (a failed exchange must hand the caller's buffers
        const lv_state x_prior = *x;                                                // back untouched: update_end writes into them)
        const std::vector<double> P_prior(P, peer ? P + NS * NS : P);
        if (int rc = update_begin(in, x, P)) return rc;
        const bool timed = profiling;
        if (int rc = run_passes(in, route(in), timed)) return rc;
        int np = 0;
        if (int re = update_end(in.stream, x, P, &np, per_pass || trace)) return re;
        if (peer) {
            // update_end has waited for the update's last launch, so every pull of this update has run: a pull that gave up on a
            // peer (or met a poisoned flag) has set the sticky status word.  The caller gets its prior back, nothing is adopted.
            LV_HIP(hipStreamSynchronize(in.stream));
            if (ranks.failed()) {
                *x = x_prior;
                std::memcpy(P, P_prior.data(), sizeof(double) * NS * NS);
                return poisoned();
            }
        }
        if (passes) *passes = np;
        if (per_pass)
            for (int i = 0; i < np && i < MAX_PASSES; ++i) unpack_sums(h_kf->sums_log + (size_t)i * SUMS_LEN, &per_pass[i]);
        if (trace) std::memcpy(trace, h_kf->trace, sizeof(double) * 49 * (size_t)(np < MAX_PASSES ? np : MAX_PASSES));
        if (timed) read_events(np, npass);
        return LV_OK;
    }
    void read_events(int np, int npass) {   // a profiled lv_update, after its end
        const auto ms = [](hipEvent_t a, hipEvent_t b) { float t = 0.f; hipEventElapsedTime(&t, a, b); return t; };
        timing.last_update_ms = ms(ev_begin, ev_end);
        float r = 0.f, s = 0.f;
        for (int i = 0; i < np && i < npass; ++i) {
            const float a = ms(ev_pass[3 * i + 0], ev_pass[3 * i + 1]), b = ms(ev_pass[3 * i + 1], ev_pass[3 * i + 2]);
            r += a, s += b;
            if (i >= 8) continue;
            timing.pass_match_ms[i] = a, timing.pass_solve_ms[i] = b;
            timing.pass_collective_ms[i] = coll_timed ? ms(ev_coll[2 * i], ev_coll[2 * i + 1]) : 0.f;
        }
        timing.last_reduce_ms = r / (np > 0 ? np : 1);
        timing.last_solve_ms = s / (np > 0 ? np : 1);
    }
    int correct(const UpdateInputs& in, int* passes) {
        if (int rs = filter.need("lv_correct")) return rs;
        if (int rp = filter.flush(in.stream, d_kf)) { filter.drop(); return rp; }   // (its queued predictions are gone)
        filter.latest = ResidentFilter::Source::Filter;
        if (passes) *passes = 0;
        if (in.map->m == 0) return LV_OK;  // Localizator::correct returns without a map (Localizator.cpp:24)
        if (int rq = poisoned()) return rq;   // (a failed exchange of an EARLIER, asynchronous lv_correct surfaces here at the latest)
        const Route r = route(in);
        if (r == Route::Refused) return ranks.refuse_unfused();   // (before anything is enqueued: the filter stays exactly where it was)
        update_seq = (update_seq + 1) & 0x3fffffff;   // (the finishing pass echoes it into the mailbox: lv_filter_get polls for it)
        const ResidentFilter::Prior prior = filter.prior();
        if (int rc = begin_device(in, prior.host, prior.host != nullptr, prior)) { filter.drop(); return rc; }   // (prior() has moved it on)
        in_update = true;
        const int rc = run_passes(in, r, false);
        in_update = false;
        if (rc) { filter.drop(); return rc; }   // (an enqueue failed part of the way: passes that did run may have moved kf->x)
        filter.correct_done();
        if (passes) {  // optional: the only synchronisation point
            LV_HIP(hipStreamSynchronize(in.stream));
            if (int rq = poisoned()) return rq;
            *passes = h_io->passes;   // stored by solve_kernel into the pinned mailbox
        }
        return LV_OK;
    }
    int filter_get(hipStream_t s, lv_state* x, double* P) {
        const int rc = filter.get(s, d_kf, h_io, update_seq, spin_ok(), &mailbox_resyncs, x, P);
        return rc > 0 ? report_fault(s, rc) : rc;
    }
    int set_sums_buffer(hipStream_t s, void* device_ptr) {
        if (int rb = busy("lv_set_sums_buffer")) return rb;
        LV_HIP(hipStreamSynchronize(s));
        d_sums = device_ptr ? static_cast<double*>(device_ptr) : d_sums_own;
        return LV_OK;
    }
    int calculate_H(const UpdateInputs& in, const lv_state* x, const float* p_world, const float* abcd, const float* dist, size_t n, double* H,
                    double* h) {
        if (int rb = busy("lv_calculate_H")) return rb;
        int rc = begin(in, x, nullptr, false);  // derives the pass constants from x on the device (begin kernel)
        if (rc) return rc;
        float* d_in = nullptr;
        double* d_out = nullptr;
        hipStream_t s = in.stream;
        if (hipMalloc(&d_in, n * 8 * sizeof(float)) != hipSuccess || hipMalloc(&d_out, n * 13 * sizeof(double)) != hipSuccess) {
            hipFree(d_in);
            set_error("lv_calculate_H: HIP error");
            return LV_EHIP;
        }
        float *d_pw = d_in, *d_abcd = d_in + 3 * n, *d_dist = d_in + 7 * n;
        if (hipMemcpyAsync(d_pw, p_world, n * 3 * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(d_abcd, abcd, n * 4 * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(d_dist, dist, n * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess)
            rc = LV_EHIP;
        if (!rc) rc = launch_rows_from_matches(s, d_kf, d_pw, d_abcd, d_dist, (uint32_t)n, prm.estimate_extrinsics, d_out, d_out + n * 12);
        if (!rc && hipMemcpyAsync(H, d_out, n * 12 * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) rc = LV_EHIP;
        if (!rc && hipMemcpyAsync(h, d_out + n * 12, n * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) rc = LV_EHIP;
        if (hipStreamSynchronize(s) != hipSuccess) rc = LV_EHIP;
        hipFree(d_in), hipFree(d_out);
        if (rc == LV_EHIP) set_error("lv_calculate_H: HIP error");
        return rc;
    }
    // lv_get_degeneracy_values: per pass of the last update, the eigenvalues of the pose block of H^T H
    int degeneracy_values(hipStream_t s, double* eig, int capacity_passes, int* n_passes) {
        LV_HIP(hipStreamSynchronize(s));
        int np = 0;
        LV_HIP(hipMemcpy(&np, &d_kf->passes, sizeof(int), hipMemcpyDeviceToHost));
        np = np > MAX_PASSES ? MAX_PASSES : np, np = np > capacity_passes ? capacity_passes : np;
        if (np > 0 && last_update_fused) {
            // degeneracy_mode 1 is a REPORT (print_degeneracy_values, config/params.yaml:53): the one-launch-per-pass form does not
            // compute it on the device at all (a cyclic Jacobi is a serial f64 chain of ~75 us in one lane) — the eigenvalues are derived
            // here, on demand, from the sums record each pass logged, by the same fixed 8 sweeps as degeneracy_stage (lv_solve_dev.hpp)
            std::vector<double> log((size_t)np * SUMS_LEN);
            LV_HIP(hipMemcpy(log.data(), d_kf->sums_log, log.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int p = 0; p < np; ++p) host_pose_eigenvalues(&log[(size_t)p * SUMS_LEN], eig + 6 * p);
        } else if (np > 0) {
            LV_HIP(hipMemcpy(eig, d_kf->degen_eig, (size_t)np * 6 * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (n_passes) *n_passes = np;
        return LV_OK;
    }
};

}  // namespace lv
