// tests/emu/update_emu.cpp — HOST test of the update driver (limo-velo_amd/csrc/lv_update.hpp) and the knob table (lv_knobs.hpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_update_host.py into tests/emu/_build/ (once plain, once with AddressSanitizer +
// UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own UpdateDriver, ResidentFilter and RankExchange against
// the stand-in hip_runtime.h next to this file.  The launches are fakes that log their name and the arguments that matter into
// the stand-in's call log (so one log orders HIP calls and launches, and the stand-in's `fail` hook fails either); the launch
// that finishes an update writes a toy posterior of what the begin installed into kf and the mailbox, with a correct seqcheck.
// fit_grid_size, solve_direct_records and pass_grid_size answer what the scenario set.  Usage: update_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <memory>
#include <random>

#include "../../limo-velo_amd/csrc/lv_update.hpp"
#include "../../limo-velo_amd/csrc/lv_knobs.hpp"

using namespace lv;
using Where = ResidentFilter::Where;
using Transport = RankExchange::Transport;
using Calls = std::vector<std::string>;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            std::_Exit(1);                                                              \
        }                                                                               \
    } while (0)

namespace {

void toy_step(double* x, double* P, const double* Q, const double* st) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.75 + st[0] * (j + 1) + st[1 + j % 6] * 0.125;
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.5 + Q[k % 144] * st[0];
}
void toy_update(double* x, double* P) {
    for (int j = 0; j < NX; ++j) x[j] = x[j] * 0.5 + 1.0 / (j + 1);
    for (int k = 0; k < NS * NS; ++k) P[k] = P[k] * 0.25 + 0.01;
}

// ---- what the fakes answer and remember
UpdateDriver* g_drv = nullptr;
int g_fit_grid = 8, g_direct = 264;
struct { int nwg, steps, rounds, dedicated; } g_geom = {8, 1, 1, 0};
int g_solves = 0;               // solves since the last begin (the three-kernel forms finish on solve MAX_NUM_ITERS + 1)
enum class Finish { Normal, Late, Unchecked, Mismatch, Fault } g_finish = Finish::Normal;
unsigned long long g_late_word = 0;
bool g_peer_failed = false, g_has_allgather = true;
std::function<void(const char*)> g_hook;   // runs at every logged call
int g_fail_at = -1, g_calls_seen = 0;      // fail the call with this index (counted from arm())
std::string g_fail_prefix;                 // ... or, with g_fail_at == -2, every call whose name starts with this

int fake(hipStream_t s, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (emu_hip::call(buf, s) != hipSuccess) { set_error("%s failed", buf); return LV_EHIP; }
    return LV_OK;
}
char cpart(const double* p) { return !p ? '-' : p == g_drv->d_cpart[0] ? '0' : p == g_drv->d_cpart[1] ? '1' : p == g_drv->ranks.d_gather[0] ? 'a' :
                              p == g_drv->ranks.d_gather[1] ? 'b' : (g_drv->ranks.d_gather[0] && p > g_drv->ranks.d_gather[0] && p < g_drv->ranks.d_gather[0] + g_drv->ranks.gather_cap) ? 'A' : 'B'; }
char cost(const uint32_t* p) { return !p ? '-' : p == g_drv->d_wgcost[0] ? '0' : p == g_drv->d_wgcost[1] ? '1' : '?'; }
char recs(const double* p) { return p == g_drv->d_partials ? 'P' : p == g_drv->d_groups ? 'G' : p == g_drv->d_sums ? 'S' : '?'; }

void install(KfDev* kf, const double* x, const double* P) {
    std::memcpy(kf->x, x, sizeof(kf->x));
    std::memcpy(kf->P_post, P, sizeof(kf->P_post));
    g_solves = 0;
}
void finish(KfDev* kf, KfHostIO* io, int seq, int passes) {
    toy_update(kf->x, kf->P_post);
    kf->passes = passes;
    std::memcpy(io->x, kf->x, sizeof(io->x));
    std::memcpy(io->P_post, kf->P_post, sizeof(io->P_post));
    io->passes = passes;
    uint32_t chk = 0;
    for (int i = 0; i < NS * NS; ++i) chk ^= mailbox_mix(io->P_post[i], (uint32_t)i);
    for (int i = 0; i < NX; ++i) chk ^= mailbox_mix(io->x[i], 1000u + (uint32_t)i);
    chk ^= mailbox_mix((double)io->passes, 2000u);
    if (chk == MAILBOX_UNCHECKED) chk = 0u;
    if (g_finish == Finish::Unchecked) chk = MAILBOX_UNCHECKED;
    if (g_finish == Finish::Mismatch) chk ^= 0x5a5au;   // (some result had not arrived when the word was read)
    if (g_finish == Finish::Fault) io->fallback_queries = (int)KF_FAULT_BIT | 7, kf->fallback_queries = io->fallback_queries;
    const unsigned long long word = ((unsigned long long)chk << 32) | (uint32_t)seq;
    if (g_finish == Finish::Late) g_late_word = word;   // (arrives with the stream's synchronise)
    else io->seqcheck = word;
}

}  // namespace

// ---- the fakes: lv_match.hip, lv_solve.hip, lv_rows.hip
int lv::launch_search(hipStream_t s, int, const MapView&, const float4*, uint32_t n, KfDev* kf, float4*, uint32_t, const uint32_t* tile_order, uint32_t,
                      double, const DebugOut& dbg, const BeginArg* begin, KfHostIO*, int) {
    if (int rc = fake(s, "launch_search n=%u begin=%d tiles=%d dbg=%d", n, begin != nullptr, tile_order != nullptr, dbg.knn_idx != nullptr)) return rc;
    if (begin) install(kf, begin->x, begin->P);
    return LV_OK;
}
int lv::launch_fit_reduce(hipStream_t s, const float4*, uint32_t, uint32_t, KfDev*, const MatchParams&, double*, int grid, const DebugOut&, int) {
    return fake(s, "launch_fit_reduce grid=%d", grid);
}
int lv::fit_grid_size(uint32_t, int) { return g_fit_grid; }
int lv::solve_direct_records() { return g_direct; }
int lv::launch_kf_begin(hipStream_t s, KfDev* kf, KfHostIO*, const double* x_host, const FilterDev* filt, int in_kf) {
    if (int rc = fake(s, "launch_kf_begin host=%d filt=%d in_kf=%d", x_host != nullptr, filt != nullptr, in_kf)) return rc;
    if (x_host) install(kf, x_host, x_host + NX);
    else if (filt && !in_kf) install(kf, filt->x, filt->P);
    g_solves = 0;
    return LV_OK;
}
int lv::launch_reduce_groups(hipStream_t s, const double* partials, int nblocks, double*, int* ngroups, KfDev*) {
    *ngroups = (nblocks + PARTIAL_GROUP - 1) / PARTIAL_GROUP;
    return fake(s, "launch_reduce_groups from=%c n=%d", recs(partials), nblocks);
}
int lv::launch_reduce_final(hipStream_t s, const double* groups, int n, double*, KfDev*) { return fake(s, "launch_reduce_final from=%c n=%d", recs(groups), n); }
int lv::launch_solve(hipStream_t s, KfDev* kf, KfHostIO* io, const double* r, int nrec, double*, const SolveParams& sp) {
    if (int rc = fake(s, "launch_solve from=%c nrec=%d seq=%d", recs(r), nrec, sp.seq)) return rc;
    if (++g_solves == sp.maximum_iter + 1) finish(kf, io, sp.seq, g_solves);
    return LV_OK;
}
void lv::pass_grid_size(uint32_t, int, int* nsearch, int* steps, int* rounds, int* dedicated) {
    *nsearch = g_geom.nwg, *steps = g_geom.steps, *rounds = g_geom.rounds, *dedicated = g_geom.dedicated;
}
int lv::pass_clock_words() { return 32; }
int lv::launch_pass(hipStream_t s, const PassLaunch& pl, const BeginArg* begin) {
    if (int rc = fake(s, "launch_pass mode=%d rounds=%d nwg=%d launch=%d in=%c out=%c cost_in=%c cost_out=%c begin=%d seq=%d fast=%d qrec=%d tiles=%d nrec=%d",
                      pl.mode, pl.rounds, pl.nwg, pl.launch, cpart(pl.recs_in), cpart(pl.part_out), cost(pl.cost_in), cost(pl.cost_out), begin != nullptr,
                      pl.sp.seq, pl.mp.fast_fit, pl.qrec != nullptr, pl.tile_order != nullptr, pl.nrec))
        return rc;
    CHECK(pl.sp.degeneracy_mode == 0);
    if (begin) install(pl.kf, begin->x, begin->P);
    if (pl.rounds == 0) finish(pl.kf, pl.io, pl.sp.seq, pl.sp.maximum_iter + 1);
    return LV_OK;
}
int lv::launch_rows_from_matches(hipStream_t s, const KfDev*, const float*, const float*, const float*, uint32_t n, int, double*, double*) {
    return fake(s, "launch_rows n=%u", n);
}
// ---- lv_predict.hip, lv_observe.hip
int lv::launch_predict(hipStream_t s, FilterDev* f, const KfDev* src, const double* Q, int n, const double (*steps)[7]) {
    if (int rc = fake(s, "launch_predict from_kf=%d n=%d", src != nullptr, n)) return rc;
    FilterDev t;
    std::memcpy(t.x, src ? src->x : f->x, sizeof(t.x));
    std::memcpy(t.P, src ? src->P_post : f->P, sizeof(t.P));
    for (int i = 0; i < n; ++i) toy_step(t.x, t.P, Q, steps[i]);
    *f = t;
    return LV_OK;
}
int lv::launch_kf_to_filter(hipStream_t s, const KfDev* kf, FilterDev* f) {
    if (int rc = fake(s, "launch_kf_to_filter")) return rc;
    std::memcpy(f->x, kf->x, sizeof(f->x));
    std::memcpy(f->P, kf->P_post, sizeof(f->P));
    return LV_OK;
}
int lv::launch_observe(hipStream_t s, FilterDev*, const lv_observation*, int, lv_observe_result*) { return fake(s, "launch_observe"); }
// ---- lv_comm.hip, lv_peer.hip
int lv::comm_unique_id(const char*, void*) { return LV_OK; }
int lv::comm_init(const char*, const void*, int, int, void** comm) { *comm = (void*)0x10; return LV_OK; }
int lv::comm_destroy(void*) { return LV_OK; }
int lv::comm_allreduce_record(void*, double* rec, hipStream_t s) { return fake(s, "allreduce rec=%c", recs(rec)); }
bool lv::comm_has_allgather() { return g_has_allgather; }
int lv::comm_allgather_inplace(void*, double* buf, size_t, int, hipStream_t s) { return fake(s, "allgather buf=%c", cpart(buf)); }
int lv::peer_export(PeerSet&, size_t, void*) { return LV_OK; }
int lv::peer_init(PeerSet&, int, int, const void*) { return LV_OK; }
int lv::peer_gather(PeerSet&, int parity, size_t, hipStream_t s) { return fake(s, "peer_gather parity=%d", parity); }
bool lv::peer_failed(const PeerSet&) { return g_peer_failed; }
void lv::peer_close(PeerSet&) {}

namespace {

size_t mark() { return emu_hip::state().log.size(); }
Calls calls(size_t from) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i) v.push_back(log[i].call);
    return v;
}
Calls launches(size_t from) {   // the launches and collectives alone (what an update enqueues, whatever the buffers needed first)
    Calls v;
    for (auto& c : calls(from))
        if (c.rfind("launch_", 0) == 0 || c.rfind("all", 0) == 0 || c.rfind("peer_", 0) == 0) v.push_back(c);
    return v;
}
int count(const Calls& v, const char* prefix) {
    int n = 0;
    for (auto& c : v) n += c.rfind(prefix, 0) == 0;
    return n;
}
void show(const Calls& v) { for (auto& c : v) fprintf(stderr, "  %s\n", c.c_str()); }
#define CHECK_CALLS(got, ...)                                     \
    do {                                                          \
        const Calls _g = (got), _w = Calls{__VA_ARGS__};          \
        if (_g != _w) { fprintf(stderr, "got:\n"); show(_g); fprintf(stderr, "want:\n"); show(_w); CHECK(!"call log"); } \
    } while (0)
void arm(int at) { g_fail_at = at, g_calls_seen = 0; }

lv_params params(int iters) {
    lv_params p{};
    p.MAX_NUM_ITERS = iters, p.NUM_MATCH_POINTS = 5, p.MAX_DIST_PLANE = 2.0, p.PLANES_THRESHOLD = 5.e-2f, p.LiDAR_noise = 0.001;
    for (double& l : p.LIMITS) l = 0.001;
    p.degeneracy_threshold = 5.0, p.voxel_size = 0.5f, p.lanes_per_query = 8;
    return p;
}

struct Logical { bool set = false; double x[NX], P[NS * NS]; };
Logical seed(double v) {
    Logical m;
    m.set = true;
    for (int j = 0; j < NX; ++j) m.x[j] = v + j;
    for (int k = 0; k < NS * NS; ++k) m.P[k] = (k % (NS + 1) == 0) ? v : 0.001 * k;
    return m;
}
double g_Q[144];
const double g_acc[3] = {0.1, -0.2, 9.81}, g_gyro[3] = {0.01, 0.02, -0.03};

// a context as lv_api.hip holds it: parameters, filter, exchange, driver, and a map and a scan to view
struct Rig {
    lv_params prm;
    ResidentFilter filter;
    RankExchange ranks;
    UpdateDriver d{prm, filter, ranks};
    MapView map{};
    float4 scan[4];
    uint32_t tiles[4];
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    uint32_t n = 2000, n_tiles = 0, tile_points = 32;   // n_tiles 0: as many 32-point tiles as the scan has
    explicit Rig(int iters = 3, bool warm = true) : prm(params(iters)) {
        g_drv = &d;
        CHECK(d.alloc(8) == LV_OK && filter.alloc() == LV_OK);
        if (warm) CHECK(d.grow_records(s, 4096) == LV_OK);   // as a first update leaves it; `buffers` and the failures watch it grow
        map.m = 50000;
    }
    ~Rig() { d.release(); filter.release(); ranks.release(); g_drv = nullptr; }
    UpdateInputs in() const { return {s, &map, scan, n, tiles, n_tiles ? n_tiles : (n + 31u) / 32u, tile_points}; }
    int update(Logical& v, int* passes = nullptr, lv_sums* per_pass = nullptr) { return d.update(in(), reinterpret_cast<lv_state*>(v.x), v.P, passes, per_pass, nullptr); }
    int set(const Logical& v) { return filter.set(reinterpret_cast<const lv_state*>(v.x), v.P); }
    int predict(double dt) { return filter.predict(s, d.d_kf, dt, g_Q, g_acc, g_gyro); }
    int get(Logical& v) { return d.filter_get(s, reinterpret_cast<lv_state*>(v.x), v.P); }
    void two_ranks(Transport t) {   // as lv_comm_* + lv_comm_set_shard_max leave the exchange
        ranks.rank = 1, ranks.world = 2, ranks.shard_max = n, ranks.comm = (void*)0x10;
        CHECK(ranks.reserve(s, (size_t)g_geom.nwg * 32) == LV_OK);
        ranks.transport = t;
    }
};
bool same(const Logical& a, const Logical& b) { return !std::memcmp(a.x, b.x, sizeof(a.x)) && !std::memcmp(a.P, b.P, sizeof(a.P)); }
Logical updated(Logical v) { toy_update(v.x, v.P); return v; }
Logical predicted(Logical v, double dt) {
    const double st[7] = {dt, g_acc[0], g_acc[1], g_acc[2], g_gyro[0], g_gyro[1], g_gyro[2]};
    toy_step(v.x, v.P, g_Q, st);
    return v;
}
std::string pass(int mode, int rounds, int launch, char in, char out, char ci, char co, int begin, int seq, int fast = 0, int qrec = 0, int tiles = 1,
                 int nwg = 8, int nrec = 8) {
    char b[256];
    snprintf(b, sizeof(b), "launch_pass mode=%d rounds=%d nwg=%d launch=%d in=%c out=%c cost_in=%c cost_out=%c begin=%d seq=%d fast=%d qrec=%d tiles=%d nrec=%d",
             mode, rounds, nwg, launch, in, out, ci, co, begin, seq, fast, qrec, tiles, nrec);
    return b;
}
Calls fused_log(int iters, int seq, bool pending, bool by_cost = true, int fast = 0, int qrec = 0, int tiles = 1) {
    Calls v;
    for (int i = 0; i <= iters + 1; ++i) {
        const char a = '0' + ((i + 1) & 1), b = '0' + (i & 1);
        v.push_back(pass(i == 0 ? (pending ? 0 : 2) : 1, i == iters + 1 ? 0 : 1, i, a, b, (i > 0 && by_cost) ? a : '-', b, i == 0 && pending, seq, fast, qrec, tiles));
    }
    return v;
}
std::string fmt(const char* f, ...) {
    char b[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof(b), f, ap);
    va_end(ap);
    return b;
}
Calls three_log(int iters, int seq, int n, int grid, bool direct, bool rccl = false, bool dbg = false) {
    Calls v;
    for (int i = 0; i <= iters; ++i) {
        v.push_back(fmt("launch_search n=%d begin=%d tiles=1 dbg=%d", n, i == 0, (int)dbg));
        v.push_back(fmt("launch_fit_reduce grid=%d", grid));
        const int ng = (grid + PARTIAL_GROUP - 1) / PARTIAL_GROUP;
        if (!direct) v.push_back(fmt("launch_reduce_groups from=P n=%d", grid));
        if (rccl) {
            v.push_back(direct ? fmt("launch_reduce_final from=P n=%d", grid) : fmt("launch_reduce_final from=G n=%d", ng));
            v.push_back("allreduce rec=S");
            v.push_back(fmt("launch_solve from=S nrec=1 seq=%d", seq));
        } else {
            v.push_back(direct ? fmt("launch_solve from=P nrec=%d seq=%d", grid, seq) : fmt("launch_solve from=G nrec=%d seq=%d", ng, seq));
        }
    }
    return v;
}

// ---- scenarios
void fused_by_value() {
    for (int iters : {0, 3}) {
        Rig r(iters);
        Logical v = seed(1.0);
        const Logical want = updated(v);
        int passes = -1;
        size_t t = mark();
        CHECK(r.update(v, &passes) == LV_OK);
        CHECK(launches(t) == fused_log(iters, 1, true));
        CHECK(count(calls(t), "launch_kf_begin") == 0 && count(calls(t), "hipEventRecord") == 0);
        CHECK(same(v, want) && passes == iters + 1 && r.d.update_seq == 1 && r.d.last_update_fused && !r.d.in_update && !r.d.begin_pending);
        CHECK(!r.d.qrec_valid && r.d.pclk_wg == 8);
        // the second update needs no buffer: its launches and nothing else (the mailbox has the word: no synchronise)
        t = mark();
        CHECK(r.update(v, &passes) == LV_OK);
        CHECK(calls(t) == fused_log(iters, 2, true));
        // the knobs that show in the launch arguments
        r.d.keeper_by_cost = false, r.d.fast_fit = true, r.d.record_dump = true;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(calls(t) == fused_log(iters, 3, true, false, 1, 1));
        CHECK(r.d.qrec_valid);
        r.d.keeper_by_cost = true, r.d.fast_fit = false, r.d.record_dump = false;
        // the tile order is for 32-point tiles of this scan, and for tile_lpt
        for (int k = 0; k < 3; ++k) {
            if (k == 0) r.tile_points = 64;
            if (k == 1) r.n_tiles = 62;
            if (k == 2) r.d.tile_lpt = false;
            t = mark();
            CHECK(r.update(v) == LV_OK);
            CHECK(calls(t) == fused_log(iters, 4 + k, true, true, 0, 0, 0));
            r.tile_points = 32, r.n_tiles = 0, r.d.tile_lpt = true;
        }
        // fast_fit is not for the 12-column rows
        r.prm.estimate_extrinsics = 1, r.d.fast_fit = true;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(calls(t) == fused_log(iters, 7, true));
        // profiling: an event before and two after every pass launch, ev_begin / ev_end around, the elapsed times read at the end
        r.prm.estimate_extrinsics = 0, r.d.fast_fit = false, r.d.profiling = true;
        emu_hip::state().elapsed_ms = 0.25f;
        t = mark();
        CHECK(r.update(v, &passes) == LV_OK);
        const Calls c = calls(t);
        CHECK(launches(t) == fused_log(iters, 8, true));
        CHECK(count(c, "hipEventRecord") == 2 + 3 * (iters + 1) && count(c, "hipStreamSynchronize") == 1);
        CHECK(c[0] == "hipEventRecord" && emu_hip::state().log[t].event == r.d.ev_begin);
        CHECK(count(c, "hipEventElapsedTime") == 1 + 2 * (iters + 1));
        CHECK(r.d.timing.last_update_ms == 0.25f && r.d.timing.pass_match_ms[0] == 0.25f && r.d.timing.last_passes == iters + 1);
    }
}
void three_kernel_by_value() {
    for (int iters : {0, 3}) {
        Rig r(iters);
        r.d.fused_pass = false;
        Logical v = seed(2.0);
        const Logical want = updated(v);
        int passes = -1;
        g_fit_grid = 8;
        size_t t = mark();
        CHECK(r.update(v, &passes) == LV_OK);
        CHECK(launches(t) == three_log(iters, 1, 2000, 8, true));
        CHECK(same(v, want) && passes == iters + 1 && !r.d.last_update_fused && r.d.qrec_valid && r.d.fold_direct && !r.d.dbg_valid);
        g_fit_grid = 264;   // the most the solve folds itself
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(calls(t) == three_log(iters, 2, 2000, 264, true));
        g_fit_grid = 265;   // one more: the group records
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(calls(t) == three_log(iters, 3, 2000, 265, false));
        CHECK(!r.d.fold_direct && r.d.ngroups == 9);
        // RCCL: the rank's record, all-reduced in place, one record solved; collective events only when profiling
        r.two_ranks(Transport::Rccl);
        r.ranks.fused = false;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(calls(t) == three_log(iters, 4, 2000, 265, false, true));
        g_fit_grid = 8;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(calls(t) == three_log(iters, 5, 2000, 8, true, true));
        r.d.profiling = true;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(launches(t) == three_log(iters, 6, 2000, 8, true, true));
        CHECK(count(calls(t), "hipEventRecord") == 2 + 5 * (iters + 1) && r.d.coll_timed);
        {   // the collective's events bracket it
            const auto& log = emu_hip::state().log;
            int k = 0;
            for (size_t i = t; i < log.size(); ++i)
                if (log[i].call == "allreduce rec=S") {
                    CHECK(log[i - 1].call == "hipEventRecord" && log[i - 1].event == r.d.ev_coll[2 * k]);
                    CHECK(log[i + 1].call == "hipEventRecord" && log[i + 1].event == r.d.ev_coll[2 * k + 1]);
                    ++k;
                }
            CHECK(k == iters + 1);
        }
        r.d.profiling = false;
        r.ranks.transport = Transport::None, r.ranks.world = 1, r.ranks.rank = 0, r.ranks.comm = nullptr;
        // capture: the capture buffers (sized by NUM_MATCH_POINTS) go to both kernels, the histogram is cleared at the begin, the end synchronises
        r.d.capture = true;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        CHECK(launches(t) == three_log(iters, 7, 2000, 8, true, false, true));
        CHECK(r.d.dbg_valid && r.d.cap_n == 2000 && count(calls(t), "hipMemsetAsync") == 1 && count(calls(t), "hipMalloc") == 8);
        CHECK(count(calls(t), "hipStreamSynchronize") == 1);
        // an empty scan: no search, the begin kernel instead of a ride, the rest of the pass all the same
        r.d.capture = false, r.n = 0;
        t = mark();
        CHECK(r.update(v) == LV_OK);
        Calls want_log = {"launch_kf_begin host=1 filt=0 in_kf=0"};
        for (int i = 0; i <= iters; ++i) want_log.push_back("launch_fit_reduce grid=8"), want_log.push_back("launch_solve from=P nrec=8 seq=8");
        CHECK(calls(t) == want_log);
        CHECK(!r.d.qrec_valid);
    }
}
void route_table() {
    Rig r;
    Logical v = seed(3.0);
    auto fused = [&] { return r.d.fused_applies(r.in()); };
    auto route = [&] { return r.d.route(r.in()); };
    using Route = UpdateDriver::Route;
    CHECK(fused() && route() == Route::Fused);
#define FLIPS(set, unset) do { set; CHECK(!fused() && route() == Route::ThreeKernel); CHECK(r.update(v) == LV_OK && !r.d.last_update_fused); \
                               unset; CHECK(fused()); CHECK(r.update(v) == LV_OK && r.d.last_update_fused); } while (0)
    FLIPS(r.d.fused_pass = false, r.d.fused_pass = true);
    FLIPS(r.d.capture = true, r.d.capture = false);
    FLIPS(r.d.phase_clocks = true, r.d.phase_clocks = false);
    FLIPS(r.prm.degeneracy_mode = 2, r.prm.degeneracy_mode = 1);
    FLIPS(r.prm.NUM_MATCH_POINTS = 4, r.prm.NUM_MATCH_POINTS = 5);
    FLIPS(r.prm.lanes_per_query = 4, r.prm.lanes_per_query = 8);
    FLIPS((r.prm.estimate_extrinsics = 1, r.d.fused_ext = false), r.d.fused_ext = true);
    r.prm.estimate_extrinsics = 0;
    FLIPS(r.n = 0, r.n = 2000);
    FLIPS((g_geom.rounds = 17), g_geom.rounds = 16);                                  // -1: up to PK_DEFAULT_MAX_ROUNDS
    FLIPS((r.d.fused_multi_round = 0, g_geom.rounds = 4), g_geom.rounds = 3);         // 0: up to three
    FLIPS((g_geom.rounds = 1000, r.d.fused_multi_round = -1), r.d.fused_multi_round = 1);   // 1: whatever
    g_geom.rounds = 1, r.d.fused_multi_round = -1;
#undef FLIPS
    r.map.m = 0;   // an empty map: no update at all (lv_update uploads x), and no one-launch form
    CHECK(!fused());
    r.map.m = 50000;
    // several ranks: ready (the largest shard told, the scan within it, an all-gather, the buffers), and fitting
    r.two_ranks(Transport::Rccl);
    CHECK(fused());
    r.ranks.shard_max = 0;      CHECK(!fused() && route() == Route::ThreeKernel);   r.ranks.shard_max = 1999; CHECK(!fused());   r.ranks.shard_max = 2000;
    r.ranks.fused = false;      CHECK(!fused());   r.ranks.fused = true;
    g_has_allgather = false;    CHECK(!fused());   g_has_allgather = true;
    g_geom.nwg = 9;             CHECK(!fused());   g_geom.nwg = 8;   // (2 ranks x 9 workgroups x 32 doubles do not fit the reserve)
    r.n = 0;                    CHECK(fused());    r.n = 2000;       // (a rank without points still runs every launch)
    CHECK(fused());
    {   // the exchange after every launch but the last, on the buffer the launch wrote; this rank's slot of it
        size_t t = mark();
        CHECK(r.update(v) == LV_OK);
        const Calls c = calls(t);
        CHECK(c.size() == 5 + 4 && c[0] == pass(0, 1, 0, 'b', 'A', '-', '0', 1, r.d.update_seq, 0, 0, 1, 8, 16) && c[1] == "allgather buf=a");
        CHECK(c[2] == pass(1, 1, 1, 'a', 'B', '0', '1', 0, r.d.update_seq, 0, 0, 1, 8, 16) && c[3] == "allgather buf=b" && c.back().rfind("launch_pass mode=1 rounds=0", 0) == 0);
    }
    // a gather-only rank has no other form: lv_update refuses after its begin, lv_correct before anything
    r.ranks.transport = Transport::HostGather;
    r.d.fused_pass = false;
    CHECK(route() == Route::Refused);
    const Logical before = v;
    int seq = r.d.update_seq;
    size_t t = mark();
    CHECK(r.update(v) == LV_ESTATE && std::strstr(g_err, "does not take the one-launch-per-pass form"));
    CHECK(calls(t).empty() && r.d.update_seq == seq + 1 && !r.d.in_update && !r.d.begin_pending && same(v, before));   // (the begin rode nowhere)
    CHECK(!std::memcmp(r.d.h_io->x_in, v.x, sizeof(v.x)));
    CHECK(r.set(v) == LV_OK);
    seq = r.d.update_seq;
    t = mark();
    CHECK(r.d.correct(r.in(), nullptr) == LV_ESTATE);
    CHECK(calls(t).empty() && r.d.update_seq == seq && r.filter.where == Where::Host && !r.d.in_update);
}
void iterate() {
    Rig r;
    Logical v = seed(4.0);
    lv_sums out;
    std::memset(&out, 0xff, sizeof(out));
    r.d.dbg_valid = true, r.n = 0;
    size_t t = mark();
    CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_OK);
    CHECK(calls(t).empty() && !r.d.dbg_valid && out.n_valid == 0 && out.HTH[5] == 0.0 && r.d.update_seq == 0);
    r.n = 2000, r.map.m = 0, r.d.dbg_valid = true;
    CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_OK && calls(t).empty() && !r.d.dbg_valid);
    r.map.m = 50000;
    // capture is forced for the call and restored; the record is finalised and copied; the fallback counter is a difference
    r.d.d_kf->fallback_queries = 5;
    t = mark();
    CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_OK);
    CHECK(launches(t) == (Calls{"launch_search n=2000 begin=1 tiles=1 dbg=1", "launch_fit_reduce grid=8", "launch_reduce_final from=P n=8"}));
    CHECK(!r.d.capture && r.d.dbg_valid && r.d.timing.fallback_queries == 5 && r.d.fallback_base == 5 && !r.d.in_update && !r.d.begin_pending);
    CHECK(r.d.h_io->P_in[0] == 1.0 && r.d.h_io->P_in[1] == 0.0 && r.d.h_io->P_in[NS + 1] == 1.0);   // (identity covariance)
    r.d.d_kf->fallback_queries = 12 | (int)KF_FAULT_BIT;   // (the fault bit is not part of the count)
    CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_OK);
    CHECK(r.d.timing.fallback_queries == 7 && r.d.fallback_base == 12);
    g_fit_grid = 300;   // the groups on the way to the record
    t = mark();
    CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_OK);
    CHECK(launches(t) == (Calls{"launch_search n=2000 begin=1 tiles=1 dbg=1", "launch_fit_reduce grid=300", "launch_reduce_groups from=P n=300",
                                "launch_reduce_final from=G n=10"}));
    g_fit_grid = 8;
    // a failing launch: capture restored all the same, nothing marked captured
    for (const char* what : {"launch_search", "launch_fit_reduce", "launch_reduce_final", "hipMemcpyAsync", "hipStreamSynchronize"}) {
        r.d.dbg_valid = false;
        g_fail_prefix = what, arm(-2);
        CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_EHIP);
        arm(-1);
        CHECK(!r.d.capture && !r.d.in_update && !r.d.begin_pending);
        if (!std::strcmp(what, "launch_search") || !std::strcmp(what, "launch_fit_reduce")) CHECK(!r.d.dbg_valid);
    }
    CHECK(r.d.iterate(r.in(), reinterpret_cast<lv_state*>(v.x), &out) == LV_OK && r.d.dbg_valid);
}
void split_api() {
    Rig r;
    Logical v = seed(5.0), o = seed(0.0);
    int passes = 0;
    CHECK(r.d.split_reduce(r.in()) == LV_ESTATE && std::strstr(g_err, "lv_pass_reduce outside"));
    CHECK(r.d.split_solve(r.s) == LV_ESTATE && std::strstr(g_err, "lv_pass_solve outside"));
    CHECK(r.d.update_end(r.s, nullptr, nullptr, nullptr) == LV_ESTATE && std::strstr(g_err, "lv_update_end without"));
    CHECK(r.d.busy("lv_set_option") == LV_OK);
    size_t t = mark();
    CHECK(r.d.update_begin(r.in(), reinterpret_cast<lv_state*>(v.x), v.P) == LV_OK && r.d.in_update && r.d.begin_pending);
    // inside: everything that would pull the ground away refuses (lv_set_option, the lv_comm_* calls, ... ask busy())
    for (const char* call : {"lv_set_option", "lv_comm_init", "lv_comm_destroy", "lv_comm_set_host_gather", "lv_comm_peer_export", "lv_comm_peer_init",
                             "lv_comm_set_shard_max"})
        CHECK(r.d.busy(call) == LV_ESTATE && std::strstr(g_err, call) && std::strstr(g_err, "inside an update"));
    CHECK(r.d.set_sums_buffer(r.s, nullptr) == LV_ESTATE && std::strstr(g_err, "lv_set_sums_buffer inside an update"));
    float f[8] = {};
    double H[12], h[1];
    CHECK(r.d.calculate_H(r.in(), reinterpret_cast<lv_state*>(v.x), f, f, f, 1, H, h) == LV_ESTATE && std::strstr(g_err, "lv_calculate_H inside an update"));
    for (int i = 0; i < 4; ++i) { CHECK(r.d.split_reduce(r.in()) == LV_OK); CHECK(r.d.split_solve(r.s) == LV_OK); }
    CHECK(r.d.update_end(r.s, reinterpret_cast<lv_state*>(o.x), o.P, &passes) == LV_OK && !r.d.in_update);
    Calls want;
    for (int i = 0; i < 4; ++i) {
        want.push_back(fmt("launch_search n=2000 begin=%d tiles=1 dbg=0", i == 0));
        want.push_back("launch_fit_reduce grid=8"), want.push_back("launch_reduce_final from=P n=8"), want.push_back("launch_solve from=S nrec=1 seq=1");
    }
    CHECK(launches(t) == want && same(o, updated(v)) && passes == 4);
    CHECK(r.d.update_end(r.s, nullptr, nullptr, nullptr) == LV_ESTATE);
    // outside again: the same calls pass, and lv_calculate_H takes the begin kernel (no ride: nothing searches)
    double own = 0;
    CHECK(r.d.set_sums_buffer(r.s, &own) == LV_OK && r.d.d_sums == &own);
    CHECK(r.d.set_sums_buffer(r.s, nullptr) == LV_OK && r.d.d_sums == r.d.d_sums_own);
    t = mark();
    const long m0 = emu_hip::state().mallocs, f0 = emu_hip::state().frees;
    CHECK(r.d.calculate_H(r.in(), reinterpret_cast<lv_state*>(v.x), f, f, f, 1, H, h) == LV_OK);
    CHECK(launches(t) == (Calls{"launch_kf_begin host=1 filt=0 in_kf=0", "launch_rows n=1"}) && !r.d.begin_pending);
    CHECK(emu_hip::state().mallocs - m0 == 2 && emu_hip::state().frees - f0 == 2);
    // The failed begin.  (At the commit before the driver moved, lv_update_begin set in_update first and left it set when the begin
    // failed: every call above then refused with "inside an update" for the life of the context.  This check fails there.)
    for (const char* what : {"launch_predict", "hipMalloc"}) {
        Rig q;
        CHECK(q.set(v) == LV_OK && q.predict(0.01) == LV_OK);   // (something for the filter to flush)
        q.n = 5000;                                              // (... and records to grow: past the first 4096)
        g_fail_prefix = what, arm(-2);
        CHECK(q.d.update_begin(q.in(), reinterpret_cast<lv_state*>(v.x), v.P) == LV_EHIP);
        arm(-1);
        CHECK(!q.d.in_update && !q.d.begin_pending && q.d.busy("lv_set_option") == LV_OK);
        if (!std::strcmp(what, "hipMalloc")) CHECK(q.d.qstride == 0 && q.d.d_qrec == nullptr);
        Logical w = v;
        CHECK(q.update(w) == LV_OK && same(w, updated(v)) && q.d.qstride == 8192);
    }
}

// fail every call of `run` in turn, on a fresh rig each time; after() judges the wreck, then the same driver runs `run` cleanly
void fail_everywhere(const std::function<void(Rig&)>& prepare, const std::function<int(Rig&)>& run, const std::function<void(Rig&, const std::string&)>& after,
                     const std::function<void(Rig&)>& again) {
    Calls clean;   // the calls of a run nothing fails, in order
    {
        Rig r;
        prepare(r);
        const size_t t = mark();
        arm(1 << 30);
        CHECK(run(r) == LV_OK);
        CHECK((size_t)g_calls_seen == mark() - t);
        clean = calls(t);
        arm(-1);
    }
    CHECK(clean.size() > 4);
    for (size_t k = 0; k < clean.size(); ++k) {
        Rig r;
        prepare(r);
        arm((int)k);
        const int rc = run(r);
        arm(-1);
        // the only calls whose result nobody looks at: the free of a buffer being regrown, the elapsed-time reads
        if (clean[k] == "hipFree" || clean[k] == "hipEventElapsedTime") { CHECK(rc == LV_OK); continue; }
        CHECK(rc == LV_EHIP);
        CHECK(!r.d.in_update && !r.d.begin_pending);
        after(r, g_err);
        again(r);
    }
}
void failures_by_value() {
    const Logical v0 = seed(6.0);
    for (int form = 0; form < 3; ++form) {   // one launch per pass, three kernels (with groups), three kernels over RCCL; all profiled
        Logical v;
        Logical filt = seed(60.0);
        auto prepare = [&](Rig& r) {
            v = v0;
            r.d.profiling = true, r.n = 5000;
            r.d.fused_pass = form == 0;
            g_fit_grid = form == 1 ? 300 : 8;
            if (form == 2) r.two_ranks(Transport::Rccl), r.ranks.fused = false;
            CHECK(r.set(filt) == LV_OK && r.predict(0.01) == LV_OK);   // (a filter with a queue: the begin flushes it)
        };
        lv_sums logged[MAX_PASSES];   // (asked for: the end is the copy of the log and a synchronise)
        auto run = [&](Rig& r) { int p = 0; return r.update(v, &p, logged); };
        auto after = [&](Rig& r, const std::string&) {
            CHECK(same(v, v0));                              // the caller's x, P untouched
            CHECK(r.filter.where != Where::Unset);           // a by-value update does not drop the filter
        };
        auto again = [&](Rig& r) {
            const size_t t = mark();
            int p = 0;
            CHECK(r.update(v, &p) == LV_OK && same(v, updated(v0)) && p == 4);
            const Calls l = launches(t);
            Calls want = form == 0 ? fused_log(3, r.d.update_seq, true) : three_log(3, r.d.update_seq, 5000, g_fit_grid, form != 1, form == 2);
            Calls got;
            for (auto& c : l) if (c.rfind("launch_predict", 0) && c.rfind("launch_kf_to", 0)) got.push_back(c);
            CHECK_CALLS(got, want);
        };
        fail_everywhere(prepare, run, after, again);
        g_fit_grid = 8;
    }
}
void failures_correct() {
    const Logical v0 = seed(7.0);
    for (int form = 0; form < 4; ++form) {   // host prior / device prior (a queued prediction), each on both forms
        auto prepare = [&](Rig& r) {
            r.n = 5000, r.d.fused_pass = form < 2;
            CHECK(r.set(v0) == LV_OK);
            if (form & 1) CHECK(r.predict(0.01) == LV_OK);
        };
        auto run = [&](Rig& r) { int p = 0; return r.d.correct(r.in(), &p); };
        auto after = [&](Rig& r, const std::string& err) {
            // dropped: the caller seeds it again.  (All but the wait for the pass count: by then everything is enqueued and adopted.)
            if (r.filter.where == Where::Kf) { CHECK(err.find("hipStreamSynchronize") != std::string::npos); return; }
            CHECK(r.filter.where == Where::Unset);
            Logical o;
            CHECK(r.get(o) == LV_ESTATE && r.d.correct(r.in(), nullptr) == LV_ESTATE);
        };
        auto again = [&](Rig& r) {
            CHECK(r.set(v0) == LV_OK);
            const size_t t = mark();
            int p = 0;
            CHECK(r.d.correct(r.in(), &p) == LV_OK && p == 4);
            CHECK_CALLS(launches(t), r.d.fused_pass ? fused_log(3, r.d.update_seq, true) : three_log(3, r.d.update_seq, 5000, 8, true));
            Logical o;
            CHECK(r.get(o) == LV_OK && same(o, updated(v0)));
        };
        fail_everywhere(prepare, run, after, again);
    }
}
void update_end() {
    Rig r;
    Logical v = seed(8.0);
    const Logical v0 = v;
    // the word has arrived: no HIP call at all behind the launches
    size_t t = mark();
    CHECK(r.update(v) == LV_OK && calls(t) == fused_log(3, 1, true) && r.d.mailbox_resyncs == 0);
    // a log is wanted: one copy of the log prefix and a synchronise
    lv_sums per_pass[MAX_PASSES];
    int passes = 0;
    t = mark();
    CHECK(r.update(v, &passes, per_pass) == LV_OK);
    Calls want = fused_log(3, 2, true);
    want.push_back("hipMemcpyAsync"), want.push_back("hipStreamSynchronize");
    CHECK(calls(t) == want);
    // late / unchecked / polling off: one synchronise, nothing counted; a mismatch: counted
    g_hook = [&](const char* call) { if (g_late_word && !std::strcmp(call, "hipStreamSynchronize")) r.d.h_io->seqcheck = g_late_word, g_late_word = 0; };
    struct { Finish f; bool spin; long resyncs; } cases[] = {{Finish::Late, true, 0}, {Finish::Unchecked, true, 0}, {Finish::Normal, false, 0}, {Finish::Mismatch, true, 1}};
    int seq = 2;
    for (auto& c : cases) {
        g_finish = c.f, r.d.spin_wait = c.spin;
        v = v0;
        t = mark();
        CHECK(r.update(v) == LV_OK && same(v, updated(v0)));
        want = fused_log(3, ++seq, true);
        want.push_back("hipStreamSynchronize");
        CHECK(calls(t) == want && r.d.mailbox_resyncs == c.resyncs);
        g_finish = Finish::Normal, r.d.spin_wait = true;
    }
    // what else waits on the stream anyway switches the poll off
    CHECK(r.d.spin_ok());
    r.d.profiling = true; CHECK(!r.d.spin_ok()); r.d.profiling = false;
    r.d.phase_clocks = true; CHECK(!r.d.spin_ok()); r.d.phase_clocks = false;
    r.d.capture = true; CHECK(!r.d.spin_ok()); r.d.capture = false;
    // the fault bit: this update fails, the word is cleared on the device and in the base, the next update runs
    g_finish = Finish::Fault;
    v = v0;
    t = mark();
    CHECK(r.update(v) == LV_EHIP && std::strstr(g_err, "bounded wait") && same(v, v0) && !r.d.in_update);
    CHECK(count(calls(t), "hipStreamSynchronize") == 1 && count(calls(t), "hipMemcpy") == 1);
    CHECK(r.d.d_kf->fallback_queries == 7 && r.d.h_io->fallback_queries == 7 && r.d.fallback_base == 7);
    g_finish = Finish::Normal;
    CHECK(r.update(v) == LV_OK && same(v, updated(v0)) && r.d.timing.fallback_queries == 0);
    // ... the same through lv_filter_get
    CHECK(r.set(v0) == LV_OK);
    g_finish = Finish::Fault;
    CHECK(r.d.correct(r.in(), nullptr) == LV_OK);
    Logical o = v0;
    CHECK(r.get(o) == LV_EHIP && same(o, v0) && r.d.fallback_base == 7 && r.d.h_io->fallback_queries == 7);
    g_finish = Finish::Normal;
    g_hook = nullptr;
}
void peer_failure() {
    Rig r;
    r.two_ranks(Transport::PeerMapped);
    Logical v = seed(9.0);
    const Logical v0 = v;
    CHECK(r.set(seed(90.0)) == LV_OK);
    size_t t = mark();
    CHECK(r.update(v) == LV_OK && same(v, updated(v0)));
    CHECK(count(calls(t), "peer_gather") == 4 && calls(t).back() == "hipStreamSynchronize");   // (a peer update always waits for its pulls)
    v = v0;
    g_hook = [&](const char* call) { if (!std::strncmp(call, "launch_pass mode=1 rounds=0", 27)) g_peer_failed = true; };
    CHECK(r.update(v) == LV_ESTATE && std::strstr(g_err, "peer-mapped gather"));
    g_hook = nullptr;
    CHECK(same(v, v0) && r.filter.where == Where::Unset && !r.d.in_update);   // the prior back bit for bit; the filter dropped
    t = mark();
    CHECK(r.update(v) == LV_ESTATE && r.set(v0) == LV_OK && r.d.correct(r.in(), nullptr) == LV_ESTATE && r.filter.where == Where::Unset);
    CHECK(calls(t) == Calls{"hipEventSynchronize"} && same(v, v0));   // (lv_filter_set's wait for its last upload: nothing is enqueued)
    g_peer_failed = false, r.ranks.transport = Transport::None;   // (lv_comm_destroy)
    CHECK(r.update(v) == LV_OK && same(v, updated(v0)));
}
void update_no_map() {
    Rig r;
    r.map.m = 0;
    Logical v = seed(10.0), f = seed(100.0);
    CHECK(r.set(f) == LV_OK && r.d.correct(r.in(), nullptr) == LV_OK && r.filter.where == Where::Host);   // (no map: lv_correct returns)
    r.map.m = 50000;
    CHECK(r.d.correct(r.in(), nullptr) == LV_OK && r.filter.where == Where::Kf);
    r.map.m = 0;
    int passes = 7;
    size_t t = mark();
    CHECK(r.update(v, &passes) == LV_OK && passes == 0);
    CHECK(calls(t) == (Calls{"launch_kf_to_filter", "hipStreamSynchronize", "hipMemcpyAsync"}));
    CHECK(r.filter.where == Where::Copied && r.filter.latest == ResidentFilter::Source::ByValue && !std::memcmp(r.d.d_kf->x, v.x, sizeof(v.x)));
    CHECK(r.d.update_seq == 1 && !r.d.in_update);
    Logical o;
    CHECK(r.get(o) == LV_OK && same(o, updated(f)));   // (the mailbox still holds the correct's posterior)
}
void correct() {
    Rig r;
    Logical v = seed(11.0), o;
    // a host prior rides in launch 0: no upload, no begin kernel, no synchronise
    CHECK(r.set(v) == LV_OK);
    size_t t = mark();
    CHECK(r.d.correct(r.in(), nullptr) == LV_OK);
    CHECK(calls(t) == fused_log(3, 1, true) && r.d.update_seq == 1 && r.filter.where == Where::Kf && !r.d.in_update);
    t = mark();
    CHECK(r.get(o) == LV_OK && same(o, updated(v)) && calls(t).empty());
    // a device prior in kf (correct after correct): the begin kernel finds it there, launch 0 has mode 2
    t = mark();
    CHECK(r.d.correct(r.in(), nullptr) == LV_OK);
    Calls want = {"launch_kf_begin host=0 filt=1 in_kf=1"};
    for (auto& c : fused_log(3, 2, false)) want.push_back(c);
    CHECK(calls(t) == want && r.d.update_seq == 2);
    v = updated(updated(v));
    // a device prior in d (a prediction in between): flushed out of kf, installed from d
    CHECK(r.predict(0.01) == LV_OK);
    int passes = 0;
    t = mark();
    CHECK(r.d.correct(r.in(), &passes) == LV_OK && passes == 4);
    want = {"launch_predict from_kf=1 n=1", "launch_kf_begin host=0 filt=1 in_kf=0"};
    for (auto& c : fused_log(3, 3, false)) want.push_back(c);
    want.push_back("hipStreamSynchronize");   // (asked for the passes: the only wait)
    CHECK(calls(t) == want);
    CHECK(r.get(o) == LV_OK && same(o, updated(predicted(v, 0.01))));
    // on three kernels the same begin
    r.d.fused_pass = false;
    CHECK(r.set(v) == LV_OK);
    t = mark();
    CHECK(r.d.correct(r.in(), nullptr) == LV_OK && calls(t) == three_log(3, 4, 2000, 8, true));
    CHECK(r.d.correct(r.in(), nullptr) == LV_OK);
    CHECK(r.get(o) == LV_OK && same(o, updated(updated(v))));
    // before a filter is set
    Rig q;
    CHECK(q.d.correct(q.in(), nullptr) == LV_ESTATE && std::strstr(g_err, "lv_correct before lv_filter_set") && q.d.update_seq == 0);
}
void buffers() {
    {
        Rig r(3, false);
        CHECK(r.d.qstride == 0);
        size_t t = mark();
        CHECK(r.d.grow_records(r.s, 100) == LV_OK && r.d.qstride == 4096);
        CHECK(calls(t) == (Calls{"hipStreamSynchronize", "hipFree", "hipMalloc"}));   // (the synchronise before the free)
        CHECK(emu_hip::state().last_alloc_bytes == (size_t)4096 * 8 * sizeof(float4));
        t = mark();
        CHECK(r.d.grow_records(r.s, 4096) == LV_OK && calls(t).empty());
        CHECK(r.d.grow_records(r.s, 4097) == LV_OK && r.d.qstride == 8192);
        CHECK(r.d.grow_records(r.s, 70000) == LV_OK && r.d.qstride == 131072);
        g_fail_prefix = "hipMalloc", arm(-2);
        CHECK(r.d.grow_records(r.s, 131073) == LV_EHIP && r.d.qstride == 0 && r.d.d_qrec == nullptr);
        arm(-1);
        CHECK(r.d.grow_records(r.s, 10) == LV_OK && r.d.qstride == 4096);
        // capture buffers: K words per point, grown for a larger scan, kept for a smaller one
        r.prm.NUM_MATCH_POINTS = 7;
        CHECK(r.d.ensure_capture(0) == LV_OK && r.d.cap_n == 1);
        t = mark();
        CHECK(r.d.ensure_capture(100) == LV_OK && r.d.cap_n == 100 && count(calls(t), "hipMalloc") == 8);
        CHECK(emu_hip::state().last_alloc_bytes == 100 * sizeof(double));
        r.d.dbg_valid = true;
        t = mark();
        CHECK(r.d.ensure_capture(50) == LV_OK && calls(t).empty() && r.d.dbg_valid);
        r.d.new_scan();
        CHECK(!r.d.dbg_valid && !r.d.qrec_valid && r.d.cap_n == 100);
        // phase clocks: allocated by the first pass that stamps
        r.d.phase_clocks = true, r.prm.NUM_MATCH_POINTS = 5;
        Logical v = seed(12.0);
        CHECK(r.update(v) == LV_OK && r.d.d_clk != nullptr);
    }
    {   // a driver whose alloc failed part of the way releases what it has
        lv_params prm = params(3);
        ResidentFilter f;
        RankExchange x;
        for (int k = 0; k < 30; ++k) {
            UpdateDriver d{prm, f, x};
            d.pass_clk = true;
            arm(k);
            const int rc = d.alloc(8);
            arm(-1);
            CHECK(rc == LV_EHIP || k >= 20);
            d.release();
            CHECK(emu_hip::state().mallocs == emu_hip::state().frees && emu_hip::state().events_created == emu_hip::state().events_destroyed);
        }
    }
}

// ---- the knob table over a stand-in context with lv_ctx's member names
struct FakeCtx {
    lv_params prm = params(3);
    ResidentFilter filter;
    RankExchange ranks;
    UpdateDriver upd{prm, filter, ranks};
    hipStream_t stream = nullptr;
    bool overlap_insert = true;
    struct { struct { bool async = false; size_t async_min = 0; uint32_t pause_us = 0, slice_wgs = 0; size_t journal_max = 8; int test_delay_ms = 0; bool test_race = false; } opt; } rebuild;
    struct { bool merged_back = true, sweep_evict = true, small_front = true, surv_list = true; } map;
    struct { bool small_enabled = true, large_enabled = true; } scan;
    struct { int chunk_hyp = 0; } batch;
};
struct KnobCase { const char* option; const char* env; bool is_bool; std::function<long(FakeCtx&)> get; };
void knobs() {
    // every option name lv_set_option knew and every variable lv_create read before the table, as literals: a dropped row fails
    const KnobCase cases[] = {
        {"fused_pass", "LV_FUSED_PASS", true, [](FakeCtx& c) { return (long)c.upd.fused_pass; }},
        {"fused_ext", "LV_FUSED_EXT", true, [](FakeCtx& c) { return (long)c.upd.fused_ext; }},
        {"fast_fit", nullptr, true, [](FakeCtx& c) { return (long)c.upd.fast_fit; }},
        {"async_relinearise", "LV_ASYNC_RELINEARISE", true, [](FakeCtx& c) { return (long)c.rebuild.opt.async; }},
        {"async_relinearise_min", nullptr, false, [](FakeCtx& c) { return (long)c.rebuild.opt.async_min; }},
        {"async_relinearise_pause_us", "LV_RELIN_PAUSE_US", false, [](FakeCtx& c) { return (long)c.rebuild.opt.pause_us; }},
        {"async_relinearise_slice_wgs", "LV_RELIN_SLICE_WGS", false, [](FakeCtx& c) { return (long)c.rebuild.opt.slice_wgs; }},
        {"async_relinearise_journal_max", nullptr, false, [](FakeCtx& c) { return (long)c.rebuild.opt.journal_max; }},
        {"async_relinearise_test_delay_ms", nullptr, false, [](FakeCtx& c) { return (long)c.rebuild.opt.test_delay_ms; }},
        {"async_relinearise_test_race", nullptr, true, [](FakeCtx& c) { return (long)c.rebuild.opt.test_race; }},
        {"multi_overlap", "LV_MULTI_OVERLAP", true, [](FakeCtx& c) { return (long)c.upd.multi_overlap; }},
        {"fused_multi_round", "LV_FUSED_MULTI", true, [](FakeCtx& c) { return (long)c.upd.fused_multi_round; }},
        {"keeper_by_cost", "LV_KEEPER_BY_COST", true, [](FakeCtx& c) { return (long)c.upd.keeper_by_cost; }},
        {"tile_lpt", "LV_TILE_LPT", true, [](FakeCtx& c) { return (long)c.upd.tile_lpt; }},
        {"spin_wait", "LV_SPIN_WAIT", true, [](FakeCtx& c) { return (long)c.upd.spin_wait; }},
        {"comm_fused", "LV_COMM_FUSED", true, [](FakeCtx& c) { return (long)c.ranks.fused; }},
        {"mail_filter", "LV_MAIL_FILTER", true, [](FakeCtx& c) { return (long)c.filter.mail_filter; }},
        {"overlap_insert", "LV_OVERLAP_INSERT", true, [](FakeCtx& c) { return (long)c.overlap_insert; }},
        {"batch_predict", "LV_BATCH_PREDICT", true, [](FakeCtx& c) { return (long)c.filter.batch_predict; }},
        {"merged_insert", "LV_MERGED_INSERT", true, [](FakeCtx& c) { return (long)c.map.merged_back; }},
        {"sweep_evict", "LV_SWEEP_EVICT", true, [](FakeCtx& c) { return (long)c.map.sweep_evict; }},
        {"small_window", "LV_SMALL_WINDOW", true, [](FakeCtx& c) { return (long)c.scan.small_enabled; }},
        {"large_window", "LV_LARGE_WINDOW", true, [](FakeCtx& c) { return (long)c.scan.large_enabled; }},
        {"small_insert", "LV_SMALL_INSERT", true, [](FakeCtx& c) { return (long)c.map.small_front; }},
        {"survivor_list", "LV_SURV_LIST", true, [](FakeCtx& c) { return (long)c.map.surv_list; }},
        {"batch_chunk_hypotheses", nullptr, false, [](FakeCtx& c) { return (long)c.batch.chunk_hyp; }},
        {nullptr, "LV_BLOCKS_PER_CU", false, [](FakeCtx& c) { return (long)c.upd.blocks_per_cu; }},
        {nullptr, "LV_PASS_WG", false, [](FakeCtx& c) { return (long)c.upd.pass_max_wg; }},
        {nullptr, "LV_PASS_CLK", true, [](FakeCtx& c) { return (long)c.upd.pass_clk; }},
    };
    const size_t rows = Knobs<FakeCtx>::table().size();
    CHECK(rows == sizeof(cases) / sizeof(cases[0]));   // (and nothing the list above does not know)
    std::vector<long> defaults;
    { FakeCtx c; for (auto& k : cases) defaults.push_back(k.get(c)); }
    for (size_t i = 0; i < rows; ++i) {
        const KnobCase& k = cases[i];
        for (int v : {1, 0, 7, -3}) {
            const long want = k.is_bool ? (v != 0) : !std::strcmp(k.option ? k.option : "", "async_relinearise_test_delay_ms") ? v :
                              !std::strcmp(k.option ? k.option : "", "async_relinearise_journal_max") ? (v > 0 ? v : 1) : (v > 0 ? v : 0);
            if (k.option) {
                FakeCtx c;
                CHECK(Knobs<FakeCtx>::set_option(c, k.option, v) == LV_OK && k.get(c) == want);
                for (size_t j = 0; j < rows; ++j) CHECK(j == i || cases[j].get(c) == defaults[j]);   // ... and nowhere else
            }
            if (k.env) {
                FakeCtx c;
                char val[16];
                snprintf(val, sizeof(val), "%d", v);
                setenv(k.env, val, 1);
                CHECK(Knobs<FakeCtx>::read_environment(c) == LV_OK && k.get(c) == want);
                for (size_t j = 0; j < rows; ++j) CHECK(j == i || cases[j].get(c) == defaults[j]);
                unsetenv(k.env);
            }
        }
        if (!k.option) {   // fixed at creation: not an option
            FakeCtx c;
            CHECK(Knobs<FakeCtx>::set_option(c, k.env, 1) == LV_EINVAL);
        }
    }
    FakeCtx c;
    CHECK(Knobs<FakeCtx>::read_environment(c) == LV_OK);
    for (size_t j = 0; j < rows; ++j) CHECK(cases[j].get(c) == defaults[j]);   // (nothing set: nothing moves)
    CHECK(Knobs<FakeCtx>::set_option(c, "no_such_knob", 1) == LV_EINVAL && !std::strcmp(g_err, "lv_set_option: unknown option 'no_such_knob'"));
    // batch_predict flushes the queue that was filled under the other rule first
    g_drv = &c.upd;
    CHECK(c.upd.alloc(8) == LV_OK && c.filter.alloc() == LV_OK);
    CHECK(c.filter.set(reinterpret_cast<const lv_state*>(seed(1.0).x), seed(1.0).P) == LV_OK);
    CHECK(c.filter.predict(c.stream, c.upd.d_kf, 0.01, g_Q, g_acc, g_gyro) == LV_OK && c.filter.n == 1);
    const size_t t = mark();
    CHECK(Knobs<FakeCtx>::set_option(c, "batch_predict", 0) == LV_OK && c.filter.n == 0 && !c.filter.batch_predict);
    CHECK(count(calls(t), "launch_predict") == 1);
    // inside an update lv_set_option asks busy() first
    c.upd.in_update = true;
    CHECK(c.upd.busy("lv_set_option") == LV_ESTATE);
    c.upd.release(), c.filter.release();
    g_drv = nullptr;
}

// seeded random sequences of set / predict / correct / update / iterate / get with failing launches, against what the caller sees
void random_sequence(unsigned seed_value) {
    std::mt19937 rng(seed_value);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    Rig r;
    Logical m;   // the filter as the caller sees it
    int gets = 0, failed = 0;
    for (int op = 0; op < 1500; ++op) {
        const int k = pick(100);
        const bool fail = pick(12) == 0;
        if (fail) { static const char* what[] = {"launch_pass", "launch_search", "launch_fit_reduce", "launch_solve"}; g_fail_prefix = what[pick(4)], arm(-2); }
        if (k < 10 || (!m.set && k < 40)) {
            m = seed(op * 0.5);
            CHECK(r.set(m) == LV_OK);
        } else if (k < 30) {
            const int rc = r.predict(0.001 * (1 + op % 5));
            CHECK(rc == (m.set ? LV_OK : LV_ESTATE));
            if (m.set) m = predicted(m, 0.001 * (1 + op % 5));
        } else if (k < 50) {
            int passes = 0;
            const int rc = r.d.correct(r.in(), pick(2) ? &passes : nullptr);
            if (!m.set) CHECK(rc == LV_ESTATE);
            else if (rc != LV_OK) { CHECK(fail && rc == LV_EHIP); m.set = false; ++failed; }
            else m = updated(m);
        } else if (k < 70) {
            Logical o;
            const int rc = r.get(o);
            CHECK(rc == (m.set ? LV_OK : LV_ESTATE));
            if (m.set) { CHECK(same(o, m)); ++gets; }
        } else if (k < 85) {
            Logical v = seed(1000.0 + op);
            const Logical v0 = v;
            int passes = 0;
            const int rc = r.update(v, &passes);
            if (rc != LV_OK) { CHECK(fail && rc == LV_EHIP && same(v, v0)); ++failed; }
            else CHECK(same(v, updated(v0)) && passes == 4);
        } else if (k < 90) {
            lv_sums out;
            const Logical v = seed(2000.0 + op);
            const int rc = r.d.iterate(r.in(), reinterpret_cast<const lv_state*>(v.x), &out);
            CHECK(rc == LV_OK || (fail && rc == LV_EHIP));
        } else if (k < 94) {
            r.d.fused_pass = pick(2), r.d.capture = pick(4) == 0, r.filter.mail_filter = pick(2);
        } else if (k < 97) {
            r.n = pick(3) == 0 ? 0 : 100 + pick(9000);
            r.d.new_scan();
        } else {
            CHECK(r.filter.flush(r.s, r.d.d_kf) == LV_OK);   // (lv_synchronize)
        }
        arm(-1);
        CHECK(!r.d.in_update && !r.d.begin_pending);
        CHECK((r.filter.where == Where::Unset) == !m.set);
    }
    CHECK(gets > 60 && failed > 5);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: update_emu <scenario>\n"); return 2; }
    for (int k = 0; k < 144; ++k) g_Q[k] = 1e-3 * (k + 1);
    emu_hip::state().fail = [](const char* call) {
        if (g_hook) g_hook(call);
        if (g_fail_at == -2) return std::strncmp(call, g_fail_prefix.c_str(), g_fail_prefix.size()) == 0;
        return g_fail_at >= 0 && g_calls_seen++ == g_fail_at;
    };
    const std::string s = argv[1];
    if (s == "fused_by_value") fused_by_value();
    else if (s == "three_kernel_by_value") three_kernel_by_value();
    else if (s == "route_table") route_table();
    else if (s == "iterate") iterate();
    else if (s == "split_api") split_api();
    else if (s == "failures_by_value") failures_by_value();
    else if (s == "failures_correct") failures_correct();
    else if (s == "update_end") update_end();
    else if (s == "peer_failure") peer_failure();
    else if (s == "update_no_map") update_no_map();
    else if (s == "correct") correct();
    else if (s == "buffers") buffers();
    else if (s == "knobs") knobs();
    else if (s.rfind("random", 0) == 0) random_sequence((unsigned)std::stoul(s.substr(6)));
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees && st.events_created == st.events_destroyed);
    printf("ok %s\n", s.c_str());
    return 0;
}
