// tests/emu/exchange_emu.cpp — HOST test of the multi-rank exchange (limo-velo_amd/csrc/lv_exchange.hpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_exchange_host.py into tests/emu/_build/ (once plain, once with AddressSanitizer +
// UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own RankExchange against the stand-in hip_runtime.h next
// to this file, with logged fakes of lv_comm.hip (comm_*) and lv_peer.hip (peer_*): peer_export / peer_close allocate and free
// through the stand-in's counted hipMalloc / hipFree, peer_init points buf[] into that allocation, and a test sets peer_failed.
// The drivers below call the class exactly as the entry points of lv_api.hip do; the HIP stand-in logs every call, so a scenario
// asserts what each step did.  Usage: exchange_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <random>
#include <thread>

#include "../../limo-velo_amd/csrc/lv_exchange.hpp"

using namespace lv;
using T = RankExchange::Transport;

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

// ---- what the fakes saw
struct Seen {
    int init_rank = -1, init_world = -1;
    void* destroyed = nullptr;
    void* reduce_comm = nullptr; const double* reduce_record = nullptr;
    void* gather_comm = nullptr; const double* gather_buf = nullptr; size_t gather_count = 0; int gather_rank = -1;
    size_t export_cap = 0;
    int peer_parity = -1; size_t peer_slot = 0;
};
Seen g_seen;
bool g_has_allgather = true;
bool g_peer_failed = false;
int g_init_fails = 0;      // comm_init returns this (0: succeeds)
int g_export_fails = 0;    // 1: peer_export fails before it allocates, 2: after (its allocation stays behind, as lv_peer.hip's may)

}  // namespace

// ---- the fakes of lv_comm.hip
int lv::comm_init(const char*, const void*, int rank, int world, void** comm_out) {
    emu_hip::call("comm_init");
    g_seen.init_rank = rank, g_seen.init_world = world;
    if (g_init_fails) return set_error("ncclCommInitRank failed"), g_init_fails;
    *comm_out = emu_hip::new_handle<void*>();
    return LV_OK;
}
int lv::comm_destroy(void* comm) { emu_hip::call("comm_destroy"); g_seen.destroyed = comm; return LV_OK; }
int lv::comm_allreduce_record(void* comm, double* record, hipStream_t s) {
    emu_hip::call("comm_allreduce_record", s);
    g_seen.reduce_comm = comm, g_seen.reduce_record = record;
    return LV_OK;
}
bool lv::comm_has_allgather() { return g_has_allgather; }
int lv::comm_allgather_inplace(void* comm, double* buf, size_t count, int rank, hipStream_t s) {
    emu_hip::call("comm_allgather_inplace", s);
    g_seen.gather_comm = comm, g_seen.gather_buf = buf, g_seen.gather_count = count, g_seen.gather_rank = rank;
    return LV_OK;
}
// ---- the fakes of lv_peer.hip
int lv::peer_export(PeerSet& P, size_t cap, void*) {
    emu_hip::call("peer_export");
    if (P.local_alloc) return set_error("peer buffers already exported"), LV_ESTATE;
    g_seen.export_cap = cap;
    if (g_export_fails == 1) return set_error("export failed"), LV_EHIP;
    CHECK(hipMalloc(&P.local_alloc, 2 * cap * sizeof(double)) == hipSuccess);
    if (g_export_fails == 2) return set_error("export failed"), LV_EHIP;
    P.cap = cap;
    return LV_OK;
}
int lv::peer_init(PeerSet& P, int rank, int world, const void*) {
    emu_hip::call("peer_init");
    CHECK(P.local_alloc && !P.active);   // (RankExchange refuses everything else itself)
    if (world < 1 || world > LV_PEER_MAX || rank < 0 || rank >= world) return set_error("peer exchange: rank %d of %d", rank, world), LV_EINVAL;
    P.buf[0] = static_cast<double*>(P.local_alloc), P.buf[1] = P.buf[0] + P.cap;
    P.rank = rank, P.world = world, P.active = true;
    return LV_OK;
}
int lv::peer_gather(PeerSet& P, int parity, size_t slot, hipStream_t s) {
    emu_hip::call("peer_gather", s);
    CHECK(P.active);
    g_seen.peer_parity = parity, g_seen.peer_slot = slot;
    return LV_OK;
}
bool lv::peer_failed(const PeerSet& P) { return P.active && g_peer_failed; }
void lv::peer_close(PeerSet& P) {
    emu_hip::call("peer_close");
    hipFree(P.local_alloc);
    P = PeerSet();
}

namespace {

using Calls = std::vector<std::string>;
size_t mark() { return emu_hip::state().log.size(); }
Calls calls(size_t from) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i) v.push_back(log[i].call);
    return v;
}
long live() { return emu_hip::state().mallocs - emu_hip::state().frees; }
const Calls kGrow = {"hipStreamSynchronize", "hipFree", "hipFree", "hipMalloc", "hipMemset", "hipMalloc", "hipMemset"};
bool zero(const double* p, size_t n) { for (size_t i = 0; i < n; ++i) if (p[i] != 0.0) return false; return true; }
int noop_gather(void*, void*, size_t, int, int) { return 0; }

// a context as lv_api.hip holds it: the exchange, the stream, the grid limit; the drivers are the entry points' bodies
struct Ctx {
    RankExchange x;
    hipStream_t s = emu_hip::new_handle<hipStream_t>();
    int max_wg = 64;
    char id[128] = {}, blob[LV_PEER_BLOB] = {};
    int init(int r, int w) { return x.init_rccl(nullptr, id, r, w); }
    int host_gather(int r, int w, lv_gather_fn fn = noop_gather, void* user = nullptr) { return x.set_host_gather(s, r, w, fn, user); }
    int remove_gather() { return x.set_host_gather(s, 1, 3, nullptr, this); }   // (rank, world and user are ignored)
    int peer_export() { return x.peer_export(s, max_wg, blob); }
    int peer_init(int r, int w) { return x.peer_init(s, r, w, blob); }
    int destroy() { return x.destroy(s); }
    // lv_comm_set_shard_max, with a stand-in for pass_grid_size (one workgroup per 256 points, at most max_wg) and 32-double partials
    static size_t slot_for(size_t n, int max_wg) { return (size_t)std::min<size_t>((n + 255) / 256, (size_t)max_wg) * 32u; }
    int shard_max(size_t n) {
        if (n > 0xFFFFFFF0ull) return set_error("shard too large"), LV_EINVAL;
        x.shard_max = n;
        if (!x.multi_rank() || n == 0) return LV_OK;
        return x.reserve(s, slot_for(n, max_wg));
    }
    void release() { x.release_comm(s); x.release(); }   // lv_destroy
};

// each transport set up on a fresh context (PeerMapped: rank 1 of 2)
void setup(Ctx& c, T t) {
    if (t == T::Rccl) CHECK(c.init(1, 2) == LV_OK);
    if (t == T::HostGather) CHECK(c.host_gather(1, 2) == LV_OK);
    if (t == T::PeerExported || t == T::PeerMapped) CHECK(c.peer_export() == LV_OK);
    if (t == T::PeerMapped) CHECK(c.peer_init(1, 2) == LV_OK);
    CHECK(c.x.transport == t);
}

// ---- scenarios
void exclusive() {
    for (T t : {T::Rccl, T::HostGather, T::PeerExported, T::PeerMapped}) {
        Ctx c;
        setup(c, t);
        CHECK(c.shard_max(4096) == LV_OK);
        const RankExchange before = c.x;
        const size_t m = mark();
        const long mallocs = emu_hip::state().mallocs, frees = emu_hip::state().frees;
        auto refused = [&](int rc, const char* what) {
            CHECK(rc == LV_ESTATE && std::strstr(g_err, what));
            CHECK(calls(m).empty() && emu_hip::state().mallocs == mallocs && emu_hip::state().frees == frees);
            CHECK(c.x.transport == t && c.x.rank == before.rank && c.x.world == before.world && c.x.shard_max == before.shard_max);
            CHECK(c.x.d_gather[0] == before.d_gather[0] && c.x.gather_cap == before.gather_cap && c.x.comm == before.comm);
        };
        const char* here = t == T::Rccl ? "lv_comm_init" : t == T::HostGather ? "lv_comm_set_host_gather" : "lv_comm_peer_export";
        if (t != T::Rccl) refused(c.init(0, 2), here);
        else refused(c.init(0, 2), "lv_comm_init: a library communicator (lv_comm_init) is in place");
        if (t != T::HostGather) {
            refused(c.host_gather(0, 2), here);
            refused(c.remove_gather(), here);
        }
        if (t == T::Rccl || t == T::HostGather) refused(c.peer_export(), here);
        if (t == T::Rccl || t == T::HostGather) refused(c.peer_init(0, 2), "lv_comm_peer_export first");
        if (t == T::PeerMapped) refused(c.peer_init(0, 2), "already set up");
        if (t == T::PeerExported || t == T::PeerMapped) {   // a second export: refused by lv::peer_export, behind the synchronise
            CHECK(c.peer_export() == LV_ESTATE && std::strstr(g_err, "already exported"));
            CHECK((calls(m) == Calls{"hipStreamSynchronize", "peer_export"}) && c.x.transport == t);
            CHECK(emu_hip::state().mallocs == mallocs && emu_hip::state().frees == frees);
        }
        c.release();
    }
    Ctx c;   // arguments: a host gather with a bad rank is refused before the stream is touched
    const size_t m = mark();
    CHECK(c.host_gather(2, 2) == LV_EINVAL && c.host_gather(0, 0) == LV_EINVAL && calls(m).empty() && c.x.transport == T::None);
    g_init_fails = LV_EHIP;   // a failed comm_init leaves nothing in place
    CHECK(c.init(0, 2) == LV_EHIP && c.x.transport == T::None && c.x.comm == nullptr && c.x.world == 1);
    g_init_fails = 0;
    for (int how = 1; how <= 2; ++how) {   // a failed export: it counts as one if it left its allocation behind
        g_export_fails = how;
        CHECK(c.peer_export() == LV_EHIP);
        g_export_fails = 0;
        CHECK(c.x.transport == (how == 1 ? T::None : T::PeerExported));
        if (how == 2) CHECK(c.init(0, 2) == LV_ESTATE && c.destroy() == LV_OK && c.x.transport == T::None);
    }
    c.release();
}
void host_gather_remove() {
    Ctx c;
    size_t m = mark();
    c.x.shard_max = 777;
    CHECK(c.host_gather(1, 2) == LV_OK);
    CHECK(calls(m) == Calls{"hipStreamSynchronize"});
    CHECK(c.x.transport == T::HostGather && c.x.rank == 1 && c.x.world == 2 && c.x.shard_max == 0 && c.x.multi_rank() && c.x.gather_only());
    const size_t slot = Ctx::slot_for(3000, c.max_wg);
    m = mark();
    CHECK(c.shard_max(3000) == LV_OK);
    Calls want = {"hipStreamSynchronize", "hipHostMalloc"};
    want.insert(want.end(), kGrow.begin(), kGrow.end());
    CHECK(calls(m) == want);
    CHECK(c.x.shard_max == 3000 && c.x.h_gather_cap == 2 * slot && c.x.gather_cap == 2 * slot && zero(c.x.h_gather, 2 * slot));
    CHECK(c.x.fused_ready(3000) && !c.x.fused_ready(3001) && c.x.fits(slot) && !c.x.fits(slot + 1));
    // replaced by a world of 3: the shard is unknown again, and sizing grows the staging for three ranks
    CHECK(c.host_gather(2, 3) == LV_OK && c.x.shard_max == 0 && !c.x.fused_ready(1) && c.x.world == 3);
    CHECK(c.shard_max(3000) == LV_OK && c.x.h_gather_cap == 3 * slot && c.x.gather_cap == 3 * slot);
    double* const staging = c.x.h_gather;
    // removed: rank 0 of 1, shard unknown, the staging kept
    m = mark();
    CHECK(c.remove_gather() == LV_OK);
    CHECK(calls(m) == Calls{"hipStreamSynchronize"});
    CHECK(c.x.transport == T::None && c.x.rank == 0 && c.x.world == 1 && c.x.shard_max == 0 && !c.x.multi_rank());
    CHECK(c.x.gather_cb == nullptr && c.x.gather_user == nullptr && c.x.h_gather == staging && c.x.h_gather_cap == 3 * slot);
    m = mark();
    CHECK(c.shard_max(100000) == LV_OK && c.x.shard_max == 100000 && calls(m).empty());   // (stored, nothing sized: one rank)
    CHECK(c.shard_max(0x100000000ull) == LV_EINVAL && c.x.shard_max == 100000);
    CHECK(c.remove_gather() == LV_OK);   // (removing what is not there)
    c.release();
}
void reserve_grows() {
    {   // a communicator: device buffers only
        Ctx c;
        setup(c, T::Rccl);
        size_t m = mark();
        CHECK(c.shard_max(1000) == LV_OK && calls(m) == kGrow);
        const size_t s1 = Ctx::slot_for(1000, c.max_wg);
        CHECK(c.x.gather_cap == 2 * s1 && c.x.h_gather == nullptr && c.x.h_gather_cap == 0);
        CHECK(zero(c.x.d_gather[0], 2 * s1) && zero(c.x.d_gather[1], 2 * s1));
        double* const b0 = c.x.d_gather[0];
        m = mark();
        CHECK(c.shard_max(300) == LV_OK && calls(m).empty() && c.x.gather_cap == 2 * s1 && c.x.d_gather[0] == b0);   // never shrinks
        const long frees = emu_hip::state().frees;
        CHECK(c.shard_max(20000) == LV_OK && calls(m) == kGrow && emu_hip::state().frees == frees + 2);
        const size_t s2 = Ctx::slot_for(20000, c.max_wg);
        CHECK(c.x.gather_cap == 2 * s2 && zero(c.x.d_gather[0], 2 * s2) && zero(c.x.d_gather[1], 2 * s2));
        c.x.d_gather[0][0] = 5.0;
        m = mark();
        CHECK(c.shard_max(0) == LV_OK && c.x.shard_max == 0 && calls(m).empty() && c.x.d_gather[0][0] == 5.0);
        c.release();
    }
    {   // a host gather: the staging grows too, and only when it must
        Ctx c;
        setup(c, T::HostGather);
        CHECK(c.shard_max(256 * 10) == LV_OK && c.x.h_gather_cap == 2 * 320);
        c.x.h_gather[3] = 1.0;
        const size_t m = mark();
        CHECK(c.shard_max(256 * 5) == LV_OK && calls(m).empty() && c.x.h_gather[3] == 1.0);
        c.release();
    }
    {   // a mapped peer set: its capacity, and LV_EINVAL beyond it (the shard stays stored)
        Ctx c;
        c.max_wg = 2;   // (cap: (2 + 8) x 96 x 8 doubles)
        setup(c, T::PeerMapped);
        const size_t cap = (size_t)(c.max_wg + 8) * 96u * LV_PEER_MAX;
        CHECK(c.x.gather_cap == cap && g_seen.export_cap == cap);
        size_t m = mark();
        CHECK(c.shard_max(512) == LV_OK && calls(m).empty());
        c.max_wg = 1000;   // (a larger grid than the export was sized for)
        const size_t n = 256 * 500;
        m = mark();
        CHECK(c.shard_max(n) == LV_EINVAL && std::strstr(g_err, "exceed the exported buffers") && calls(m).empty());
        CHECK(c.x.shard_max == n && c.x.gather_cap == cap && c.x.d_gather[0] == c.x.peer.buf[0]);
        c.release();
    }
    {   // an export without its init: one rank, nothing sized
        Ctx c;
        setup(c, T::PeerExported);
        const size_t m = mark();
        CHECK(c.shard_max(5000) == LV_OK && calls(m).empty() && c.x.gather_cap == 0 && c.x.shard_max == 5000);
        c.release();
    }
}
void peer_lifecycle() {
    for (int with_init = 0; with_init < 2; ++with_init) {
        const long live0 = live();
        Ctx c;
        setup(c, T::HostGather);   // (buffers of this context's own, from an earlier transport)
        CHECK(c.shard_max(2000) == LV_OK && c.remove_gather() == LV_OK);
        double* const own0 = c.x.d_gather[0];
        size_t m = mark();
        CHECK(c.peer_export() == LV_OK);
        CHECK((calls(m) == Calls{"hipStreamSynchronize", "peer_export", "hipMalloc"}));
        CHECK(c.x.transport == T::PeerExported && !c.x.multi_rank() && c.x.world == 1 && c.x.d_gather[0] == own0);
        CHECK(g_seen.export_cap == (size_t)(c.max_wg + 8) * 96u * LV_PEER_MAX);
        if (with_init) {
            c.x.shard_max = 99;
            const long frees = emu_hip::state().frees;
            m = mark();
            CHECK(c.peer_init(1, 3) == LV_OK);
            CHECK((calls(m) == Calls{"peer_init", "hipStreamSynchronize", "hipFree", "hipFree"}) && emu_hip::state().frees == frees + 2);
            CHECK(c.x.transport == T::PeerMapped && c.x.multi_rank() && c.x.gather_only());
            CHECK(c.x.d_gather[0] == c.x.peer.buf[0] && c.x.d_gather[1] == c.x.peer.buf[1] && c.x.gather_cap == c.x.peer.cap);
            CHECK(c.x.rank == 1 && c.x.world == 3 && c.x.shard_max == 0 && c.x.nrec(7) == 21);
            CHECK(c.x.part_out(1, 10) == c.x.peer.buf[1] + 10);
            m = mark();
            CHECK(c.peer_init(0, 3) == LV_ESTATE && std::strstr(g_err, "already set up") && calls(m).empty());
            CHECK(c.x.exchange(c.s, 5, 64) == LV_OK && g_seen.peer_parity == 1 && g_seen.peer_slot == 64);
            CHECK(!c.x.failed());
            g_peer_failed = true;
            CHECK(c.x.failed());
            g_peer_failed = false;
        }
        c.x.shard_max = 42;
        const long frees = emu_hip::state().frees;
        m = mark();
        CHECK(c.destroy() == LV_OK);
        CHECK((calls(m) == Calls{"hipStreamSynchronize", "peer_close", "hipFree"}) && emu_hip::state().frees == frees + 1);
        CHECK(c.x.transport == T::None && c.x.rank == 0 && c.x.world == 1 && c.x.shard_max == 0 && !c.x.failed());
        if (with_init) CHECK(c.x.d_gather[0] == nullptr && c.x.d_gather[1] == nullptr && c.x.gather_cap == 0);
        else CHECK(c.x.d_gather[0] == own0);   // (still this context's)
        m = mark();
        CHECK(c.destroy() == LV_OK && calls(m).empty());
        CHECK(c.peer_export() == LV_OK && c.x.transport == T::PeerExported);   // (a new exchange after the teardown)
        c.release();
        CHECK(live() == live0);
    }
}
void release_each() {
    for (int grown = 0; grown < 3; ++grown) {   // 0: as set up, 1: then sized, 2: sized under a host gather first
        for (T t : {T::None, T::Rccl, T::HostGather, T::PeerExported, T::PeerMapped}) {
            const long live0 = live();
            Ctx c;
            if (grown == 2) CHECK(c.host_gather(0, 2) == LV_OK && c.shard_max(7000) == LV_OK && c.remove_gather() == LV_OK);
            if (t != T::None) setup(c, t);
            if (grown) CHECK(c.shard_max(256 * 40) == (LV_OK));
            void* const comm = c.x.comm;
            const size_t m = mark();
            c.release();
            CHECK(live() == live0);
            const Calls v = calls(m);
            if (t == T::Rccl) CHECK(v.size() >= 2 && v[0] == "hipStreamSynchronize" && v[1] == "comm_destroy" && g_seen.destroyed == comm);
            else CHECK(std::count(v.begin(), v.end(), std::string("comm_destroy")) == 0);
        }
    }
}
// two ranks in two threads: the callback swaps their slots through shared memory
struct Shared {
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0, generation = 0;
    std::vector<double> slots;
    struct Seen { size_t bytes; int rank, world; void* staging; };
    std::vector<Seen> seen[2];
    void barrier() {
        std::unique_lock<std::mutex> g(mu);
        const int gen = generation;
        if (++arrived == 2) { arrived = 0; ++generation; cv.notify_all(); }
        else cv.wait(g, [&] { return generation != gen; });
    }
};
struct RankArg { Shared* sh; };
int swap_gather(void* user, void* slots, size_t bytes, int rank, int world) {
    RankArg* a = static_cast<RankArg*>(user);
    a->sh->seen[rank].push_back({bytes, rank, world, slots});
    const size_t n = bytes / sizeof(double);
    { std::lock_guard<std::mutex> g(a->sh->mu); std::memcpy(a->sh->slots.data() + rank * n, static_cast<double*>(slots) + rank * n, bytes); }
    a->sh->barrier();
    { std::lock_guard<std::mutex> g(a->sh->mu); std::memcpy(static_cast<double*>(slots) + (1 - rank) * n, a->sh->slots.data() + (1 - rank) * n, bytes); }
    a->sh->barrier();
    return 0;
}
double pattern(int rank, int launch, size_t j) { return rank * 1e6 + launch * 1e3 + (double)j; }
void host_gather_two_ranks() {
    Shared sh;
    const size_t slot = Ctx::slot_for(256 * 3, 64);
    sh.slots.assign(2 * slot, 0.0);
    bool ok[2] = {false, false};
    auto run = [&](int rank) {
        Ctx c;
        RankArg arg{&sh};
        CHECK(c.host_gather(rank, 2, swap_gather, &arg) == LV_OK);
        CHECK(c.shard_max(256 * 3) == LV_OK && c.x.fused_ready(256 * 2) && c.x.fits(slot) && c.x.nrec(3) == 6);
        for (int launch = 0; launch < 4; ++launch) {
            const int p = launch & 1;
            double* own = c.x.part_out(p, slot);
            CHECK(own == c.x.d_gather[p] + rank * slot);
            for (size_t j = 0; j < slot; ++j) own[j] = pattern(rank, launch, j);   // (this rank's pass kernel)
            CHECK(c.x.exchange(c.s, launch, slot) == LV_OK);
            for (int r = 0; r < 2; ++r)
                for (size_t j = 0; j < slot; ++j) CHECK(c.x.d_gather[p][r * slot + j] == pattern(r, launch, j));
        }
        c.release();
        ok[rank] = true;
    };
    std::thread t0(run, 0), t1(run, 1);
    t0.join();
    t1.join();
    CHECK(ok[0] && ok[1]);
    for (int r = 0; r < 2; ++r) {
        CHECK(sh.seen[r].size() == 4);
        for (const auto& s : sh.seen[r]) CHECK(s.bytes == slot * sizeof(double) && s.rank == r && s.world == 2 && s.staging);
    }
}
int failing_gather(void*, void*, size_t, int, int) { return 3; }
void host_gather_failure() {
    Ctx c;
    CHECK(c.host_gather(0, 2, failing_gather) == LV_OK && c.shard_max(256) == LV_OK);
    const size_t m = mark();
    CHECK(c.x.exchange(c.s, 3, 32) == LV_ESTATE);
    CHECK(std::strcmp(g_err, "host gather callback failed (launch 3)") == 0);
    CHECK((calls(m) == Calls{"hipMemcpyAsync", "hipStreamSynchronize"}));   // (nothing copied back)
    CHECK(c.x.refuse_unfused() == LV_ESTATE && std::strstr(g_err, "does not take the one-launch-per-pass form"));
    c.release();
}
void rccl_calls() {
    Ctx c;
    CHECK(c.init(2, 3) == LV_OK);
    CHECK(g_seen.init_rank == 2 && g_seen.init_world == 3 && c.x.comm != nullptr && c.x.rank == 2 && c.x.world == 3);
    CHECK(c.x.multi_rank() && !c.x.gather_only() && !c.x.fused_ready(100));   // (no shard told)
    CHECK(c.shard_max(256 * 8) == LV_OK && c.x.fused_ready(256 * 8) && c.x.nrec(8) == 24);
    g_has_allgather = false;
    CHECK(!c.x.fused_ready(256 * 8));
    g_has_allgather = true;
    c.x.fused = false;
    CHECK(!c.x.fused_ready(256 * 8));
    c.x.fused = true;
    size_t m = mark();
    CHECK(c.x.exchange(c.s, 3, 256) == LV_OK && calls(m) == Calls{"comm_allgather_inplace"});
    CHECK(g_seen.gather_comm == c.x.comm && g_seen.gather_buf == c.x.d_gather[1] && g_seen.gather_count == 256 && g_seen.gather_rank == 2);
    CHECK(c.x.part_out(0, 256) == c.x.d_gather[0] + 512);
    double record[96];
    CHECK(c.x.allreduce(c.s, record) == LV_OK && g_seen.reduce_comm == c.x.comm && g_seen.reduce_record == record);
    void* const comm = c.x.comm;
    m = mark();
    CHECK(c.destroy() == LV_OK);
    CHECK((calls(m) == Calls{"hipStreamSynchronize", "comm_destroy"}) && g_seen.destroyed == comm);
    CHECK(c.x.transport == T::None && c.x.comm == nullptr && c.x.rank == 0 && c.x.world == 1);
    CHECK(c.x.shard_max == 256 * 8);   // (a communicator's teardown keeps the shard)
    CHECK(c.init(0, 1) == LV_OK && c.x.fused_ready(0));   // (again, world 1: the shard and the buffers are still there)
    c.release();
}
// seeded random sequences against a model of the transport, rank, world, shard, capacities and allocations
void random_sequence(unsigned seed_value) {
    std::mt19937 rng(seed_value);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    auto ctx = std::make_unique<Ctx>();
    const long live0 = live();
    struct Model { T t = T::None; int rank = 0, world = 1; size_t shard = 0, cap = 0, hcap = 0, peer_cap = 0; bool own = false; } m;
    int counts[5] = {};
    for (int op = 0; op < 2000; ++op) {
        Ctx& c = *ctx;
        const int r = pick(100);
        const int w = 1 + pick(4), rk = pick(w);
        if (r < 10) {
            const int rc = c.init(rk, w);
            CHECK(rc == (m.t == T::None ? LV_OK : LV_ESTATE));
            if (!rc) m.t = T::Rccl, m.rank = rk, m.world = w;
        } else if (r < 22) {
            const bool remove = pick(3) == 0;
            const int rc = remove ? c.remove_gather() : c.host_gather(rk, w);
            CHECK(rc == (m.t == T::None || m.t == T::HostGather ? LV_OK : LV_ESTATE));
            if (!rc) m.t = remove ? T::None : T::HostGather, m.rank = remove ? 0 : rk, m.world = remove ? 1 : w, m.shard = 0;
        } else if (r < 30) {
            const int rc = c.peer_export();
            CHECK(rc == (m.t == T::None ? LV_OK : LV_ESTATE));
            if (!rc) m.t = T::PeerExported, m.peer_cap = (size_t)(c.max_wg + 8) * 96u * LV_PEER_MAX;
        } else if (r < 38) {
            const int rc = c.peer_init(rk, w);
            CHECK(rc == (m.t == T::PeerExported ? LV_OK : LV_ESTATE));
            if (!rc) m.t = T::PeerMapped, m.rank = rk, m.world = w, m.shard = 0, m.cap = m.peer_cap, m.own = false;
        } else if (r < 48) {
            CHECK(c.destroy() == LV_OK);
            if (m.t == T::PeerExported || m.t == T::PeerMapped) m.shard = 0;
            if (m.t == T::PeerMapped) m.cap = 0;
            if (m.t != T::HostGather) m.t = T::None, m.rank = 0, m.world = 1;
        } else if (r < 78) {
            c.max_wg = pick(4) == 0 ? 1000 : 64;
            const size_t n = pick(5) == 0 ? 0 : (size_t)pick(256 * 2000);
            const int rc = c.shard_max(n);
            m.shard = n;
            const bool multi = m.t == T::Rccl || m.t == T::HostGather || m.t == T::PeerMapped;
            const size_t need = Ctx::slot_for(n, c.max_wg) * (size_t)m.world;
            const bool over = multi && n && need > m.cap;
            CHECK(rc == (over && m.t == T::PeerMapped ? LV_EINVAL : LV_OK));
            if (multi && n && m.t == T::HostGather) m.hcap = std::max(m.hcap, need);
            if (over && m.t != T::PeerMapped) m.cap = need, m.own = true;
        } else if (r < 88) {
            const uint32_t scan_n = (uint32_t)pick(256 * 2000);
            const bool ready = m.shard && scan_n <= m.shard && m.cap;
            CHECK(c.x.fused_ready(scan_n) == ready);
            if (ready && c.x.multi_rank() && c.x.fits(Ctx::slot_for(m.shard, c.max_wg))) {
                const int launch = pick(8);
                CHECK(c.x.exchange(c.s, launch, Ctx::slot_for(m.shard, c.max_wg)) == LV_OK);
            }
        } else if (r < 94) {
            c.release();
            CHECK(live() == live0);
            ctx = std::make_unique<Ctx>();
            m = Model();
        } else {
            CHECK(c.x.failed() == false && c.x.refuse_unfused() == LV_ESTATE);
        }
        const Ctx& k = *ctx;
        ++counts[(int)m.t];
        CHECK(k.x.transport == m.t && k.x.rank == m.rank && k.x.world == m.world && k.x.shard_max == m.shard);
        CHECK(k.x.gather_cap == m.cap && k.x.h_gather_cap == m.hcap);
        CHECK(k.x.multi_rank() == (m.t == T::Rccl || m.t == T::HostGather || m.t == T::PeerMapped));
        CHECK(k.x.gather_only() == (m.t == T::HostGather || m.t == T::PeerMapped));
        if (m.t == T::PeerMapped) CHECK(k.x.d_gather[0] == k.x.peer.buf[0] && k.x.d_gather[1] == k.x.peer.buf[1]);
        else CHECK((k.x.d_gather[0] != nullptr) == m.own && (k.x.d_gather[1] != nullptr) == m.own);
        const bool peer = m.t == T::PeerExported || m.t == T::PeerMapped;
        CHECK(live() - live0 == (m.own ? 2 : 0) + (m.hcap ? 1 : 0) + (peer ? 1 : 0));
    }
    ctx->release();
    CHECK(live() == live0);
    for (int t = 0; t < 5; ++t) CHECK(counts[t] > 20);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: exchange_emu <scenario>\n"); return 2; }
    const std::string s = argv[1];
    if (s == "exclusive") exclusive();
    else if (s == "host_gather_remove") host_gather_remove();
    else if (s == "reserve_grows") reserve_grows();
    else if (s == "peer_lifecycle") peer_lifecycle();
    else if (s == "release_each") release_each();
    else if (s == "host_gather_two_ranks") host_gather_two_ranks();
    else if (s == "host_gather_failure") host_gather_failure();
    else if (s == "rccl_calls") rccl_calls();
    else if (s.rfind("random", 0) == 0) random_sequence((unsigned)std::stoul(s.substr(6)));
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees);
    printf("ok %s\n", s.c_str());
    return 0;
}
