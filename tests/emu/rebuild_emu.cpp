// tests/emu/rebuild_emu.cpp — HOST test of the background map rebuild (limo-velo_amd/csrc/lv_rebuild.hpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_rebuild_host.py into tests/emu/_build/ (once plain, once with ThreadSanitizer),
// never shipped.  It compiles the product's own MapRebuild template against the stand-in hip_runtime.h next to this file,
// instantiated with FakeStore: a "map" kept as a host vector whose operations can be held at a gate or made to fail on the
// worker thread.  Each scenario drives the class exactly as the map entry points of lv_api.hip do and compares the active
// store with a reference store that saw the same operations directly.  Usage: rebuild_emu <scenario>; exit status 0 = pass.
#include <hip/hip_runtime.h>

#include <array>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <set>
#include <thread>
#include <tuple>

#include <sys/syscall.h>
#include <unistd.h>

#include "../../limo-velo_amd/csrc/lv_rebuild.hpp"

using namespace lv;

// ---- what lv_rebuild.hpp takes from the rest of the library
static thread_local char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* lv_last_error(void) { return g_err; }
static std::atomic<uint32_t> g_pause_us{0};   // what the worker set
void lv::set_slice_pause_us(uint32_t us) { g_pause_us = us; }

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            fflush(stderr);                                                             \
            std::_Exit(1);                                                              \
        }                                                                               \
    } while (0)

namespace {

// ---- gates and failures: they act on the worker thread only (the caller's threads set t_caller)
thread_local bool t_caller = false;
std::mutex g_mu;
std::condition_variable g_cv;
std::map<std::string, std::pair<bool, bool>> g_gate;   // name -> {closed, reached}
std::set<std::string> g_fail;

void close_gate(const std::string& n) { std::lock_guard<std::mutex> g(g_mu); g_gate[n] = {true, false}; }
void open_gate(const std::string& n) { std::lock_guard<std::mutex> g(g_mu); g_gate[n].first = false; g_cv.notify_all(); }
// (bounded: a worker that never arrives fails the scenario.  A timed condition-variable wait is not used: this libstdc++ makes it
// with pthread_cond_clockwait, which ThreadSanitizer does not see release the mutex)
void wait_until(const std::function<bool()>& done) {
    const auto t0 = std::chrono::steady_clock::now();
    while (!done()) {
        CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10));
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}
void wait_reached(const std::string& n) {
    wait_until([&] { std::lock_guard<std::mutex> g(g_mu); return g_gate[n].second; });
}
// a caller thread that has entered `body`: waits until the kernel shows it blocked in one of `syscalls` — the point inside the
// product call the scenario must reach before it lets the worker go on (read from /proc, so no sleep decides the path taken)
struct Caller {
    std::atomic<long> tid{0};
    std::thread t;
    explicit Caller(std::function<void()> body) : t([this, body] { t_caller = true; tid = syscall(SYS_gettid); body(); }) {}
    void wait_blocked_in(std::initializer_list<long> syscalls) {
        wait_until([&] {
            if (!tid) return false;
            char path[64];
            snprintf(path, sizeof(path), "/proc/self/task/%ld/syscall", tid.load());
            FILE* f = fopen(path, "r");
            CHECK(f);
            long nr = -1;
            if (fscanf(f, "%ld", &nr) != 1) nr = -1;   // ("running")
            fclose(f);
            for (long s : syscalls) if (nr == s) return true;
            return false;
        });
    }
};

void fail_on_worker(const std::string& n) { std::lock_guard<std::mutex> g(g_mu); g_fail.insert(n); }
int worker_step(const char* n) {   // a gated / failing step of a store operation
    if (t_caller) return LV_OK;
    std::unique_lock<std::mutex> g(g_mu);
    auto& gate = g_gate[n];
    gate.second = true;
    g_cv.notify_all();
    g_cv.wait(g, [&] { return !g_gate[n].first; });
    if (g_fail.count(n)) { lv::set_error("emulated failure of %s", n); return LV_EHIP; }
    return LV_OK;
}

std::atomic<uint32_t> g_worker_slice_wgs{0};                 // the slice size the copy carried into its reserve
std::atomic<size_t> g_snap_capacity{0}, g_snap_m{0};      // the last snapshot: the copy's capacity, the points taken

bool alive(const float4& p) { return std::isfinite(p.x); }
std::tuple<int, int, int> box_of(const float4& p, float b) { return {(int)std::floor(p.x / b), (int)std::floor(p.y / b), (int)std::floor(p.z / b)}; }

struct FakeStore;
std::set<FakeStore*> g_stores;   // (main thread only: the worker creates no store)

// The map as the rebuild sees a MapStore: points by id (dead: x = +inf), living count, statistics.  add_staged keeps a point
// unless, with down-sampling, a living point (or an earlier one of the batch) shares its box — a rule that depends on the point
// set and the id order only, like the real one; evictions drop a box's inside / outside or the oldest living.
struct FakeStore {
    std::vector<float4> pts;
    size_t capacity = 0;
    uint32_t n_ids = 0, m = 0;
    bool built = false, defer_relinearise = false, have_boxes = false;
    uint32_t slice_wgs = 0;
    uint64_t relinearisations = 0, incremental_adds = 0, dropped_total = 0;
    std::vector<float4> staging;
    float4* d_new = nullptr;
    size_t batch_cap = 0;

    FakeStore() { g_stores.insert(this); }
    FakeStore(FakeStore&& o) noexcept { g_stores.insert(this); *this = std::move(o); }
    FakeStore& operator=(FakeStore&&) = default;
    ~FakeStore() { g_stores.erase(this); }

    void load(const std::vector<float4>& p) {   // lv_map_build
        pts = p;
        n_ids = m = (uint32_t)p.size();
        capacity = std::max(capacity, p.size());
        built = true;
    }
    std::vector<float4> living() const {
        std::vector<float4> out;
        for (auto& p : pts) if (alive(p)) out.push_back(p);
        return out;
    }
    void kill(uint32_t id) { pts[id].x = INFINITY; --m; }

    int reserve(size_t cap) {
        if (!t_caller) g_worker_slice_wgs = slice_wgs;
        if (int rc = worker_step("reserve")) return rc;
        capacity = std::max(capacity, cap);
        return LV_OK;
    }
    int rebuild(hipStream_t s) {
        emu_hip::call("rebuild", s);
        if (int rc = worker_step("rebuild")) return rc;
        built = true;
        return LV_OK;
    }
    int reserve_batch(size_t k) {
        if (k > batch_cap) { staging.resize(k); batch_cap = k; d_new = staging.data(); }
        return LV_OK;
    }
    int add_staged(hipStream_t s, uint32_t k, int downsample, float box, bool build_if_empty) {
        emu_hip::call("add_staged", s);
        if (int rc = worker_step("add")) return rc;
        const bool rule = downsample && !(build_if_empty && m == 0);
        std::set<std::tuple<int, int, int>> taken;
        if (rule) for (auto& p : pts) if (alive(p)) taken.insert(box_of(p, box));
        for (uint32_t i = 0; i < k; ++i) {
            const float4 p = d_new[i];
            if (rule && !taken.insert(box_of(p, box)).second) { ++dropped_total; continue; }
            pts.push_back(p);
            ++n_ids;
            ++m;
        }
        capacity = std::max(capacity, pts.size());
        built = true;
        ++incremental_adds;
        return LV_OK;
    }
    int settle(hipStream_t) { return LV_OK; }
    int evict_box(hipStream_t s, const float lo[3], const float hi[3], int keep_inside, uint32_t* n_evicted) {
        emu_hip::call("evict_box", s);
        if (int rc = worker_step("evict")) return rc;
        uint32_t ne = 0;
        for (uint32_t id = 0; id < n_ids; ++id) {
            const float4 p = pts[id];
            if (!alive(p)) continue;
            const bool in = p.x >= lo[0] && p.x <= hi[0] && p.y >= lo[1] && p.y <= hi[1] && p.z >= lo[2] && p.z <= hi[2];
            if (in != (keep_inside != 0)) { kill(id); ++ne; }
        }
        if (n_evicted) *n_evicted = ne;
        return LV_OK;
    }
    int evict_oldest(hipStream_t s, uint32_t n, uint32_t* n_evicted) {
        emu_hip::call("evict_oldest", s);
        if (int rc = worker_step("evict")) return rc;
        uint32_t ne = 0;
        for (uint32_t id = 0; id < n_ids && ne < n; ++id) if (alive(pts[id])) { kill(id); ++ne; }
        if (n_evicted) *n_evicted = ne;
        return LV_OK;
    }
    bool wants_relinearise(size_t) const { return n_ids > 0 && (uint64_t)(n_ids - m) * 3 >= n_ids; }
    int snapshot_into(FakeStore& dst, hipStream_t s) {
        emu_hip::call("snapshot_into", s);
        g_snap_capacity = dst.capacity;
        g_snap_m = m;
        if (dst.capacity < m) { lv::set_error("snapshot: the copy is too small"); return LV_EINVAL; }
        dst.pts = living();
        dst.n_ids = dst.m = m;
        return LV_OK;
    }
    int ensure_boxes(hipStream_t, float) { have_boxes = true; return LV_OK; }
    void refresh_view() {}
    void release() { *this = FakeStore(); }
};

std::vector<float4> points(size_t n, uint32_t seed, float lo = -5.f, float span = 10.f) {
    std::vector<float4> p(n);
    uint32_t s = seed * 2654435761u + 1;
    auto u = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / (float)(1u << 24); };
    for (auto& q : p) q = make_float4(lo + span * u(), lo + span * u(), lo + span * u(), 0.f);
    return p;
}

bool same(const std::vector<float4>& a, const std::vector<float4>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(float4)));
}

// A context: the active store, its streams and the rebuild, driven the way lv_api.hip's entry points drive them; `ref` sees every
// operation directly (no rebuild).
struct Ctx {
    FakeStore map, ref;
    MapRebuild<FakeStore> rb;
    hipStream_t stream = nullptr, side = nullptr;
    hipEvent_t staged = nullptr;
    bool overlap = true;

    explicit Ctx(size_t arena_bytes = 1u << 20) : rb(arena_bytes) {
        CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess);
        CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking) == hipSuccess);
        CHECK(hipEventCreateWithFlags(&staged, hipEventDisableTiming) == hipSuccess);
        CHECK(rb.create_streams(0) == LV_OK);
        rb.opt.async_min = 1;
    }
    void destroy() {   // lv_destroy
        rb.release(map, cs());
        map.release();
        hipEventDestroy(staged);
        hipStreamDestroy(side);
        hipStreamDestroy(stream);
    }
    CtxStreams cs() const { return {stream, side, staged, overlap}; }
    FakeStore& shadow() {   // the rebuild's second store
        for (FakeStore* s : g_stores) if (s != &map && s != &ref) return *s;
        CHECK(false);
        return map;
    }

    void build(const std::vector<float4>& p) {   // lv_map_build
        rb.cancel(map, cs());
        map.load(p);
        ref.load(p);
    }
    int poll() { return rb.poll(map, cs()); }
    // lv_map_add (scan: lv_map_add_scan); before_journal runs between the staging of the batch and its journal entry
    void add(const std::vector<float4>& p, int downsample, bool scan = false, const std::function<void()>& before_journal = {}) {
        const uint32_t n = (uint32_t)p.size();
        CHECK(poll() == LV_OK);
        CHECK(rb.maybe_start(map, n) == LV_OK);
        CHECK(map.reserve_batch(n) == LV_OK);
        CHECK(hipMemcpyAsync(map.d_new, p.data(), n * sizeof(float4), hipMemcpyHostToDevice, stream) == hipSuccess);
        if (before_journal) before_journal();
        CHECK(rb.journal_add(map, cs(), n, downsample, 0.2f, scan) == LV_OK);
        const hipStream_t is = map.built && map.m > 0 ? cs().side_behind() : stream;
        CHECK(rb.order(cs(), is) == LV_OK);
        CHECK(map.add_staged(is, n, downsample, 0.2f, scan) == LV_OK);
        ref.reserve_batch(n);
        std::memcpy(ref.d_new, p.data(), n * sizeof(float4));
        CHECK(ref.add_staged(stream, n, downsample, 0.2f, scan) == LV_OK);
    }
    void evict_box(const float lo[3], const float hi[3], int keep_inside, const std::function<void()>& before_journal = {}) {
        CHECK(poll() == LV_OK);
        if (before_journal) before_journal();
        CHECK(rb.journal_evict(map, cs(), 2, lo, hi, keep_inside, 0) == LV_OK);
        CHECK(rb.order(cs(), stream) == LV_OK);
        uint32_t a = 0, b = 0;
        CHECK(map.evict_box(stream, lo, hi, keep_inside, &a) == LV_OK);
        CHECK(ref.evict_box(stream, lo, hi, keep_inside, &b) == LV_OK);
        CHECK(a == b);
    }
    void evict_oldest(uint32_t n) {
        CHECK(poll() == LV_OK);
        CHECK(rb.journal_evict(map, cs(), 3, nullptr, nullptr, 0, n) == LV_OK);
        CHECK(rb.order(cs(), stream) == LV_OK);
        CHECK(map.evict_oldest(stream, n, nullptr) == LV_OK);
        CHECK(ref.evict_oldest(stream, n, nullptr) == LV_OK);
    }
    std::array<uint64_t, 4> status(int wait = 0) {
        std::array<uint64_t, 4> out{};
        CHECK(rb.status(map, cs(), wait, out.data()) == LV_OK);
        return out;
    }
    void wait_state(RebuildState s) {   // (status(0) does not poll, so nothing is adopted meanwhile)
        wait_until([&] { return status()[0] == (uint64_t)s; });
    }
    // a map with a third of its ids dead (what makes maybe_start start a rebuild)
    void start_state() {
        build(points(600, 1));
        const float lo[3] = {-5, -5, -5}, hi[3] = {1.5f, 5, 5};
        evict_box(lo, hi, 1);
        CHECK(map.wants_relinearise(0));
    }
    // start a rebuild and take its snapshot; the worker then holds at the "rebuild" gate
    void to_rebuilding() {
        close_gate("rebuild");
        CHECK(rb.start(map) == LV_OK);
        wait_state(RebuildState::Allocated);
        CHECK(poll() == LV_OK);
        CHECK(status()[0] == (uint64_t)RebuildState::Rebuilding);
        wait_reached("rebuild");
    }
    void check_map() { CHECK(same(map.living(), ref.living())); CHECK(map.m == ref.m); }
};

void check_balanced() {
    auto& s = emu_hip::state();
    CHECK(s.mallocs == s.frees);
    CHECK(s.events_created == s.events_destroyed);
    CHECK(s.streams_created == s.streams_destroyed);
}

const float BOX_LO[3] = {-2, -2, -5}, BOX_HI[3] = {2, 2, 5};

// 1. Idle -> Allocating -> Allocated -> (snapshot at the next poll) Rebuilding -> Ready -> (adopted at the next poll) Idle
void full_cycle() {
    Ctx c;
    c.start_state();
    c.map.relinearisations = 5;
    c.map.incremental_adds = 7;
    c.map.dropped_total = 3;
    close_gate("reserve");
    close_gate("rebuild");
    CHECK(c.rb.start(c.map) == LV_OK);
    c.rb.opt.pause_us = 999;    // the live options change while the worker runs: it must go on with the copy start() took
    c.rb.opt.slice_wgs = 7;
    c.rb.opt.test_delay_ms = 1000000;
    auto s = c.status();
    CHECK(s[0] == (uint64_t)RebuildState::Allocating && s[1] == 1 && s[2] == 0);
    CHECK(c.map.defer_relinearise);
    CHECK(c.poll() == LV_OK);   // (allocating: nothing to do)
    wait_reached("reserve");
    CHECK(c.status()[0] == (uint64_t)RebuildState::Allocating);
    open_gate("reserve");
    c.wait_state(RebuildState::Allocated);
    CHECK(c.poll() == LV_OK);   // the snapshot
    CHECK(c.status()[0] == (uint64_t)RebuildState::Rebuilding);
    CHECK(g_snap_m == c.map.m);
    wait_reached("rebuild");
    open_gate("rebuild");
    c.wait_state(RebuildState::Ready);
    CHECK(g_pause_us == 100 && g_worker_slice_wgs == 256);
    CHECK(c.poll() == LV_OK);   // adopted
    s = c.status();
    CHECK(s[0] == (uint64_t)RebuildState::Idle && s[1] == 1 && s[2] == 1 && s[3] == 0);
    CHECK(c.map.relinearisations == 6 && c.map.incremental_adds == 7 && c.map.dropped_total == 3);
    CHECK(!c.map.defer_relinearise && !c.shadow().defer_relinearise);
    CHECK(c.map.n_ids == c.map.m);   // (the adopted store is the compacted copy)
    c.check_map();
    c.destroy();
    check_balanced();
}

// 2. what the active map went through while the copy was rebuilt is replayed on the copy in order
void replay_in_order() {
    Ctx c;
    c.start_state();
    c.to_rebuilding();
    c.add(points(150, 2), 1);
    c.evict_oldest(40);
    c.add(points(120, 3), 0);
    c.evict_box(BOX_LO, BOX_HI, 0);
    c.add(points(100, 4), 1, true);
    c.evict_oldest(25);
    c.evict_box(BOX_LO, BOX_HI, 1);
    c.add(points(80, 5, -2.f, 4.f), 1);
    CHECK(c.status()[3] == 8);
    open_gate("rebuild");
    c.wait_state(RebuildState::Ready);
    CHECK(c.status()[3] == 0);
    CHECK(c.poll() == LV_OK);
    CHECK(c.status()[2] == 1);
    CHECK(c.map.n_ids < c.ref.n_ids);   // (the copy, not the old store)
    c.check_map();
    c.destroy();
    check_balanced();
}

// 3. a worker that falls journal_max operations behind is given up: the copy is dropped, async switched off, the map untouched
void journal_bound() {
    Ctx c;
    c.rb.opt.journal_max = 3;
    c.start_state();
    c.to_rebuilding();
    c.add(points(50, 2), 1);
    c.evict_oldest(10);
    c.evict_box(BOX_LO, BOX_HI, 0);
    CHECK(c.status()[3] == 3);
    // the fourth operation cancels the copy, which joins the worker: it is let go once the entry was refused (its event freed)
    const long destroyed = emu_hip::state().events_destroyed;
    std::thread helper([&] { t_caller = true; c.add(points(60, 3), 1); });
    wait_until([&] { return emu_hip::state().events_destroyed != destroyed; });
    open_gate("rebuild");
    helper.join();
    auto s = c.status();
    CHECK(s[0] == (uint64_t)RebuildState::Idle && s[2] == 0 && s[3] == 0);
    CHECK(!c.rb.opt.async);
    CHECK(!c.map.defer_relinearise);
    c.check_map();
    CHECK(c.map.n_ids == c.ref.n_ids);   // (the active store, never swapped)
    c.add(points(40, 6), 0);            // the map still wants a rebuild: with async off nothing starts
    CHECK(c.map.wants_relinearise(0));
    CHECK(c.rb.maybe_start(c.map, 10) == LV_OK);
    CHECK(c.status()[1] == 1);
    c.destroy();
    check_balanced();
}

// 4. the worker reports Ready between a call's poll and its journal entry: the call adopts the copy and acts on it
void adoption_race() {
    for (int evict = 0; evict < 2; ++evict) {
        Ctx c;
        c.start_state();
        c.to_rebuilding();
        c.add(points(70, 2), 1);
        auto ready = [&] { open_gate("rebuild"); c.wait_state(RebuildState::Ready); };
        if (evict) c.evict_box(BOX_LO, BOX_HI, 0, ready);
        else c.add(points(90, 3), 1, false, ready);
        auto s = c.status();
        CHECK(s[0] == (uint64_t)RebuildState::Idle && s[2] == 1 && s[3] == 0);
        CHECK(c.map.n_ids < c.ref.n_ids);   // (adopted)
        c.check_map();
        c.add(points(30, 4), 1);
        c.check_map();
        c.destroy();
        check_balanced();
    }
}

// 5. cancel in Allocating (as lv_map_build), in Allocated (as lv_map_relinearise) and in Rebuilding (as lv_destroy)
void cancel() {
    for (int at = 0; at < 3; ++at) {
        Ctx c;
        c.start_state();
        if (at == 0) {
            close_gate("reserve");
            CHECK(c.rb.start(c.map) == LV_OK);
            wait_reached("reserve");
            // the cancel finds the worker still allocating: it waits (sleeping between looks) until the worker reaches its wait
            Caller helper([&] { c.build(points(300, 9)); });
            helper.wait_blocked_in({SYS_nanosleep, SYS_clock_nanosleep});
            open_gate("reserve");
            helper.t.join();
        } else if (at == 1) {
            CHECK(c.rb.start(c.map) == LV_OK);
            c.wait_state(RebuildState::Allocated);
            c.rb.cancel(c.map, c.cs());
        } else {
            c.to_rebuilding();
            c.add(points(40, 2), 1);
            c.evict_oldest(5);
            // the cancel finds the worker rebuilding: it joins it, and the worker then replays what is journaled
            Caller helper([&] { c.destroy(); });
            helper.wait_blocked_in({SYS_futex});
            CHECK(c.status()[0] == (uint64_t)RebuildState::Rebuilding);
            open_gate("rebuild");
            helper.t.join();
            check_balanced();
            continue;
        }
        auto s = c.status();
        CHECK(s[0] == (uint64_t)RebuildState::Idle && s[2] == 0 && s[3] == 0);
        CHECK(!c.map.defer_relinearise);
        CHECK(c.rb.opt.async);
        auto& h = emu_hip::state();
        CHECK(h.mallocs - h.frees == 1);   // (the journal arena, kept for the next rebuild)
        c.check_map();
        c.destroy();
        check_balanced();
    }
}

// 6. the worker fails (reserve, the wait for the snapshot, rebuild, a replay): Failed; the next poll drops the copy, says so on
// stderr and turns async off; the map is as it was
void worker_failure() {
    for (int where = 0; where < 4; ++where) {
        {
            std::lock_guard<std::mutex> g(g_mu);
            g_fail.clear();
        }
        emu_hip::state().fail = nullptr;
        Ctx c;
        c.start_state();
        if (where == 0) fail_on_worker("reserve");
        if (where == 1) emu_hip::state().fail = [](const char* call) { return !t_caller && !std::strcmp(call, "hipStreamWaitEvent"); };
        if (where == 2) fail_on_worker("rebuild");
        if (where == 3) fail_on_worker("add");
        if (where == 3) {
            c.to_rebuilding();
            c.add(points(50, 2), 1);
            open_gate("rebuild");
        } else {
            CHECK(c.rb.start(c.map) == LV_OK);
            if (where) {
                c.wait_state(RebuildState::Allocated);
                CHECK(c.poll() == LV_OK);
            }
        }
        c.wait_state(RebuildState::Failed);
        CHECK(c.poll() == LV_OK);
        auto s = c.status();
        CHECK(s[0] == (uint64_t)RebuildState::Idle && s[2] == 0 && s[3] == 0);
        CHECK(!c.rb.opt.async);
        CHECK(!c.map.defer_relinearise);
        c.check_map();
        CHECK(c.map.n_ids == c.ref.n_ids);
        emu_hip::state().fail = nullptr;
        c.destroy();
        check_balanced();
    }
}

// 7. the map outgrows the copy's slack while the worker allocates: the snapshot's poll reserves the copy for m + 1
void outgrow() {
    Ctx c;
    c.start_state();
    const size_t m0 = c.map.m;
    close_gate("reserve");
    close_gate("rebuild");
    CHECK(c.rb.start(c.map) == LV_OK);
    wait_reached("reserve");
    c.add(points(m0 / 8 + 262144 + 100, 7), 0);   // (Allocating: nothing journaled, the snapshot will hold it)
    open_gate("reserve");
    c.wait_state(RebuildState::Allocated);
    CHECK(c.poll() == LV_OK);
    CHECK(c.status()[0] == (uint64_t)RebuildState::Rebuilding);
    CHECK(g_snap_m == c.map.m && g_snap_capacity == (size_t)c.map.m + 1);
    open_gate("rebuild");
    c.status(1);
    c.check_map();
    CHECK(c.status()[2] == 1);
    c.destroy();
    check_balanced();
}

// 8. the journal arena is exhausted: the entry gets an allocation of its own, freed after its replay
void arena_exhausted() {
    Ctx c(4096);   // room for one batch of 200 points (3 328 bytes), not two
    c.start_state();
    c.to_rebuilding();
    auto& h = emu_hip::state();
    const long outstanding = h.mallocs - h.frees;   // (the arena)
    c.add(points(200, 2), 1);
    CHECK(h.mallocs - h.frees == outstanding);
    c.add(points(200, 3), 0);
    CHECK(h.mallocs - h.frees == outstanding + 1);
    open_gate("rebuild");
    c.wait_state(RebuildState::Ready);
    CHECK(h.mallocs - h.frees == outstanding);
    CHECK(c.poll() == LV_OK);
    c.check_map();
    c.destroy();
    check_balanced();
}

// 9. a snapshot on the side stream: the first mutation enqueued on the context's stream waits for it, later ones do not
void stream_order() {
    Ctx c;
    c.start_state();
    close_gate("rebuild");   // (the copy must not be adopted before the last check: adoption ends the ordering)
    CHECK(c.rb.start(c.map) == LV_OK);
    c.wait_state(RebuildState::Allocated);
    auto& h = emu_hip::state();
    auto log_from = [&](size_t i) { std::lock_guard<std::mutex> g(h.mu); return std::vector<emu_hip::Call>(h.log.begin() + i, h.log.end()); };
    auto log_size = [&] { std::lock_guard<std::mutex> g(h.mu); return h.log.size(); };
    size_t at = log_size();
    CHECK(c.poll() == LV_OK);
    hipEvent_t snap = nullptr;
    {
        auto l = log_from(at);
        size_t i = 0;
        while (i < l.size() && l[i].call != "snapshot_into") ++i;
        CHECK(i >= 2 && i + 1 < l.size());
        CHECK(l[i].stream == c.side);
        CHECK(l[i - 2].call == "hipEventRecord" && l[i - 2].event == c.staged && l[i - 2].stream == c.stream);
        CHECK(l[i - 1].call == "hipStreamWaitEvent" && l[i - 1].event == c.staged && l[i - 1].stream == c.side);
        CHECK(l[i + 1].call == "hipEventRecord" && l[i + 1].stream == c.side);
        snap = l[i + 1].event;
    }
    auto waits_on_snap = [&](size_t from, hipStream_t s) {
        for (auto& e : log_from(from)) if (e.call == "hipStreamWaitEvent" && e.event == snap && e.stream == s) return true;
        return false;
    };
    at = log_size();
    c.add(points(50, 2), 1);   // (on the side stream, behind the snapshot already)
    CHECK(!waits_on_snap(at, c.side) && !waits_on_snap(at, c.stream));
    at = log_size();
    c.evict_oldest(5);
    {
        auto l = log_from(at);
        size_t w = l.size(), m = l.size();
        for (size_t i = 0; i < l.size(); ++i) {
            if (w == l.size() && l[i].call == "hipStreamWaitEvent" && l[i].event == snap && l[i].stream == c.stream) w = i;
            if (m == l.size() && l[i].call == "evict_oldest" && l[i].stream == c.stream) m = i;
        }
        CHECK(w < m && m < l.size());
    }
    at = log_size();
    c.evict_box(BOX_LO, BOX_HI, 0);
    c.evict_oldest(3);
    CHECK(!waits_on_snap(at, c.stream));
    open_gate("rebuild");
    c.status(1);
    c.check_map();
    c.destroy();
    check_balanced();
}

// 10. status(wait = 1) drives a rebuild to its end and returns at Idle
void status_wait() {
    Ctx c;
    c.start_state();
    c.map.relinearisations = 2;
    CHECK(c.rb.start(c.map) == LV_OK);
    auto s = c.status(1);
    CHECK(s[0] == (uint64_t)RebuildState::Idle && s[1] == 1 && s[2] == 1 && s[3] == 0);
    CHECK(c.map.relinearisations == 3 && !c.map.defer_relinearise);
    c.check_map();
    c.destroy();
    check_balanced();
}

}  // namespace

int main(int argc, char** argv) {
    t_caller = true;
    const std::map<std::string, void (*)()> scenarios = {
        {"full_cycle", full_cycle},         {"replay_in_order", replay_in_order}, {"journal_bound", journal_bound},
        {"adoption_race", adoption_race},   {"cancel", cancel},                   {"worker_failure", worker_failure},
        {"outgrow", outgrow},               {"arena_exhausted", arena_exhausted}, {"stream_order", stream_order},
        {"status_wait", status_wait},
    };
    if (argc != 2 || !scenarios.count(argv[1])) {
        fprintf(stderr, "usage: rebuild_emu <scenario>\n");
        return 2;
    }
    scenarios.at(argv[1])();
    printf("ok %s\n", argv[1]);
    return 0;
}
