// lv_rebuild.hpp — background re-linearisation of the map (row f-1; ikd-Tree rebuilds beside its searches too: the tree is
// constructed with delete / balance criteria 0.3 / 0.6, src/Modules/Mapper.cpp:65, and rebuilds sub-trees on a second thread).
//
// When the active map wants a compaction (MapStore::wants_relinearise: a third of its id space is dead) and holds at least
// RebuildOptions::async_min points, a compacted copy of its living points is taken (one launch chain on the context's stream) and
// its search structure is rebuilt by a WORKER THREAD on a stream of its own, while searches and inserts go on against the active
// map; every mutation of the active map in the meantime is journaled (a device copy of the staged batch) and replayed on the copy
// by the worker; the stores are swapped at the next map call after the worker has caught up.  The map's point set, id order and
// hence every search result are the same as with the stop-the-world rebuild (tests/test_gpu_map_async.py; the state machine and
// its locking on the host: tests/test_rebuild_host.py).
//
// The product instantiates MapRebuild<MapStore> once, in lv_ctx; the template parameter lets the host test substitute a fake store.
// The class touches the active store and the context's streams only as the caller hands them over, call by call.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>

#include "../../include/limovelo_hip.h"
#include "lv_common.hpp"

namespace lv {

// lv_map_rebuild_status reports these in out[0] (include/limovelo_hip.h): the numbers are ABI.  The cycle is
// Idle -> Allocating -> Allocated -> (snapshot) Rebuilding -> Ready -> (adopted) Idle; Failed until the next poll drops the copy.
enum class RebuildState : int { Idle = 0, Rebuilding = 1, Ready = 2, Failed = 3, Allocating = 4, Allocated = 5 };

struct RebuildOptions {
    bool async = true;             // lv_set_option "async_relinearise" / LV_ASYNC_RELINEARISE=0: always stop-the-world
    size_t async_min = 200000;     // "async_relinearise_min": smaller maps rebuild in ~2 ms: not worth a thread
    size_t journal_max = 4096;     // "async_relinearise_journal_max": journal entries beyond which a rebuild that cannot keep up is
                                   // given up: the copy is cancelled and the active map takes the stop-the-world path
                                   // when it needs one
    uint32_t pause_us = 100;       // LV_RELIN_PAUSE_US / "async_relinearise_pause_us": the worker's slices are spaced by that long (lv_map.hip launch_sliced):
                                   // a cycle beside the rebuild 0.25 instead of 0.29 ms, p99 0.53-0.57 instead of 0.62-0.68, the rebuild ~8 x longer in wall time
                                   // (profiles/experiments_r06/rebuild_spaced_slices_ab.txt); 0: slices back to back
    uint32_t slice_wgs = 256;      // LV_RELIN_SLICE_WGS / "async_relinearise_slice_wgs": slice size of the worker's large launches (0: whole grids).  (Round 5's
                                   // opt-in PACED form — the grids as at most 32 looping 1024-thread workgroups — is gone: p99 0.5 instead of 0.6 ms, but two
                                   // 4.6 ms cycles in 5 of 17 replays that plain slices never showed, cause not found: profiles/experiments_r05/async_rebuild.txt §10-11)
    int test_delay_ms = 0;         // "async_relinearise_test_delay_ms": the worker pauses between rebuild and replay (tests)
    bool test_race = false;        // "async_relinearise_test_race": see journal_add (tests)
};

// The context's streams, as a call hands them to the rebuild
struct CtxStreams {
    hipStream_t stream;   // the context's stream (its own or the caller's)
    hipStream_t side;     // its side stream (lv_map_add_scan's insert runs there); may be null
    hipEvent_t staged;    // the event that orders the side stream behind `stream`
    bool overlap;         // work may move to the side stream: it exists, overlap_insert is on and `stream` is the context's own
    // the side stream, ordered behind what `stream` holds so far, when the overlap applies and HIP agrees; `stream` otherwise
    hipStream_t side_behind() const {
        if (!overlap || hipEventRecord(staged, stream) != hipSuccess || hipStreamWaitEvent(side, staged, 0) != hipSuccess) return stream;
        return side;
    }
};

template <class Store>
class MapRebuild {
public:
    RebuildOptions opt;   // the live settings; a worker runs with the copy its start() took

    explicit MapRebuild(size_t arena_bytes = 64u << 20) : arena_bytes_(arena_bytes) {}

    // the worker's stream and the snapshot event, created when the context is (creating a stream costs ~15 ms: not inside a
    // cycle).  quiet (lv_create): what fails is left for the first start, which tries again, with a stream of default priority
    // as the fallback, and reports a failure
    int create_streams(int device, bool quiet = false) {
        device_ = device;
        if (!stream_) {
            // LOWEST priority: the rebuild's kernels sort and scatter millions of points; the cycle's small launches on the context's
            // streams must get the compute units as they free up, not queue behind them
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; (void)hipGetLastError(); }
            if (hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, lo) != hipSuccess) {
                stream_ = nullptr;
                (void)hipGetLastError();
                if (!quiet) LV_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
            }
        }
        if (!snapshot_) {
            if (!quiet) LV_HIP(hipEventCreateWithFlags(&snapshot_, hipEventDisableTiming));
            else if (hipEventCreateWithFlags(&snapshot_, hipEventDisableTiming) != hipSuccess) { snapshot_ = nullptr; (void)hipGetLastError(); }
        }
        return LV_OK;
    }

    // Called at the start of every map call (the map is settled): the cycle boundary the reference's loop gives us
    // (src/main.cpp:102).  An allocated copy gets its snapshot here (a launch chain, no allocation, no wait); a finished rebuild is
    // adopted here; a failed one is dropped (the stop-the-world path remains).
    int poll(Store& map, const CtxStreams& cs) {
        if (state_ == RebuildState::Idle) return LV_OK;
        const RebuildState st = locked_state();
        if (st == RebuildState::Rebuilding || st == RebuildState::Allocating) return LV_OK;
        if (st == RebuildState::Allocated) return snapshot(map, cs);
        if (worker_.joinable()) worker_.join();
        if (st == RebuildState::Failed) {
            //  a failed worker — out of memory for the second store is the likely, and persistent, cause — must not be
            // started again by the very call that found it failed: cancel lifts the deferral, and with the background form
            // switched off for this context the insert that follows takes the stop-the-world path (MapStore::needs_relinearise),
            // which rebuilds in place and needs no second store.  lv_set_option "async_relinearise" 1 turns it back on.
            fprintf(stderr, "[limovelo_hip] background map rebuild failed (%s); the map stays as it is, re-linearisations of this context stop the world from here on\n",
                    error_.c_str());
            give_up(map, cs);
            return LV_OK;
        }
        // Ready: the worker's stream is drained (it synchronised after its last operation).  Nothing the caller enqueued against
        // the old store is disturbed — its buffers stay allocated (it becomes the next rebuild's target, written by launches that
        // are ordered behind everything enqueued on the context's stream so far) — so the swap needs no wait at all.
        std::swap(map, shadow_);   // (shadow_ is the OLD active store from here on: it carries the history)
        map.slice_wgs = 0;
        snap_side_ = false;        // (the snapshot was complete before the worker's first launch)
        map.defer_relinearise = false;
        shadow_.defer_relinearise = false;
        map.relinearisations = shadow_.relinearisations + 1;
        map.incremental_adds = shadow_.incremental_adds;
        map.dropped_total = shadow_.dropped_total;
        map.refresh_view();
        state_ = RebuildState::Idle;
        arena_used_ = 0;
        ++adopted_;
        return LV_OK;
    }

    // start the worker (its first phase allocates; the snapshot follows at the next map call: poll)
    int start(Store& map) {
        if (state_ != RebuildState::Idle) return LV_OK;
        { int rs = create_streams(device_); if (rs) return rs; }
        map.defer_relinearise = true;
        error_.clear();
        state_ = RebuildState::Allocating;
        ++started_;
        worker_ = std::thread(&MapRebuild::worker_main, this, opt, copy_size(map));
        return LV_OK;
    }

    // an insert of n points is about to go to the active map: start a background rebuild if the map wants one
    int maybe_start(Store& map, size_t incoming) {
        if (state_ != RebuildState::Idle || !opt.async || !map.built || map.m < opt.async_min) return LV_OK;
        if ((uint64_t)map.n_ids + incoming > 0xFFFFFFF0ull) return LV_OK;     // id space exhausted: only the stop-the-world path helps
        if (!map.wants_relinearise(incoming)) return LV_OK;
        return start(map);
    }

    // a mutation of the active map is about to be enqueued on `s`: it must not overtake a snapshot that is being taken on the side stream
    int order(const CtxStreams& cs, hipStream_t s) {
        if (!snap_side_ || s == cs.side) return LV_OK;
        LV_HIP(hipStreamWaitEvent(s, snapshot_, 0));
        if (s == cs.stream) snap_side_ = false;   // (everything later on the context's stream is behind it as well)
        return LV_OK;
    }

    // journal a batch staged in map.d_new (copied on the context's stream, which staged it) for the worker to replay
    int journal_add(Store& map, const CtxStreams& cs, uint32_t n, int downsample, float box, bool build_if_empty) {
        if (n == 0) return LV_OK;
        if (opt.test_race && state_ == RebuildState::Rebuilding) {   // (test hook: let the worker report "ready" right here, between this call's poll and its journal entry)
            const auto t0 = std::chrono::steady_clock::now();
            while (state_ == RebuildState::Rebuilding && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(5))
                std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        RebuildState st = state_;
        if (st != RebuildState::Rebuilding && st != RebuildState::Ready) return LV_OK;   // (Allocating / Allocated: the snapshot is still to come and will contain this batch)
        if (st == RebuildState::Rebuilding) {
            Entry e;
            e.kind = build_if_empty ? 1 : 0;
            e.n = n;
            e.downsample = downsample;
            e.box = box;
            { int rc = copy_in(e, map.d_new, (size_t)n * sizeof(float4), cs.stream); if (rc) return rc; }
            if (push(e, st)) return LV_OK;
            free_entry(e);
            if (st == RebuildState::Rebuilding) {   // the worker does not drain the journal as fast as the caller fills it: give the copy up
                fprintf(stderr, "[limovelo_hip] background map rebuild cannot keep up (%zu journaled operations): cancelled; re-linearisations of this context stop the world from here on\n",
                        opt.journal_max);
                give_up(map, cs);
                return LV_OK;
            }
        }
        if (st == RebuildState::Ready) {
            // The worker caught up and reported "ready" after this call's poll: the copy no longer takes journal entries, so this
            // batch must go to the copy AS THE ACTIVE MAP — adopt it now and move the staged batch over (it sits in the old store's
            // staging buffer); the caller's add_staged then acts on the adopted store.
            float4* staged_old = map.d_new;
            int rc = poll(map, cs);
            if (rc) return rc;
            rc = map.reserve_batch(n);
            if (rc) return rc;
            LV_HIP(hipMemcpyAsync(map.d_new, staged_old, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, cs.stream));
        }
        return LV_OK;   // (Failed: the worker failed meanwhile — the active map simply stays)
    }

    // journal an eviction (kind 2: box lo / hi / keep_inside, 3: the n_oldest oldest) for the worker to replay
    int journal_evict(Store& map, const CtxStreams& cs, int kind, const float* lo, const float* hi, int keep_inside, uint32_t n_oldest) {
        if (state_ != RebuildState::Rebuilding && state_ != RebuildState::Ready) return LV_OK;
        Entry e;
        e.kind = kind;
        if (lo) for (int a = 0; a < 3; ++a) { e.lo[a] = lo[a]; e.hi[a] = hi[a]; }
        e.keep_inside = keep_inside;
        e.n_oldest = n_oldest;
        RebuildState st;
        if (push(e, st)) return LV_OK;
        if (st == RebuildState::Rebuilding) give_up(map, cs);   // (journal full: see journal_add)
        if (st == RebuildState::Ready) return poll(map, cs);    // (ready since this call's poll: adopt the copy first, the caller's eviction then acts on it)
        return LV_OK;
    }

    // The replay hook of an operation the rebuild does not know (kind 4, lv_map_remove_dynamic): called by the worker with the copy,
    // its stream and the worker's copy of the operation's device data; it returns an LV_ code.  The rule must be a pure function of
    // the points' coordinates and that data: ids differ between the stores.
    using Replay = std::function<int(Store&, hipStream_t, const void*)>;

    // journal such an operation: `bytes` of device data at `src` (copied on the context's stream, behind what produced them) travel
    // with it.  As journal_evict: nothing to do unless a rebuild is in flight; a full journal gives the copy up; a copy found
    // ready is adopted first, so the caller's own action then applies to it
    int journal_replay(Store& map, const CtxStreams& cs, const void* src, size_t bytes, Replay replay) {
        RebuildState st = state_;
        if (st != RebuildState::Rebuilding && st != RebuildState::Ready) return LV_OK;
        if (st == RebuildState::Rebuilding) {
            Entry e;
            e.kind = 4;
            e.replay = std::move(replay);
            { int rc = copy_in(e, src, bytes, cs.stream); if (rc) return rc; }
            if (push(e, st)) return LV_OK;
            free_entry(e);
        }
        if (st == RebuildState::Rebuilding) give_up(map, cs);   // (journal full: see journal_add)
        if (st == RebuildState::Ready) return poll(map, cs);    // (ready since this call's poll: see journal_evict)
        return LV_OK;
    }

    // join the worker and throw its work away (lv_map_build / lv_map_relinearise / lv_destroy while a rebuild is in flight)
    void cancel(Store& map, const CtxStreams& cs) {
        if (worker_.joinable()) {
            for (;;) {   // a worker that is still allocating reaches its wait first
                {
                    std::lock_guard<std::mutex> g(mu_);
                    if (state_ == RebuildState::Allocated) { state_ = RebuildState::Idle; cv_.notify_all(); }
                    if (state_ != RebuildState::Allocating) break;
                }
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
            worker_.join();
        }
        if (snap_side_) {   // (a snapshot may still be reading the active store on the side stream: build / relinearise rewrite it)
            if (cs.side) hipStreamSynchronize(cs.side);
            snap_side_ = false;
        }
        for (auto& e : journal_) free_entry(e);
        journal_.clear();
        state_ = RebuildState::Idle;
        arena_used_ = 0;
        map.defer_relinearise = false;
    }

    // Every allocation a background rebuild needs, made NOW (set-up time) instead of by the first rebuild's worker: the second store
    // is allocated for the map as it stands, filled from a snapshot and rebuilt once — synchronously, in whole grids — so that its id
    // buffers, pools and tables exist at the sizes a rebuild of this map takes, have been touched, and the journal arena is there.
    // The first background rebuild of the context then behaves like every later one (which find the previous active store waiting).
    int reserve(Store& map, const CtxStreams& cs) {
        if (state_ != RebuildState::Idle) { set_error("lv_map_reserve_rebuild: a background rebuild is in flight"); return LV_ESTATE; }
        if (!map.built || map.m == 0) return LV_OK;
        { int rs = create_streams(device_); if (rs) return rs; }
        Store& S = shadow_;
        S.n_ids = 0;
        S.m = 0;
        S.built = false;
        S.slice_wgs = 0;
        int rc = S.reserve(copy_size(map));
        if (rc) return rc;
        ensure_arena();
        LV_HIP(hipStreamSynchronize(cs.stream));
        if (cs.side) LV_HIP(hipStreamSynchronize(cs.side));
        rc = map.snapshot_into(S, cs.stream);
        if (!rc) rc = S.rebuild(cs.stream);
        if (!rc && map.batch_cap) rc = S.reserve_batch(map.batch_cap);
        if (!rc) rc = S.ensure_boxes(cs.stream, 0.2f);   // (the 0.2 m box table a down-sampling replay builds: Mapper.cpp:65)
        LV_HIP(hipStreamSynchronize(cs.stream));
        S.have_boxes = false;
        // (the copy's contents are not kept: the next rebuild takes its own snapshot)
        S.n_ids = 0;
        S.m = 0;
        S.built = false;
        return rc;
    }

    // out = {state, rebuilds started, rebuilds adopted, journaled operations not yet replayed}; wait: until a rebuild in flight is adopted
    int status(Store& map, const CtxStreams& cs, int wait, uint64_t out[4]) {
        if (wait && state_ != RebuildState::Idle) {
            { int rs = map.settle(cs.stream); if (rs) return rs; }
            for (;;) {   // allocating -> (snapshot) -> rebuilding -> ready -> adopted
                int rp = poll(map, cs);
                if (rp) return rp;
                if (locked_state() == RebuildState::Idle) break;
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
        }
        if (out) {
            {
                std::lock_guard<std::mutex> g(mu_);
                out[0] = (uint64_t)state_.load();
                out[3] = (uint64_t)journal_.size();
            }
            out[1] = started_;
            out[2] = adopted_;
        }
        return LV_OK;
    }

    // the rebuild's share of lv_destroy: join the worker, wait for the device (the old store may still be read by work of the
    // caller's), free the copy, the arena, the stream and the event
    void release(Store& map, const CtxStreams& cs) {
        cancel(map, cs);
        hipDeviceSynchronize();
        shadow_.release();
        if (arena_) hipFree(arena_);
        if (stream_) hipStreamDestroy(stream_);
        if (snapshot_) hipEventDestroy(snapshot_);
        arena_ = nullptr;
        stream_ = nullptr;
        snapshot_ = nullptr;
    }

private:
    struct Entry {
        int kind = 0;                     // 0 add (Add_Points rule), 1 add, building if empty (Mapper::add), 2 evict box, 3 evict oldest,
                                          // 4 the caller's replay hook (journal_replay)
        void* d_data = nullptr;           // device copy of the staged batch (kinds 0, 1) or of the hook's data (kind 4) (owned)
        Replay replay;
        uint32_t n = 0;
        int downsample = 0;
        float box = 0.2f;
        float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        int keep_inside = 0;
        uint32_t n_oldest = 0;
        hipEvent_t ready = nullptr;       // the copy has landed (recorded on the stream that made it)
        bool from_arena = false;
    };

    static size_t copy_size(const Store& map) { return (size_t)map.m + (size_t)map.m / 8 + 262144; }   // living points + slack

    static void free_entry(Entry& e) {
        if (e.d_data && !e.from_arena) hipFree(e.d_data);
        if (e.ready) hipEventDestroy(e.ready);
        e.d_data = nullptr;
        e.ready = nullptr;
    }

    // e.d_data = a copy of `bytes` at src, made on `s`; e.ready recorded behind it
    int copy_in(Entry& e, const void* src, size_t bytes, hipStream_t s) {
        const size_t rounded = (bytes + 255) & ~(size_t)255;
        if (arena_ && arena_used_ + rounded <= arena_bytes_) {   // a bump arena: no hipMalloc on the caller's thread
            e.d_data = static_cast<char*>(arena_) + arena_used_;
            e.from_arena = true;
            arena_used_ += rounded;
        } else {
            LV_HIP(hipMalloc(&e.d_data, bytes));
        }
        // (an error below must not leak the entry: ADVICE r05)
        hipError_t je = hipMemcpyAsync(e.d_data, src, bytes, hipMemcpyDeviceToDevice, s);
        if (je == hipSuccess) je = hipEventCreateWithFlags(&e.ready, hipEventDisableTiming);
        if (je == hipSuccess) je = hipEventRecord(e.ready, s);
        if (je != hipSuccess) {
            free_entry(e);
            set_error("map rebuild journal: %s", hipGetErrorString(je));
            return LV_EHIP;
        }
        return LV_OK;
    }

    RebuildState locked_state() {
        std::lock_guard<std::mutex> g(mu_);
        return state_;
    }

    // hands an entry to the worker if it is still rebuilding and the journal has room; `st`: the state the entry met
    bool push(const Entry& e, RebuildState& st) {
        std::lock_guard<std::mutex> g(mu_);
        st = state_;
        if (st != RebuildState::Rebuilding || journal_.size() >= opt.journal_max) return false;
        journal_.push_back(e);
        return true;
    }

    // drop the copy for good: bounded memory and bounded deferral; the context's re-linearisations stop the world from here on
    void give_up(Store& map, const CtxStreams& cs) {
        cancel(map, cs);
        opt.async = false;
    }

    void ensure_arena() {   // device memory the journal's batch copies are carved from (allocated once)
        if (!arena_ && hipMalloc(&arena_, arena_bytes_) != hipSuccess) { arena_ = nullptr; (void)hipGetLastError(); }
    }

    // snapshot of the active store into the allocated copy; the worker is told to go on
    int snapshot(Store& map, const CtxStreams& cs) {
        if ((size_t)map.m + 1 > shadow_.capacity) {   // (the map outgrew the slack while the worker was allocating: rare)
            int rr = shadow_.reserve((size_t)map.m + 1);
            if (rr) return rr;
        }
        // The snapshot only READS the active store: with the context's own stream it goes to the side stream (behind everything the
        // context's stream holds so far), where the inserts run as well — the cycle's next prediction / window / update do not queue
        // up behind the compaction of every id (0.3-0.4 ms at 10 M points: it was the slowest cycle of a rebuild).  What MUTATES the
        // map afterwards is ordered behind it: inserts by running on the side stream, anything on the context's stream by order().
        const hipStream_t ss = cs.side_behind();
        int rc = map.snapshot_into(shadow_, ss);
        if (rc) return rc;
        LV_HIP(hipEventRecord(snapshot_, ss));
        snap_side_ = ss != cs.stream;
        std::lock_guard<std::mutex> g(mu_);
        state_ = RebuildState::Rebuilding;
        cv_.notify_all();
        return LV_OK;
    }

    // The worker, with the options of its start() and the id slots to allocate.  Phase 1 (Allocating): every allocation the copy
    // needs — the id-indexed buffers, the journal arena — happens HERE, not on the caller's thread (hipMalloc of ~1 GB takes ~20 ms
    // for a 10 M-point map); then it reports Allocated and sleeps until the caller has enqueued the snapshot (Rebuilding).  Phase 2:
    // rebuild the copy's search structure, then replay what the active map went through since the snapshot, until the journal is
    // empty at a moment the lock is held — from then on the two stores hold the same point set (Ready).
    void worker_main(RebuildOptions o, size_t want) {
        auto fail = [&](const char* what) {
            std::lock_guard<std::mutex> g(mu_);
            error_ = std::string(what) + ": " + lv_last_error();
            state_ = RebuildState::Failed;
        };
        if (hipSetDevice(device_) != hipSuccess) { fail("hipSetDevice"); return; }
        Store& S = shadow_;
        S.n_ids = 0;
        S.m = 0;
        S.built = false;
        // the worker's big kernels leave the compute units every ~0.1 ms (launch_sliced, lv_map.hip)
        S.slice_wgs = o.slice_wgs;
        set_slice_pause_us(o.pause_us);   // (this thread's launches only)
        if (S.reserve(want) != LV_OK) { fail("reserve"); return; }
        ensure_arena();
        {
            std::unique_lock<std::mutex> g(mu_);
            state_ = RebuildState::Allocated;
            cv_.wait(g, [&] { return state_ != RebuildState::Allocated; });
            if (state_ != RebuildState::Rebuilding) return;   // cancelled
        }
        const hipStream_t st = stream_;
        if (hipStreamWaitEvent(st, snapshot_, 0) != hipSuccess) { fail("wait for the snapshot"); return; }
        if (S.rebuild(st) != LV_OK) { fail("rebuild"); return; }
        if (o.test_delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(o.test_delay_ms));   // (test hook: lets the journal fill)
        for (;;) {
            Entry e;
            {
                std::lock_guard<std::mutex> g(mu_);
                if (journal_.empty()) { state_ = RebuildState::Ready; return; }
                e = journal_.front();
                journal_.pop_front();
            }
            int rc = LV_OK;
            if (e.kind <= 1) {
                if (hipStreamWaitEvent(st, e.ready, 0) != hipSuccess) rc = LV_EHIP;
                if (!rc) rc = S.reserve_batch(e.n);
                if (!rc && hipMemcpyAsync(S.d_new, e.d_data, (size_t)e.n * sizeof(float4), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = LV_EHIP;
                if (!rc) rc = S.add_staged(st, e.n, e.downsample, e.box, e.kind == 1);
                if (!rc) rc = S.settle(st);
            } else if (e.kind == 2) {
                rc = S.evict_box(st, e.lo, e.hi, e.keep_inside, nullptr);
            } else if (e.kind == 3) {
                rc = S.evict_oldest(st, e.n_oldest, nullptr);
            } else {
                if (hipStreamWaitEvent(st, e.ready, 0) != hipSuccess) rc = LV_EHIP;
                if (!rc) rc = e.replay(S, st, e.d_data);
            }
            if (hipStreamSynchronize(st) != hipSuccess) rc = rc ? rc : LV_EHIP;
            free_entry(e);
            if (rc) { fail("replay of a journaled map operation"); return; }
        }
    }

    Store shadow_;                      // the copy while a rebuild is in flight; the previous active store otherwise
    std::thread worker_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Entry> journal_;         // (under mu_)
    std::atomic<RebuildState> state_{RebuildState::Idle};   // written under mu_
    std::string error_;                 // the worker's failure (under mu_)
    hipStream_t stream_ = nullptr;      // the worker's stream
    hipEvent_t snapshot_ = nullptr;     // recorded behind the snapshot
    bool snap_side_ = false;            // the snapshot was enqueued on the side stream and the context's stream has not been ordered behind it yet (order)
    void* arena_ = nullptr;             // the journal's batch copies are carved from it (a bump arena, allocated once)
    size_t arena_bytes_, arena_used_ = 0;
    int device_ = 0;
    uint64_t started_ = 0, adopted_ = 0;
};

}  // namespace lv
