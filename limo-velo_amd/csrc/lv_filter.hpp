// lv_filter.hpp — the resident filter (row f-3): where x, P live between lv_filter_set, lv_predict, lv_correct and lv_filter_get,
// and the queue of predictions waiting to launch.  lv_ctx holds one; the update driver (lv_update.hpp) and the entry points hand it the context's stream, kf and mailbox.
// The 100 Hz cycle set -> correct -> get makes no HIP call on the filter's behalf: the prior rides in the correct's first launch,
// the posterior stays in kf, the get reads the mailbox.  Rules (tests/test_filter_host.py checks them on the host, fake launches):
// - h is not overwritten while an upload out of it may be in flight (set waits on ev_up);
// - a queued prediction reads kf if the filter was in kf when it was queued, d otherwise; the queue is flushed before anything
//   else reads, replaces or overwrites the filter or kf;
// - kf is copied to d (materialise) before an update by value, lv_iterate or lv_calculate_H makes kf its working copy;
// - an aiding observation (lv_observe) works on d: queue flushed, h uploaded, kf materialised first; afterwards the filter is d's
//   and the mailbox no longer holds it (tests/test_observe_host.py).
#pragma once
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstring>

#include "lv_common.hpp"
#include "lv_device.hpp"
#include "lv_observe.hpp"

namespace lv {

// The pass that finishes an update stores the sequence number after all results (system-scope stores): poll it for a bounded
// time (an update takes ~0.2 ms) instead of paying the stream-synchronise wake-up.  false: the caller synchronises the stream.
inline bool mailbox_wait(const KfHostIO* io, int seq, bool enabled, long* resyncs) {
    if (!enabled) return false;
    volatile const unsigned long long* sc = &io->seqcheck;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long word = 0;
    bool seen = false;
    for (int it = 0;; ++it) {
        word = *sc;
        if ((uint32_t)word == (uint32_t)seq) { seen = true; break; }
        if ((it & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!seen) return false;
    // the results were stored before the word, but only the checksum proves that they have all ARRIVED
    const uint32_t want = (uint32_t)(word >> 32);
    uint32_t chk = 0;
    for (int i = 0; i < NS * NS; ++i) chk ^= mailbox_mix(io->P_post[i], (uint32_t)i);
    for (int i = 0; i < NX; ++i) chk ^= mailbox_mix(io->x[i], 1000u + (uint32_t)i);
    chk ^= mailbox_mix((double)io->passes, 2000u);
    if (chk == MAILBOX_UNCHECKED) chk = 0u;
    // (MAILBOX_UNCHECKED: the update ended on a pass without matches — a legitimate path that carries no
    // checksum: synchronise the stream without counting it)
    if (want == MAILBOX_UNCHECKED) return false;
    if (chk != want) ++*resyncs;
    return chk == want;
}

struct ResidentFilter {
    enum class Where {
        Unset,    // never set, or dropped (a failed lv_correct, a failed peer exchange)
        Host,     // h, as lv_filter_set left it (d is stale)
        Device,   // d, followed by the queued predictions
        Kf,       // the posterior of the last lv_correct: kf->x / kf->P_post, and the mailbox
        Copied,   // that posterior copied to d (materialise); the mailbox still holds it
    };
    enum class Source { None, Filter, ByValue };   // who produced the latest state: lv_map_add_scan transforms the scan with it
    struct Prior { const double* host; const FilterDev* dev; int dev_in_kf; };   // launch_kf_begin's x_host, filt, filt_in_kf

    Where where = Where::Unset;
    Source latest = Source::None;
    FilterDev *d = nullptr, *h = nullptr;   // h: pinned
    hipEvent_t ev_up = nullptr;    // recorded behind the last upload out of h
    bool up_pending = false;
    double Q[144] = {};            // the queue: up to PREDICT_BATCH steps {dt, acc[3], gyro[3]} with one Q
    double steps[PREDICT_BATCH][7] = {};
    int n = 0;
    bool src_kf = false;           // the first queued step reads kf
    bool batch_predict = true;     // lv_set_option "batch_predict" / LV_BATCH_PREDICT=0: one launch per lv_predict
    bool mail_filter = true;       // lv_set_option "mail_filter" / LV_MAIL_FILTER=0: lv_filter_get always copies

    int alloc() {
        LV_HIP(hipMalloc(&d, sizeof(FilterDev)));
        LV_HIP(hipMemset(d, 0, sizeof(FilterDev)));
        LV_HIP(hipHostMalloc((void**)&h, sizeof(FilterDev), hipHostMallocDefault));
        return LV_OK;
    }
    void release() { if (ev_up) hipEventDestroy(ev_up); if (h) hipHostFree(h); hipFree(d); }
    int need(const char* call) const { return where != Where::Unset ? LV_OK : (set_error("%s before lv_filter_set", call), LV_ESTATE); }
    bool in_mailbox() const { return where == Where::Kf || where == Where::Copied; }
    // Nothing goes to the device here: the filter waits in h until something needs it there (lv_correct does not: prior)
    int set(const lv_state* x, const double* P) {
        n = 0;   // (queued predictions of a filter that is being replaced)
        if (up_pending) { LV_HIP(hipEventSynchronize(ev_up)); up_pending = false; }
        std::memcpy(h->x, x, sizeof(double) * NX);
        std::memcpy(h->P, P, sizeof(double) * NS * NS);
        where = Where::Host, latest = Source::Filter;
        return LV_OK;
    }
    int predict(hipStream_t s, const KfDev* kf, double dt, const double* Qn, const double* acc, const double* gyro) {
        if (int r = need("lv_predict")) return r;
        latest = Source::Filter;
        if (n > 0 && (n >= PREDICT_BATCH || std::memcmp(Q, Qn, sizeof(Q)) != 0))
            if (int r = flush(s, kf)) return r;
        if (n == 0) { std::memcpy(Q, Qn, sizeof(Q)); src_kf = where == Where::Kf; }
        if (in_mailbox()) where = Where::Device;
        double* st = steps[n++];
        st[0] = dt;
        for (int i = 0; i < 3; ++i) { st[1 + i] = acc[i]; st[4 + i] = gyro[i]; }
        return batch_predict ? LV_OK : flush(s, kf);
    }
    int flush(hipStream_t s, const KfDev* kf) {
        if (n == 0) return LV_OK;
        if (int r = upload(s)) return r;
        const int k = n;
        const KfDev* src = src_kf ? kf : nullptr;
        n = 0, src_kf = false;
        return launch_predict(s, d, src, Q, k, steps);
    }
    int upload(hipStream_t s) {
        if (where != Where::Host) return LV_OK;
        where = Where::Device;
        LV_HIP(hipMemcpyAsync(d, h, sizeof(FilterDev), hipMemcpyHostToDevice, s));
        if (!ev_up) LV_HIP(hipEventCreateWithFlags(&ev_up, hipEventDisableTiming));
        LV_HIP(hipEventRecord(ev_up, s));
        up_pending = true;
        return LV_OK;
    }
    int materialise(hipStream_t s, const KfDev* kf) {
        if (where != Where::Kf) return LV_OK;
        where = Where::Copied;
        return launch_kf_to_filter(s, kf, d);
    }
    // lv_correct's prior: the copy lv_filter_set left rides in the first launch's arguments (x followed by P: no upload, no begin
    // kernel; the filter counts as on the device from here), otherwise kf_begin_kernel installs d or finds the filter in kf
    Prior prior() {
        static_assert(offsetof(FilterDev, P) == sizeof(double) * NX, "x followed by P");
        if (where != Where::Host) return {nullptr, d, where == Where::Kf};
        where = Where::Device;
        return {h->x, nullptr, 0};
    }
    // before an update's begin: kf becomes its working copy, so the filter leaves it unless the update is a correct starting from it
    int begin_update(hipStream_t s, const KfDev* kf, bool from_filter) {
        if (int r = flush(s, kf)) return r;
        if (int r = upload(s)) return r;
        if (int r = from_filter ? LV_OK : materialise(s, kf)) return r;
        if (where == Where::Copied) where = Where::Device;   // (the mailbox is about to receive this update's results)
        return LV_OK;
    }
    // lv_observe: aiding observations applied to d in one launch, behind the queued predictions (calls keep their order in time).
    // The posterior of a correct leaves kf first; afterwards the filter is d's, and the mailbox no longer holds it.
    int observe(hipStream_t s, const KfDev* kf, const lv_observation* obs, size_t n_obs, lv_observe_result* d_results) {
        if (int r = need("lv_observe")) return r;
        if (int r = observations_ok(obs, n_obs)) return r;   // (before anything is enqueued)
        if (int r = flush(s, kf)) return r;
        if (int r = upload(s)) return r;
        if (int r = materialise(s, kf)) return r;
        where = Where::Device, latest = Source::Filter;
        return launch_observe(s, d, obs, (int)n_obs, d_results);
    }
    void correct_done() { where = Where::Kf; }
    // a failed correct (kf may hold a half-iterated state, d an older one) or peer exchange: the caller re-seeds the filter
    void drop() { where = Where::Unset; n = 0; }
    // lv_filter_get.  > 0: the mailbox's fallback word, which carries KF_FAULT_BIT (x, P untouched)
    int get(hipStream_t s, const KfDev* kf, const KfHostIO* io, int seq, bool spin, long* resyncs, lv_state* x, double* P) {
        if (int r = need("lv_filter_get")) return r;
        if (int r = flush(s, kf)) return r;
        const double *sx = h->x, *sP = h->P;   // (Host: where lv_filter_set put it)
        if (in_mailbox() && mail_filter) {
            // the posterior of the lv_correct just enqueued, which its finishing pass stores into the mailbox as well: a poll instead
            // of a copy + stream synchronise (~30 us of wake-up, once per 100 Hz cycle: src/main.cpp:96-102 reads it after every correct)
            if (!mailbox_wait(io, seq, spin, resyncs)) LV_HIP(hipStreamSynchronize(s));
            if ((unsigned)io->fallback_queries & KF_FAULT_BIT) return io->fallback_queries;
            sx = io->x, sP = io->P_post;
        } else if (where != Where::Host) {
            if (int r = materialise(s, kf)) return r;
            LV_HIP(hipMemcpyAsync(h, d, sizeof(FilterDev), hipMemcpyDeviceToHost, s));
            LV_HIP(hipStreamSynchronize(s));
        }
        if (x) std::memcpy(x, sx, sizeof(double) * NX);
        if (P) std::memcpy(P, sP, sizeof(double) * NS * NS);
        return LV_OK;
    }
    // lv_map_add_scan's state (after upload): the latest one (main.cpp:92,102: the state the update just produced, or before the
    // first map exists the propagated state the caller handed to lv_update)
    const double* scan_x(const KfDev* kf) const { return latest == Source::ByValue || where == Where::Unset || where == Where::Kf ? kf->x : d->x; }
};

}  // namespace lv
