// lv_exchange.hpp — the multi-rank exchange (row e): how the per-pass partials of N ranks reach every rank, over RCCL (lv_comm.hip),
// the caller's host gather or peer-mapped buffers (lv_peer.hip).  lv_ctx holds one; the entry points hand it the context's stream.
// Rules (tests/test_exchange_host.py checks them on the host, fake transports): one transport at a time (a host gather may be
// replaced or removed, a peer export counts before its init); once the peer set is mapped, d_gather aliases its buffers and
// peer_close alone frees them; the gather buffers grow, zeroed, and never shrink; a peer set's capacity is fixed by its export.
#pragma once
#include <cstddef>
#include <cstring>

#include "lv_common.hpp"

namespace lv {

// lv_comm.hip — RCCL bound at run time
struct UniqueId128 { char internal[128]; };  // ncclUniqueId
int comm_unique_id(const char* library, void* id128);
int comm_init(const char* library, const void* id128, int rank, int world, void** comm_out);
int comm_destroy(void* comm);
int comm_allreduce_record(void* comm, double* record, hipStream_t stream);
bool comm_has_allgather();
int comm_allgather_inplace(void* comm, double* buf, size_t count_per_rank, int rank, hipStream_t stream);
// lv_peer.hip — the same exchange by peer-mapped memory (HIP IPC), no collective library
constexpr int LV_PEER_MAX = 8;
struct PeerSet {
    void* local_alloc = nullptr;                 // [gather buffer 0 | gather buffer 1]: read by the peers only after the pass kernel ended
    void* flag_alloc = nullptr;                  // [flag word]: its own fine-grained allocation, polled across devices in mid-kernel
    bool buf_fine = false;                       // the gather slots are in fine-grained memory (false: plain allocation)
    bool flag_fine = false;                      // (false: the runtime refused a fine-grained IPC allocation; the flag lives in a plain one)
    double* buf[2] = {nullptr, nullptr};
    unsigned long long* flag = nullptr;
    uint32_t* h_status = nullptr;                // pinned, host-mapped: set by a pull that gave up (or met a poisoned flag); sticky
    uint32_t* d_status = nullptr;                // ... its device address
    void* mapped[LV_PEER_MAX] = {};              // the other ranks' gather allocations as mapped here
    void* mapped_flag[LV_PEER_MAX] = {};         // ... and their flag allocations
    double* peer_buf[2][LV_PEER_MAX] = {};
    unsigned long long* peer_flag[LV_PEER_MAX] = {};
    size_t cap = 0;                              // doubles per gather buffer
    int rank = 0, world = 1;
    unsigned long long seq = 0;                  // launches published so far (every rank counts alike)
    long long timeout_ticks = 0;                 // give-up time of a pull's wait, 100 MHz ticks (LV_PEER_TIMEOUT_MS, default 2000 ms)
    bool active = false;
};
constexpr int LV_PEER_BLOB = 128;               // two HIP IPC handles: gather buffers, flag word (= LV_PEER_HANDLE_BYTES of the ABI)
int peer_export(PeerSet& P, size_t cap_doubles, void* handle_blob);
int peer_init(PeerSet& P, int rank, int world, const void* handles);
int peer_gather(PeerSet& P, int parity, size_t slot_doubles, hipStream_t stream);
// a pull of this context gave up on a peer or met a poisoned flag (a plain read of the host-mapped word: for completed launches)
bool peer_failed(const PeerSet& P);
void peer_close(PeerSet& P);

struct RankExchange {
    // PeerExported: lv_comm_peer_export ran, lv_comm_peer_init has not (one rank still); PeerMapped: d_gather[0/1] are peer.buf[0/1]
    enum class Transport { None, Rccl, HostGather, PeerExported, PeerMapped };
    Transport transport = Transport::None;
    void* comm = nullptr;          // Rccl
    int rank = 0, world = 1;
    double* d_gather[2] = {nullptr, nullptr};   // the one-launch form: each rank's workgroup partials in its slot, by launch parity
    size_t gather_cap = 0;         // doubles per buffer
    size_t shard_max = 0;          // largest shard of the CURRENT scan over the ranks (lv_comm_set_shard_max); 0: unknown
    bool fused = true;             // lv_set_comm_fused / LV_COMM_FUSED=0: always the three-kernel pass + all-reduce with a communicator
    PeerSet peer;                  // PeerExported, PeerMapped
    lv_gather_fn gather_cb = nullptr;   // HostGather: the caller's all-gather through h_gather
    void* gather_user = nullptr;
    double* h_gather = nullptr;    // pinned staging, world x slot doubles (kept when the host gather is removed)
    size_t h_gather_cap = 0;
    bool multi_rank() const { return transport == Transport::Rccl || gather_only(); }
    bool gather_only() const { return transport == Transport::HostGather || transport == Transport::PeerMapped; }   // (no all-reduce)
    bool peer_set() const { return transport == Transport::PeerExported || transport == Transport::PeerMapped; }
    int busy(const char* call) const {
        return set_error("%s: %s is in place", call, transport == Transport::Rccl ? "a library communicator (lv_comm_init)"
                         : transport == Transport::HostGather ? "a host gather (lv_comm_set_host_gather)" : "a peer-mapped gather (lv_comm_peer_export)"), LV_ESTATE;
    }
    int init_rccl(const char* library, const void* id128, int r, int w) {
        if (transport != Transport::None) return busy("lv_comm_init");
        if (int rc = comm_init(library, id128, r, w, &comm)) return rc;   // collective: every rank calls it (comm: set on success only)
        transport = Transport::Rccl, rank = r, world = w;
        return LV_OK;
    }
    int set_host_gather(hipStream_t s, int r, int w, lv_gather_fn fn, void* user) {   // fn == nullptr: removed (rank 0 of 1)
        if (transport != Transport::None && transport != Transport::HostGather) return busy("lv_comm_set_host_gather");
        if (fn && (w < 1 || r < 0 || r >= w)) return set_error("lv_comm_set_host_gather: bad arguments (rank %d, world %d)", r, w), LV_EINVAL;
        LV_HIP(hipStreamSynchronize(s));
        transport = fn ? Transport::HostGather : Transport::None, gather_cb = fn, gather_user = fn ? user : nullptr;
        rank = fn ? r : 0, world = fn ? w : 1, shard_max = 0;
        return LV_OK;
    }
    // sized once for the largest case (every CU a workgroup, 96-double partials, LV_PEER_MAX ranks): the other ranks map this
    // allocation, so it never moves.  A second export is refused by lv::peer_export, a failed one may leave its allocation behind
    int peer_export(hipStream_t s, int max_wg, void* blob) {
        if (transport == Transport::Rccl || transport == Transport::HostGather) return busy("lv_comm_peer_export");
        LV_HIP(hipStreamSynchronize(s));
        const int rc = lv::peer_export(peer, (size_t)(max_wg + 8) * 96u * (size_t)LV_PEER_MAX, blob);
        if (transport == Transport::None && peer.local_alloc) transport = Transport::PeerExported;
        return rc;
    }
    int peer_init(hipStream_t s, int r, int w, const void* handles) {
        if (!peer_set()) return set_error("lv_comm_peer_export first"), LV_ESTATE;
        if (transport == Transport::PeerMapped) return set_error("the peer exchange of this context is already set up (lv_comm_destroy first)"), LV_ESTATE;
        if (int rc = lv::peer_init(peer, r, w, handles)) return rc;
        transport = Transport::PeerMapped;
        LV_HIP(hipStreamSynchronize(s));
        hipFree(d_gather[0]); hipFree(d_gather[1]);   // (this rank's own, replaced by the peer set's)
        d_gather[0] = peer.buf[0], d_gather[1] = peer.buf[1], gather_cap = peer.cap, rank = r, world = w, shard_max = 0;
        return LV_OK;
    }
    void close_peer() {   // (the gather buffers it lends go with it)
        if (transport == Transport::PeerMapped) d_gather[0] = d_gather[1] = nullptr, gather_cap = 0;
        peer_close(peer);
    }
    int destroy(hipStream_t s) {   // lv_comm_destroy: the peer set or the communicator; a host gather stays
        if (!peer_set() && transport != Transport::Rccl) return LV_OK;
        LV_HIP(hipStreamSynchronize(s));
        const int rc = peer_set() ? LV_OK : comm_destroy(comm);
        if (peer_set()) close_peer(), shard_max = 0;
        transport = Transport::None, comm = nullptr, rank = 0, world = 1;
        return rc;
    }
    // lv_destroy: the communicator first (synchronised), before the context's other buffers go; release() with them
    void release_comm(hipStream_t s) { if (transport == Transport::Rccl) hipStreamSynchronize(s), comm_destroy(comm), comm = nullptr, transport = Transport::None; }
    void release() {
        if (h_gather) hipHostFree(h_gather);
        if (peer_set()) close_peer();
        hipFree(d_gather[0]); hipFree(d_gather[1]);
    }
    // lv_comm_set_shard_max: `slot` doubles per rank.  The host staging is sized for a host gather only; a mapped peer set cannot grow
    int reserve(hipStream_t s, size_t slot) {
        const size_t need = slot * (size_t)world;
        if (transport == Transport::HostGather && need > h_gather_cap) {
            LV_HIP(hipStreamSynchronize(s));
            if (h_gather) hipHostFree(h_gather), h_gather = nullptr, h_gather_cap = 0;
            LV_HIP(hipHostMalloc((void**)&h_gather, need * sizeof(double), hipHostMallocDefault));
            std::memset(h_gather, 0, need * sizeof(double)), h_gather_cap = need;
        }
        if (need <= gather_cap) return LV_OK;
        if (transport == Transport::PeerMapped)
            return set_error("peer-mapped gather: %zu doubles exceed the exported buffers (%zu)", need, gather_cap), LV_EINVAL;
        LV_HIP(hipStreamSynchronize(s));
        for (double*& d : d_gather) hipFree(d), d = nullptr;
        gather_cap = 0;
        for (double*& d : d_gather) { LV_HIP(hipMalloc(&d, need * sizeof(double))); LV_HIP(hipMemset(d, 0, need * sizeof(double))); }
        return gather_cap = need, LV_OK;
    }
    // the one-launch form across the ranks: the largest shard told (this rank's scan within it), an all-gather to carry the
    // partials (librccl's is optional), the gather buffers in place and large enough
    bool fused_ready(uint32_t scan_n) const {
        return fused && shard_max != 0 && scan_n <= shard_max && (transport != Transport::Rccl || comm_has_allgather()) && d_gather[0];
    }
    bool fits(size_t slot) const { return slot * (size_t)world <= gather_cap; }
    double* part_out(int parity, size_t slot) const { return d_gather[parity] + (size_t)rank * slot; }
    int nrec(int nwg) const { return multi_rank() ? nwg * world : nwg; }
    int exchange(hipStream_t s, int launch, size_t slot) {   // after launch `launch`: every rank's slot of buffer launch & 1, on every rank
        const int p = launch & 1;
        if (transport == Transport::PeerMapped) return peer_gather(peer, p, slot, s);   // publish this rank's slot, pull the others'
        if (transport == Transport::Rccl) return comm_allgather_inplace(comm, d_gather[p], slot, rank, s);
        // the caller's: this rank's slot to pinned memory, the callback fills in the others' (blocking), all of it back to the device
        LV_HIP(hipMemcpyAsync(h_gather + (size_t)rank * slot, part_out(p, slot), slot * sizeof(double), hipMemcpyDeviceToHost, s));
        LV_HIP(hipStreamSynchronize(s));
        if (gather_cb(gather_user, h_gather, slot * sizeof(double), rank, world) != 0)
            return set_error("host gather callback failed (launch %d)", launch), LV_ESTATE;
        LV_HIP(hipMemcpyAsync(d_gather[p], h_gather, slot * sizeof(double) * (size_t)world, hipMemcpyHostToDevice, s));
        return LV_OK;
    }
    int allreduce(hipStream_t s, double* record) { return comm_allreduce_record(comm, record, s); }   // (the three-kernel pass, in place)
    bool failed() const { return transport == Transport::PeerMapped && peer_failed(peer); }
    int refuse_unfused() const {   // lv_update / lv_correct on a gather-only transport, of a scan that does not take the one-launch form
        return set_error("host-staged / peer-mapped gather: this scan does not take the one-launch-per-pass form (largest shard told? size? options?)"), LV_ESTATE;
    }
};

}  // namespace lv
