// lv_buffers.hpp — the host-side buffers of the map, scan and cloud stores (MapStore, ScanStore, CloudStore: lv_stores.hpp), of the
// context (d_obs, h_states_ring) and of the map tools (QueryStore, BatchStore, VisStore, PaintStore, PlaceStore, SurfaceStore,
// ClusterStore, PlaneStore, OccStore, DistStore, PlanStore, FrontierStore, RayStore, ElevStore, RolloutStore, MclStore, TsdfStore,
// LatticeStore, GraphStore, TrajStore, NdtStore, MclFilterStore): a device buffer and its pinned twin that know their capacity, a stage for packed
// points, a record of four counters, and the grid size of a one-lane-per-item launch.  Host code only; tests/emu/buffers_emu.cpp
// compiles it with g++ against tests/emu/hip/hip_runtime.h and tests/test_buffers_host.py holds it to the rules of DESIGN.md
// "Host-side buffers".
//
// Plain structs, no destructors: a store releases its members in its release() (lv_destroy calls it after hipSetDevice) and may
// then reset itself with *this = XStore().
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "lv_common.hpp"

namespace lv {

// workgroups of `per` lanes for n items, one lane each
inline uint32_t blocks_of(size_t n, uint32_t per = 256) { return (uint32_t)((n + per - 1) / per); }

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
};
template <class T> struct BufElem { static constexpr size_t size = sizeof(T); };
template <> struct BufElem<void> { static constexpr size_t size = 1; };   // (a byte buffer: hipcub scratch, blobs)

// A pointer and the elements it has room for.  Growth frees and allocates anew (the contents are not kept); after a failed
// allocation the buffer is {nullptr, 0} and the next call allocates again.  grow_keep is the one growth that keeps contents.
template <class T, class Mem>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    operator T*() const { return p; }
    T* operator->() const { return p; }
    // room for n elements; grows to exactly n
    int need(size_t n) { return n <= cap ? LV_OK : resize(n); }
    // room for n elements; grows by doubling from `floor` (a buffer whose size follows the caller's batch from call to call)
    int need_pow2(size_t n, size_t floor) {
        if (n <= cap && p) return LV_OK;
        size_t c = cap ? cap : floor;
        while (c < n) c *= 2;
        return resize(c);
    }
    int resize(size_t c) {
        T* old = p;
        p = nullptr;
        cap = 0;
        if (old) LV_HIP(Mem::free(old));
        void* q = nullptr;
        LV_HIP(Mem::alloc(&q, c * BufElem<T>::size));
        p = static_cast<T*>(q);
        cap = c;
        return LV_OK;
    }
    // c elements in a new block whose first `keep` are the old block's [from, from + keep): the new block is allocated first, the
    // copy runs device to device on `stream` and is waited for, then the old block is freed.  whole_device: every stream is
    // waited for before the copy (another stream may still write the old block).  When the allocation, a wait or the copy fails the
    // old block and its capacity stand and LV_EHIP is returned.
    int grow_keep(size_t c, size_t keep, size_t from, hipStream_t stream, bool whole_device) {
        void* q = nullptr;
        LV_HIP(Mem::alloc(&q, c * BufElem<T>::size));
        const int rc = copy_kept(q, keep, from, stream, whole_device);
        if (rc) {
            Mem::free(q);
            return rc;
        }
        T* old = p;
        p = static_cast<T*>(q);
        cap = c;
        if (old) LV_HIP(Mem::free(old));
        return LV_OK;
    }
    int copy_kept(void* q, size_t keep, size_t from, hipStream_t stream, bool whole_device) const {
        if (whole_device) LV_HIP(hipDeviceSynchronize());
        const char* src = reinterpret_cast<const char*>(p) + from * BufElem<T>::size;
        if (p && keep) LV_HIP(hipMemcpyAsync(q, src, keep * BufElem<T>::size, hipMemcpyDeviceToDevice, stream));
        LV_HIP(hipStreamSynchronize(stream));
        return LV_OK;
    }
    void release() {
        if (p) Mem::free(p);
        p = nullptr;
        cap = 0;
    }
};
template <class... B> inline void release_all(B&... b) { (b.release(), ...); }
// room for n elements in every one of the buffers, in the order given; the first failure ends it
template <class... B> inline int need_all(size_t n, B&... b) {
    int rc = LV_OK;
    ((rc = rc ? rc : b.need(n)), ...);
    return rc;
}
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinBuf = Buf<T, PinnedMem>;   // NOTE: the owner synchronises the stream that reads it before need() / release()

// Points from the caller's strided arrays to the device: packed x, y, z in a pinned buffer, one upload into d.
// THE RULE: reserve() synchronises the stream before anything else, so the previous upload has left the pinned buffer before
// it is overwritten or freed; nothing else here waits.  (release() frees without a stream: its callers have synchronised.)
struct PointStage {
    PinBuf<float> h;
    DevBuf<float> d;
    size_t n = 0;   // points appended since reserve()
    // room for n_points; pow2_floor = 0: exact growth, else doubling from that many floats
    int reserve(hipStream_t stream, size_t n_points, size_t pow2_floor = 0) {
        LV_HIP(hipStreamSynchronize(stream));
        n = 0;
        int rc = pow2_floor ? h.need_pow2(3 * n_points, pow2_floor) : h.need(3 * n_points);
        if (!rc) rc = pow2_floor ? d.need_pow2(3 * n_points, pow2_floor) : d.need(3 * n_points);
        return rc;
    }
    // count points, the first three floats of every `stride` bytes, behind those already appended
    void append(const void* pts, size_t stride, size_t count) {
        const char* b = static_cast<const char*>(pts);
        for (size_t i = 0; i < count; ++i, ++n) std::memcpy(h.p + 3 * n, b + i * stride, 3 * sizeof(float));
    }
    int upload(hipStream_t stream) {
        if (n) LV_HIP(hipMemcpyAsync(d.p, h.p, 3 * n * sizeof(float), hipMemcpyHostToDevice, stream));
        return LV_OK;
    }
    void release() {
        h.release();
        d.release();
        n = 0;
    }
};

// The four 64-bit counters a call accumulates on the device and hands back (lv_occ_integrate, lv_occ_distance_build,
// lv_occ_plan_build).  Allocated by the first need() / zero().
struct Counters4 {
    DevBuf<unsigned long long> d;
    PinBuf<unsigned long long> h;
    int need() {
        const int rc = d.need(4);
        return rc ? rc : h.need(4);
    }
    // zeros travel from the pinned words, which are free: the read() before this has waited for the stream
    int zero(hipStream_t stream) {
        const int rc = need();
        if (rc) return rc;
        std::memset(h.p, 0, 4 * sizeof(unsigned long long));
        LV_HIP(hipMemcpyAsync(d.p, h.p, 4 * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
        return LV_OK;
    }
    // waits for the stream; out may be NULL
    int read(hipStream_t stream, uint64_t out[4]) {
        LV_HIP(hipMemcpyAsync(h.p, d.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
        if (out)
            for (int i = 0; i < 4; ++i) out[i] = (uint64_t)h.p[i];
        return LV_OK;
    }
    void release() {
        d.release();
        h.release();
    }
};

}  // namespace lv
