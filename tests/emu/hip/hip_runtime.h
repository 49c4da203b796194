// tests/emu/hip/hip_runtime.h — a HOST stand-in for <hip/hip_runtime.h>, TEST INFRASTRUCTURE ONLY.
//
// It lets tests/emu/mapinc_emu.cpp compile the one-thread-per-item kernels of limo-velo_amd/csrc/lv_mapinc.hpp with
// g++ and run them as plain loops (one "thread" after another, optionally in reverse or shuffled order), so the
// bookkeeping of the incremental map can be checked against the oracle in the GPU-less container; and it lets
// tests/emu/rebuild_emu.cpp, tests/emu/filter_emu.cpp and tests/emu/update_emu.cpp compile limo-velo_amd/csrc/lv_rebuild.hpp,
// lv_filter.hpp and lv_update.hpp, and tests/emu/stores_emu.cpp lv_stores.hpp, against the fake host API at the end of this file.
// Nothing here is linked into, loaded by or reachable from the product library.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)

struct float4 { float x, y, z, w; };
struct uint4 { unsigned int x, y, z, w; };
struct uint2 { unsigned int x, y; };
struct emu_dim3 { unsigned int x = 1, y = 1, z = 1; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

extern emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

static inline unsigned int __float_as_uint(float f) { unsigned int u; std::memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(unsigned int u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }

#define __HIP_MEMORY_SCOPE_SYSTEM 5
template <typename T, typename V> static inline void __hip_atomic_store(T* p, V v, int, int) { *p = (T)v; }   // (lv_note.hpp's note_post)
template <typename T> static inline T atomicAdd(T* p, T v) { T o = *p; *p = (T)(o + v); return o; }
template <typename T> static inline T atomicExch(T* p, T v) { T o = *p; *p = v; return o; }
template <typename T> static inline T atomicCAS(T* p, T cmp, T v) { T o = *p; if (o == cmp) *p = v; return o; }
template <typename T> static inline T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }
template <typename T> static inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }

using std::abs;
using std::max;
using std::min;

// ---- host API: streams, events and allocations.  Every call runs synchronously (a copy is done when the call returns) and is
// logged as (call, stream, event) so a test can assert the order of its stream work; allocations, events and streams are
// counted so leaks show.  `fail` (set by a test) makes the call it returns true for fail with hipErrorUnknown.
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3, hipMemcpyDefault = 4 };
typedef struct emu_stream* hipStream_t;
typedef struct emu_event* hipEvent_t;
#define hipStreamNonBlocking 0x01
#define hipEventDisableTiming 0x02
#define hipHostMallocDefault 0x0
#define hipHostMallocMapped 0x2

namespace emu_hip {
struct Call {
    std::string call;
    hipStream_t stream;
    hipEvent_t event;
};
struct State {
    std::mutex mu;
    std::vector<Call> log;
    std::function<bool(const char* call)> fail;
    uintptr_t next_handle = 0x1000;
    std::atomic<long> mallocs{0}, frees{0}, events_created{0}, events_destroyed{0}, streams_created{0}, streams_destroyed{0};
    std::atomic<size_t> last_alloc_bytes{0};   // of the last successful hipMalloc / hipHostMalloc
    float elapsed_ms = 0.f;                    // what hipEventElapsedTime answers (set by a test)
};
inline State& state() { static State s; return s; }
inline hipError_t call(const char* name, hipStream_t s = nullptr, hipEvent_t e = nullptr) {
    State& st = state();
    std::lock_guard<std::mutex> g(st.mu);
    if (st.fail && st.fail(name)) return hipErrorUnknown;
    st.log.push_back({name, s, e});
    return hipSuccess;
}
template <typename H> H new_handle() {
    State& st = state();
    std::lock_guard<std::mutex> g(st.mu);
    return reinterpret_cast<H>(st.next_handle += 16);
}
}  // namespace emu_hip

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess" : "emulated HIP failure"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipSetDevice(int) { return emu_hip::call("hipSetDevice"); }
inline hipError_t hipDeviceSynchronize() { return emu_hip::call("hipDeviceSynchronize"); }
inline hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return emu_hip::call("hipDeviceGetStreamPriorityRange"); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) {
    hipError_t e = emu_hip::call("hipStreamCreateWithPriority");
    if (e == hipSuccess) { *s = emu_hip::new_handle<hipStream_t>(); ++emu_hip::state().streams_created; }
    return e;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    hipError_t e = emu_hip::call("hipStreamCreateWithFlags");
    if (e == hipSuccess) { *s = emu_hip::new_handle<hipStream_t>(); ++emu_hip::state().streams_created; }
    return e;
}
inline hipError_t hipStreamDestroy(hipStream_t s) { ++emu_hip::state().streams_destroyed; return emu_hip::call("hipStreamDestroy", s); }
inline hipError_t hipStreamSynchronize(hipStream_t s) { return emu_hip::call("hipStreamSynchronize", s); }
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { return emu_hip::call("hipStreamWaitEvent", s, e); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
    hipError_t e = emu_hip::call("hipEventCreateWithFlags");
    if (e == hipSuccess) { *ev = emu_hip::new_handle<hipEvent_t>(); ++emu_hip::state().events_created; }
    return e;
}
inline hipError_t hipEventCreate(hipEvent_t* ev) {
    hipError_t e = emu_hip::call("hipEventCreate");
    if (e == hipSuccess) { *ev = emu_hip::new_handle<hipEvent_t>(); ++emu_hip::state().events_created; }
    return e;
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    hipError_t e = emu_hip::call("hipEventElapsedTime", nullptr, b);
    if (e == hipSuccess) *ms = emu_hip::state().elapsed_ms;
    return e;
}
inline hipError_t hipEventDestroy(hipEvent_t ev) { ++emu_hip::state().events_destroyed; return emu_hip::call("hipEventDestroy", nullptr, ev); }
inline hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s) { return emu_hip::call("hipEventRecord", s, ev); }
inline hipError_t hipEventSynchronize(hipEvent_t ev) { return emu_hip::call("hipEventSynchronize", nullptr, ev); }
inline hipError_t hipMalloc(void** p, size_t bytes) {
    hipError_t e = emu_hip::call("hipMalloc");
    if (e == hipSuccess) { *p = std::malloc(bytes ? bytes : 1); ++emu_hip::state().mallocs; emu_hip::state().last_alloc_bytes = bytes; }
    return e;
}
template <typename T> inline hipError_t hipMalloc(T** p, size_t bytes) { return hipMalloc(reinterpret_cast<void**>(p), bytes); }
inline hipError_t hipFree(void* p) {
    if (p) { std::free(p); ++emu_hip::state().frees; }
    return emu_hip::call("hipFree");
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t s) {
    hipError_t e = emu_hip::call("hipMemcpyAsync", s);
    if (e == hipSuccess && bytes) std::memcpy(dst, src, bytes);
    return e;
}
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    hipError_t e = emu_hip::call("hipMemcpy");
    if (e == hipSuccess && bytes) std::memcpy(dst, src, bytes);
    return e;
}
inline hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t s) {
    hipError_t e = emu_hip::call("hipMemsetAsync", s);
    if (e == hipSuccess && bytes) std::memset(dst, v, bytes);
    return e;
}
inline hipError_t hipMemset(void* dst, int v, size_t bytes) {
    hipError_t e = emu_hip::call("hipMemset");
    if (e == hipSuccess && bytes) std::memset(dst, v, bytes);
    return e;
}
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    hipError_t e = emu_hip::call("hipHostMalloc");
    if (e == hipSuccess) { *p = std::malloc(bytes ? bytes : 1); ++emu_hip::state().mallocs; emu_hip::state().last_alloc_bytes = bytes; }
    return e;
}
inline hipError_t hipHostFree(void* p) {
    if (p) { std::free(p); ++emu_hip::state().frees; }
    return emu_hip::call("hipHostFree");
}
inline hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) { *dev = host; return emu_hip::call("hipHostGetDevicePointer"); }
