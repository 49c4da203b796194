// tests/emu/buffers_emu.cpp — limo-velo_amd/csrc/lv_buffers.hpp run on the host (TEST INFRASTRUCTURE ONLY; g++ through
// tests/emu/hip/hip_runtime.h).  argv[1] names a case; the case prints one "name value..." line per fact and
// tests/test_buffers_host.py asserts the values.  The stand-in's call log, its mallocs / frees counters and its fail hook are
// the instruments.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "lv_buffers.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace lv {
static std::string g_error;
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace lv

using namespace lv;

static emu_hip::State& st() { return emu_hip::state(); }
static long count(const char* name, size_t from = 0) {
    long n = 0;
    for (size_t i = from; i < st().log.size(); ++i) n += st().log[i].call == name;
    return n;
}
// the log from `from` on, as "call call ..." (a call on stream s as "call@s", s the stream's number)
static void print_log(const char* label, size_t from, hipStream_t s1) {
    printf("%s", label);
    for (size_t i = from; i < st().log.size(); ++i) printf(" %s%s", st().log[i].call.c_str(), s1 && st().log[i].stream == s1 ? "@1" : "");
    printf("\n");
}

static int exact() {
    DevBuf<double> b{};
    int rc = b.need(100);
    printf("first %d %ld %zu %zu\n", rc, count("hipMalloc"), b.cap, (size_t)st().last_alloc_bytes);
    for (size_t i = 0; i < 100; ++i) b[i] = (double)i;   // (the sanitizer watches the end)
    rc = b.need(100);
    printf("same %d %ld %ld\n", rc, count("hipMalloc"), count("hipFree"));
    rc = b.need(7);
    printf("smaller %d %ld %ld %zu\n", rc, count("hipMalloc"), count("hipFree"), b.cap);
    const size_t mark = st().log.size();
    rc = b.need(101);
    print_log("larger", mark, nullptr);
    printf("larger_bytes %d %zu %zu\n", rc, b.cap, (size_t)st().last_alloc_bytes);
    b.release();
    printf("released %d %zu %ld %ld\n", b.p == nullptr, b.cap, (long)st().mallocs, (long)st().frees);
    DevBuf<void> v{};
    rc = v.need(37);
    printf("bytes %d %zu %zu\n", rc, v.cap, (size_t)st().last_alloc_bytes);
    rc = v.need(0);
    v.release();
    DevBuf<int> z{};
    rc = z.need(0);
    printf("zero %d %d %ld %ld\n", rc, z.p == nullptr, (long)st().mallocs, (long)st().frees);
    return 0;
}

static int doubling() {
    DevBuf<float> b{};
    const size_t ns[3] = {1, 1024, 1025};
    for (size_t n : ns) {
        const int rc = b.need_pow2(n, 1024);
        printf("cap %d %zu %zu %ld\n", rc, b.cap, (size_t)st().last_alloc_bytes, count("hipMalloc"));
    }
    int rc = b.need_pow2(5000, 1024);
    printf("cap %d %zu %zu %ld\n", rc, b.cap, (size_t)st().last_alloc_bytes, count("hipMalloc"));
    b.release();
    DevBuf<void> v{};
    rc = v.need_pow2(4097, 4096);
    printf("bytes %d %zu %zu\n", rc, v.cap, (size_t)st().last_alloc_bytes);
    v.release();
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    return 0;
}

static int failure() {
    DevBuf<int> d{};
    PinBuf<int> h{};
    int rc = d.need(8);
    rc = rc ? rc : h.need(8);
    printf("before %d %zu %zu\n", rc, d.cap, h.cap);
    st().fail = [](const char* c) { return std::string(c) == "hipMalloc" || std::string(c) == "hipHostMalloc"; };
    rc = d.need(16);
    printf("dev_failed %d %d %zu %d\n", rc == LV_EHIP, d.p == nullptr, d.cap, g_error.find("emulated HIP failure") != std::string::npos);
    rc = h.need_pow2(16, 4);
    printf("pin_failed %d %d %zu\n", rc == LV_EHIP, h.p == nullptr, h.cap);
    st().fail = nullptr;
    const long m0 = count("hipMalloc"), p0 = count("hipHostMalloc");
    rc = d.need(4);   // (smaller than the buffer lost: it still allocates)
    printf("dev_again %d %d %zu %ld\n", rc, d.p != nullptr, d.cap, count("hipMalloc") - m0);
    rc = h.need(4);
    printf("pin_again %d %d %zu %ld\n", rc, h.p != nullptr, h.cap, count("hipHostMalloc") - p0);
    d.release();
    h.release();
    d.release();   // (a second release is nothing)
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    return 0;
}

// grow_keep: the one growth that keeps contents
static int keep() {
    hipStream_t s1 = nullptr;
    if (hipStreamCreateWithFlags(&s1, hipStreamNonBlocking) != hipSuccess) return 2;
    DevBuf<int> b{};
    size_t mark = st().log.size();
    int rc = b.grow_keep(8, 0, 0, s1, false);   // from empty: nothing to copy, nothing to free
    print_log("empty", mark, s1);
    printf("from_empty %d %zu %d\n", rc, b.cap, b.p != nullptr);
    for (int i = 0; i < 8; ++i) b[i] = 100 + i;
    mark = st().log.size();
    rc = b.grow_keep(16, 5, 2, s1, false);      // elements [2, 7) to the front, on the stream
    print_log("stream", mark, s1);
    printf("kept %d %zu %zu", rc, b.cap, (size_t)st().last_alloc_bytes);
    for (int i = 0; i < 5; ++i) printf(" %d", b[i]);
    printf("\n");
    mark = st().log.size();
    rc = b.grow_keep(32, 5, 0, nullptr, true);  // the whole device waited for before the copy
    print_log("device", mark, s1);
    printf("kept_device %d %zu %d %d\n", rc, b.cap, b[0], b[4]);
    const int* old = b.p;
    mark = st().log.size();
    rc = b.grow_keep(64, 0, 0, s1, false);      // keep == 0: a new block, no copy, the wait stays
    print_log("none", mark, s1);
    printf("kept_none %d %zu %d\n", rc, b.cap, b.p != old);
    for (int i = 0; i < 4; ++i) b[i] = 7 * i;
    // a failure at each of its calls but the last leaves the old block usable and frees the new one
    const char* calls[3] = {"hipMalloc", "hipMemcpyAsync", "hipStreamSynchronize"};
    for (const char* c : calls) {
        const long m0 = (long)st().mallocs, f0 = (long)st().frees;
        old = b.p;
        st().fail = [c](const char* name) { return std::string(name) == c; };
        rc = b.grow_keep(128, 4, 0, s1, false);
        st().fail = nullptr;
        printf("failed %s %d %d %zu %d %ld\n", c, rc == LV_EHIP, b.p == old, b.cap, b[3], ((long)st().mallocs - m0) - ((long)st().frees - f0));
    }
    rc = b.grow_keep(128, 4, 0, s1, false);
    printf("after %d %zu %d\n", rc, b.cap, b[3]);
    DevBuf<void> v{};
    rc = v.need(16);
    std::memcpy(v.p, "0123456789abcdef", 16);
    rc = rc ? rc : v.grow_keep(32, 6, 10, s1, false);   // (bytes)
    printf("bytes %d %zu %.6s\n", rc, v.cap, (const char*)v.p);
    release_all(b, v);
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    return 0;
}

static int stage() {
    hipStream_t s1 = nullptr;
    if (hipStreamCreateWithFlags(&s1, hipStreamNonBlocking) != hipSuccess) return 2;
    PointStage ps{};
    int rc = ps.reserve(s1, 0);
    rc = rc ? rc : ps.upload(s1);
    printf("empty %d %ld %d %d\n", rc, (long)st().mallocs, ps.h.p == nullptr, ps.d.p == nullptr);
    // two arrays: 3 points 12 bytes apart, 2 points 32 bytes apart (the bytes between the points are poison)
    float a[9], b[16];
    for (int i = 0; i < 9; ++i) a[i] = (float)(i + 1);
    for (int i = 0; i < 16; ++i) b[i] = -777.f;
    for (int p = 0; p < 2; ++p)
        for (int c = 0; c < 3; ++c) b[8 * p + c] = (float)(100 + 3 * p + c);
    size_t mark = st().log.size();
    rc = ps.reserve(s1, 5);
    ps.append(a, 12, 3);
    ps.append(b, 32, 2);
    rc = rc ? rc : ps.upload(s1);
    print_log("first", mark, s1);
    printf("packed %d %zu", rc, ps.n);
    for (int i = 0; i < 15; ++i) printf(" %g", ps.d[i]);
    printf("\ncaps %zu %zu\n", ps.h.cap, ps.d.cap);
    mark = st().log.size();
    rc = ps.reserve(s1, 6);
    for (int i = 0; i < 2; ++i) ps.append(a, 12, 3);
    rc = rc ? rc : ps.upload(s1);
    print_log("second", mark, s1);
    printf("second_packed %d %zu %g %g\n", rc, ps.n, ps.d[9], ps.d[17]);
    mark = st().log.size();
    rc = ps.reserve(s1, 2);   // (fits: the wait stays, nothing is allocated)
    ps.append(b, 32, 2);
    rc = rc ? rc : ps.upload(s1);
    print_log("third", mark, s1);
    printf("third_packed %d %zu %g %g\n", rc, ps.n, ps.d[0], ps.d[5]);
    // doubling from a floor of 1024 floats, as the map queries stage
    PointStage pq{};
    rc = pq.reserve(s1, 2, 1024);
    printf("floor %d %zu %zu\n", rc, pq.h.cap, pq.d.cap);
    rc = pq.reserve(s1, 400, 1024);
    printf("doubled %d %zu %zu\n", rc, pq.h.cap, pq.d.cap);
    ps.release();
    pq.release();
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    return 0;
}

static int counters() {
    hipStream_t s1 = nullptr;
    if (hipStreamCreateWithFlags(&s1, hipStreamNonBlocking) != hipSuccess) return 2;
    Counters4 c{};
    printf("lazy %ld\n", (long)st().mallocs);
    size_t mark = st().log.size();
    int rc = c.zero(s1);
    print_log("zero", mark, s1);
    uint64_t out[4] = {9, 9, 9, 9};
    rc = rc ? rc : c.read(s1, out);
    printf("zeroed %d %llu %llu %llu %llu\n", rc, (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
           (unsigned long long)out[3]);
    c.d[0] = 1ull;
    c.d[1] = 0xFFFFFFFFFFFFFFFFull;
    c.d[2] = 1ull << 40;
    c.d[3] = 12345ull;
    mark = st().log.size();
    rc = c.read(s1, out);
    print_log("read", mark, s1);
    printf("values %d %llu %llu %llu %llu\n", rc, (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
           (unsigned long long)out[3]);
    rc = c.read(s1, nullptr);
    mark = st().log.size();
    rc = rc ? rc : c.zero(s1);
    printf("again %d %ld %ld\n", rc, count("hipMalloc", mark), count("hipHostMalloc", mark));
    rc = c.read(s1, out);   // (the device words held the values above)
    printf("rezeroed %d %llu %llu %llu %llu\n", rc, (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2],
           (unsigned long long)out[3]);
    c.release();
    printf("released %ld %ld\n", (long)st().mallocs, (long)st().frees);
    printf("blocks %u %u %u %u %u\n", blocks_of(0), blocks_of(1), blocks_of(256), blocks_of(257), blocks_of(9, 4));
    return 0;
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "exact") return exact();
    if (which == "doubling") return doubling();
    if (which == "failure") return failure();
    if (which == "keep") return keep();
    if (which == "stage") return stage();
    if (which == "counters") return counters();
    return 2;
}
