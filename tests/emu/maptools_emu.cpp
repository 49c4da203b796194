// tests/emu/maptools_emu.cpp — HOST test of MapSide / MapTools (limo-velo_amd/csrc/lv_maptools.hpp): how every tool on the point
// map orders itself against an insert in flight and a background rebuild, what it judges before the map is looked at, when it
// zeroes its outputs, what a removal journals, and what is freed in which order.
// TEST INFRASTRUCTURE ONLY: built by tests/test_maptools_host.py into tests/emu/_build/ (once plain, once with AddressSanitizer +
// UndefinedBehaviorSanitizer), never shipped.  It compiles the product's own lv_maptools.hpp and tool headers, unchanged, against
// the stand-in hip_runtime.h next to this file.  The stores' member functions and the tools' launches (the .hip files' in the
// product) and the rebuild are stand-ins here: each logs its name and its telling arguments through the HIP stand-in and returns
// LV_OK, or LV_ERANGE when the scenario made it the failing one.  The expected logs below are literals written down from
// lv_api.hip as it stood before the call order moved: nothing of them is produced by the code under test.
// Usage: maptools_emu <scenario>; exit 0 = pass.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../limo-velo_amd/csrc/lv_maptools.hpp"

using namespace lv;

static char g_err[512] = "";
void lv::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// (variadic: a braced list inside the condition carries commas)
#define CHECK(...)                                                                                                  \
    do {                                                                                                            \
        if (!(__VA_ARGS__)) {                                                                                       \
            fprintf(stderr, "CHECK FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #__VA_ARGS__, g_err); \
            std::_Exit(1);                                                                                          \
        }                                                                                                           \
    } while (0)

namespace {

using Calls = std::vector<std::string>;

const int FAILED = LV_ERANGE;   // what the failing stand-in returns (no code under test produces it)
int g_seen = 0;                 // stand-in calls since arm()
int g_fail_at = -1;             // the stand-in call (counted from 0) that fails; -1: none
void arm(int fail_at) { g_seen = 0; g_fail_at = fail_at; }

std::string fmt(const char* f, ...) {
    char b[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof(b), f, ap);
    va_end(ap);
    return b;
}
int ran(const std::string& what, hipStream_t s = nullptr) {
    emu_hip::call(what.c_str(), s);
    return g_seen++ == g_fail_at ? FAILED : LV_OK;
}
size_t mark() { return emu_hip::state().log.size(); }
// what ran since `from`: the stand-ins and the stream's calls (allocations are counted, not listed)
Calls calls(size_t from) {
    Calls v;
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i)
        if (log[i].call != "hipMalloc" && log[i].call != "hipFree" && log[i].call != "hipHostMalloc" && log[i].call != "hipHostFree") v.push_back(log[i].call);
    return v;
}
long live() { return emu_hip::state().mallocs - emu_hip::state().frees; }
// the stream the first `name` since `from` ran on
hipStream_t stream_of(size_t from, const std::string& name) {
    auto& log = emu_hip::state().log;
    for (size_t i = from; i < log.size(); ++i)
        if (log[i].call == name) return log[i].stream;
    return nullptr;
}
bool is_hip(const std::string& c) { return c.compare(0, 3, "hip") == 0; }
void show(const Calls& v) {
    for (const auto& c : v) fprintf(stderr, "    %s\n", c.c_str());
}
#define SAME(got, ...)                                                \
    do {                                                              \
        const Calls _g = (got), _w = Calls{__VA_ARGS__};              \
        if (_g != _w) {                                               \
            fprintf(stderr, "%s:%d: the calls were\n", __FILE__, __LINE__); \
            show(_g);                                                 \
            fprintf(stderr, "  expected\n");                          \
            show(_w);                                                 \
            std::_Exit(1);                                            \
        }                                                             \
    } while (0)
// the call was refused with this code and exactly this message
#define REFUSED(call, code, msg)                                \
    do {                                                        \
        g_err[0] = 0;                                           \
        CHECK((call) == (code) && std::string(g_err) == (msg)); \
    } while (0)

int b(const void* p) { return p ? 1 : 0; }

uint32_t g_remove = 0;   // what a removing stand-in takes out of the map it is handed

}  // namespace

// ---- the stand-ins of lv_map.hip and lv_query.hip
int MapStore::settle(hipStream_t s) { return ran("settle", s); }

int QueryStore::ensure_rank(const MapStore& map, hipStream_t s, const uint32_t** rank) {   // (NULL when ranks equal ids)
    if (int rc = ran("ensure_rank", s)) return rc;
    LV_TRY(d_rank.need(map.n_ids));
    *rank = map.n_ids != map.m ? d_rank.p : nullptr;
    return LV_OK;
}
int QueryStore::knn(const MapStore&, hipStream_t s, const void*, size_t, size_t, int, float, uint32_t*, float*, int32_t*) { return ran("QueryStore::knn", s); }
int QueryStore::radius(const MapStore&, hipStream_t s, const void*, size_t, size_t, float, size_t*, uint32_t*, float*, size_t, size_t*) {
    return ran("QueryStore::radius", s);
}
int QueryStore::box(const MapStore&, hipStream_t s, const float*, const float*, uint32_t*, float*, size_t, size_t*) { return ran("QueryStore::box", s); }
void QueryStore::release() {
    emu_hip::call("QueryStore::release");
    d_rank.release();
}

// ---- lv_visibility.hip
int VisStore::build(hipStream_t s, const lv_view*, size_t n_views, const VisRule& q) {
    if (int rc = ran(fmt("VisStore::build(n_views=%zu)", n_views), s)) return rc;
    return d_blob.need(vis_blob_bytes(q));
}
int VisStore::ensure_hits(size_t n) {
    if (int rc = ran(fmt("ensure_hits(n=%zu)", n))) return rc;
    return d_hits.resize(n);   // (exactly n: a copy of more reads past it under AddressSanitizer)
}
void VisStore::release() {
    emu_hip::call("VisStore::release");
    release_all(d_blob, d_hits);
}
int lv::vis_classify(MapStore& map, hipStream_t s, const void* d_blob, const VisRule&, const uint32_t* rank, uint8_t* hits, bool remove, uint32_t* n_removed) {
    if (int rc = ran(fmt("vis_classify(m=%u,blob=%d,remove=%d,rank=%d,hits=%d)", map.m, b(d_blob), (int)remove, b(rank), b(hits)), s)) return rc;
    if (hits) std::memset(hits, 7, map.m);
    if (remove) map.m -= g_remove;   // (the outputs are of the map as it stood BEFORE the removal)
    if (n_removed) *n_removed = remove ? g_remove : 0;
    return LV_OK;
}

// ---- lv_surface.hip
int SurfaceStore::ensure(size_t n_ids, size_t m, int job) {
    if (int rc = ran(fmt("SurfaceStore::ensure(n_ids=%zu,m=%zu,job=%d)", n_ids, m, job))) return rc;
    LV_TRY(d_part.need(2 * 256));
    LV_TRY(d_normals.resize(3 * m));
    return need_all(m, d_curv, d_mean, d_used);
}
void SurfaceStore::release() {
    emu_hip::call("SurfaceStore::release");
    release_all(d_val, d_part, d_normals, d_curv, d_mean, d_used, d_flags);
}
int lv::surface_search(const MapStore&, hipStream_t s, SurfaceStore&, const SurfRule& q, const uint32_t* rank) {
    return ran(fmt("surface_search(job=%d,k=%d,rank=%d)", q.job, q.k, b(rank)), s);
}
int lv::surface_finish(const MapStore&, hipStream_t s, SurfaceStore&, const SurfRule&, const uint32_t* rank) { return ran(fmt("surface_finish(rank=%d)", b(rank)), s); }
// as the real one: a job-1 rule that is not fixed is resolved (threshold 1.5, stats 0.25, 0.5, 1.5) and comes back fixed; a fixed
// one reports no mean and no deviation
int lv::surface_outliers(MapStore& map, hipStream_t s, SurfaceStore& st, SurfRule& q, const uint32_t* rank, bool want_flags, bool remove, uint32_t* n_removed,
                         double stats[3], bool reuse_values) {
    if (int rc = ran(fmt("surface_outliers(m=%u,job=%d,fixed=%d,threshold=%g,rank=%d,flags=%d,remove=%d,n_removed=%d,stats=%d,dry_pass=%d)", map.m, q.job,
                         q.fixed_threshold, q.threshold, b(rank), (int)want_flags, (int)remove, b(n_removed), b(stats), (int)reuse_values),
                     s))
        return rc;
    LV_TRY(st.d_val.need(1));   // (every store it is handed holds something afterwards: one that is not released leaks)
    LV_TRY(st.d_flags.resize(map.m));
    std::memset(st.d_flags.p, 5, map.m);
    double mu = 0.0, sigma = 0.0;
    if (q.job == 1 && !q.fixed_threshold) {
        mu = 0.25;
        sigma = 0.5;
        q.threshold = 1.5;
        q.fixed_threshold = 1;
    }
    if (stats) { stats[0] = q.job == 1 ? mu : 0.0; stats[1] = q.job == 1 ? sigma : 0.0; stats[2] = q.job == 1 ? q.threshold : 0.0; }
    if (remove) map.m -= g_remove;
    if (n_removed) *n_removed = remove ? g_remove : 0;
    return LV_OK;
}

// ---- lv_cluster.hip
int ClusterStore::ensure(size_t n_ids, size_t m) {
    if (int rc = ran(fmt("ClusterStore::ensure(n_ids=%zu,m=%zu)", n_ids, m))) return rc;
    LV_TRY(d_sizes.need(4));
    for (Buf<uint8_t, DeviceMem>* x : {&d_mask, &d_seeds, &d_flags}) LV_TRY(x->resize(m));
    return d_labels.resize(m);
}
void ClusterStore::release() {
    emu_hip::call("ClusterStore::release");
    release_all(d_labels, d_sizes, d_mask, d_seeds, d_flags);
}
int lv::cluster_components(const MapStore&, hipStream_t s, ClusterStore&, const ClusterRule& q, const uint32_t* rank, const uint8_t* mask) {
    return ran(fmt("cluster_components(seeded=%d,rank=%d,mask=%d)", q.seeded, b(rank), b(mask)), s);
}
int lv::cluster_labels(const MapStore&, hipStream_t s, ClusterStore& st, const ClusterRule&, const uint32_t* rank, bool want_labels, size_t* n_clusters) {
    if (int rc = ran(fmt("cluster_labels(rank=%d,labels=%d)", b(rank), (int)want_labels), s)) return rc;
    for (uint32_t i = 0; i < 4; ++i) st.d_sizes.p[i] = 40 - 10 * i;
    *n_clusters = 3;
    return LV_OK;
}
int lv::cluster_remove(MapStore& map, hipStream_t s, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, const uint8_t* seeds, uint8_t* flags, bool remove,
                       uint32_t* n_removed) {
    if (int rc = ran(fmt("cluster_remove(m=%u,seeded=%d,rank=%d,seeds=%d,flags=%d,remove=%d)", map.m, q.seeded, b(rank), b(seeds), b(flags), (int)remove), s)) return rc;
    if (flags) std::memset(flags, 3, map.m);
    if (remove) map.m -= g_remove;
    *n_removed = remove ? g_remove : 0;
    (void)st;
    return LV_OK;
}

// ---- lv_planes.hip
int PlaneStore::ensure(size_t n_ids, size_t m, uint32_t iterations) {
    if (int rc = ran(fmt("PlaneStore::ensure(n_ids=%zu,m=%zu,iterations=%u)", n_ids, m, iterations))) return rc;
    LV_TRY(d_mask.resize(m));
    return d_labels.resize(m);
}
void PlaneStore::release() {
    emu_hip::call("PlaneStore::release");
    release_all(d_labels, d_mask);
}
int lv::planes_extract(const MapStore&, hipStream_t s, PlaneStore&, const PlaneRule&, const uint32_t* rank, const uint8_t* mask, bool want_labels, lv_plane* planes,
                       size_t* n_planes) {
    if (int rc = ran(fmt("planes_extract(rank=%d,mask=%d,labels=%d)", b(rank), b(mask), (int)want_labels), s)) return rc;
    for (uint32_t i = 0; i < 2; ++i) {
        planes[i] = lv_plane{};
        planes[i].inliers = 100 + i;
    }
    *n_planes = 2;
    return LV_OK;
}

// ---- lv_paint.hip
int PaintStore::run(const MapStore& map, hipStream_t s, const lv_camera_view*, const PaintCam*, const PaintRule& q, const uint32_t* rank, bool want_rgb, bool want_depth,
                    bool want_seen) {
    if (int rc = ran(fmt("PaintStore::run(n_views=%d,rank=%d,rgb=%d,depth=%d,seen=%d)", q.n_views, b(rank), (int)want_rgb, (int)want_depth, (int)want_seen), s)) return rc;
    LV_TRY(d_rgb.resize(3 * (size_t)map.m));
    LV_TRY(d_depth.resize(map.m));
    return d_seen.resize(map.m);
}
void PaintStore::release() {
    emu_hip::call("PaintStore::release");
    release_all(d_rgb, d_depth, d_seen);
}

namespace {

// ---- the stand-in rebuild: what MapTools and MapSide call of MapRebuild<MapStore>.  journal_replay keeps the functor and a copy
// of the journaled bytes, as the real one does, for the scenario to replay on a second store; `adopt` stands for "a copy found
// ready is adopted first" (journal_replay) and for the adoption status(wait) waits for.
struct FakeRebuild {
    using Replay = std::function<int(MapStore&, hipStream_t, const void*)>;
    Replay replay;
    std::vector<unsigned char> blob;
    const void* src = nullptr;   // where the journaled bytes were read
    std::function<void(MapStore&)> adopt;

    int poll(MapStore&, const CtxStreams& cs) { return ran("poll", cs.stream); }
    int journal_replay(MapStore& map, const CtxStreams& cs, const void* src, size_t bytes, Replay r) {
        if (int rc = ran(fmt("journal_replay(bytes=%zu)", bytes), cs.stream)) return rc;
        replay = std::move(r);
        this->src = src;
        blob.assign(static_cast<const unsigned char*>(src), static_cast<const unsigned char*>(src) + bytes);
        if (adopt) adopt(map);
        return LV_OK;
    }
    int order(const CtxStreams&, hipStream_t s) { return ran("order", s); }
    int status(MapStore& map, const CtxStreams& cs, int wait, uint64_t* out) {
        if (int rc = ran(fmt("status(wait=%d,out=%d)", wait, b(out)), cs.stream)) return rc;
        if (adopt) adopt(map);
        return LV_OK;
    }
};
using Tools = MapTools<FakeRebuild>;
using Side = MapSide<FakeRebuild>;

// a context's map side as lv_api.hip holds it, with arguments every tool accepts
struct Ctx {
    MapStore map;
    FakeRebuild rb;
    Tools t;
    hipStream_t s = emu_hip::new_handle<hipStream_t>(), side_stream = emu_hip::new_handle<hipStream_t>();
    hipEvent_t ev = emu_hip::new_handle<hipEvent_t>();
    float ret[3] = {1.f, 0.f, 0.f};
    lv_view view{};
    lv_visibility_params vp{};
    lv_surface_params sp{};
    lv_outlier_params op{};
    lv_cluster_params cp{};
    lv_plane_params pp{};
    uint8_t image[4] = {0, 0, 0, 0};
    lv_camera_view cam{};
    lv_paint_params ap{};

    Ctx() {
        view.R[0] = view.R[4] = view.R[8] = 1.f;
        view.points = ret;
        view.stride = 12;
        view.n = 1;
        default_visibility_params(&vp);
        vp.width = 8;
        vp.height = 4;
        default_surface_params(&sp);
        default_outlier_params(&op);
        default_cluster_params(&cp);
        default_plane_params(&pp);
        cam.R[0] = cam.R[4] = cam.R[8] = 1.f;
        cam.fx = cam.fy = 1.f;
        cam.width = cam.height = 1;
        cam.format = LV_IMAGE_MONO8;
        cam.image = image;
        cam.row_stride = 1;
        default_paint_params(&ap);
    }
    ~Ctx() {
        t.release();
        map.d_orig.release();
    }
    Side side() { return Side{map, rb, CtxStreams{s, side_stream, ev, true}, s}; }
    // a built map of m living points among n_ids
    void living(uint32_t m, uint32_t n_ids) {
        CHECK(map.d_orig.need(n_ids ? n_ids : 1) == LV_OK);
        map.built = true;
        map.m = m;
        map.n_ids = n_ids;
        ++map.gen;
    }
};

// `call` ran these calls and returned LV_OK; then each stand-in of them fails in turn: the call ends with its code and nothing
// runs after it.  (The call must leave the map as it found it: g_remove = 0 here.)
void full_log_then_each_failing(const std::function<int()>& call, const Calls& want) {
    arm(-1);
    size_t t = mark();
    CHECK(call() == LV_OK);
    SAME(calls(t), want);
    int k = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        if (is_hip(want[i])) continue;
        arm(k++);
        t = mark();
        CHECK(call() == FAILED);
        SAME(calls(t), Calls(want.begin(), want.begin() + i + 1));
    }
    arm(-1);
    CHECK(call() == LV_OK);   // (the caller looks at the outputs of a call that went through)
}

const char* const CAPACITY = "capacity %zu < %zu living points";

// ---- scenarios
void ready() {
    Ctx c;
    c.living(3, 5);
    size_t t = mark();
    CHECK(c.side().ready() == LV_OK);
    SAME(calls(t), "settle", "poll");
    CHECK(stream_of(t, "settle") == c.s && stream_of(t, "poll") == c.s);
    arm(0);   // a failed settle: its code, no poll
    t = mark();
    CHECK(c.side().ready() == FAILED);
    SAME(calls(t), "settle");
    arm(1);   // a failed poll: its code, nothing after it
    t = mark();
    CHECK(c.t.knn(c.side(), c.ret, 12, 1, 1, 1.f, nullptr, nullptr, nullptr) == FAILED);
    SAME(calls(t), "settle", "poll");
    arm(-1);
}

void queries() {
    Ctx c;
    c.living(3, 5);
    uint32_t idx[4];
    float d2[4];
    int32_t found[1];
    size_t off[2], total = 0;
    const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    // (they judge nothing before the map: the store's call judges the arguments, on the settled map)
    full_log_then_each_failing([&] { return c.t.knn(c.side(), c.ret, 12, 1, 1, 1.f, idx, d2, found); }, {"settle", "poll", "QueryStore::knn"});
    full_log_then_each_failing([&] { return c.t.radius_search(c.side(), c.ret, 12, 1, 1.f, off, idx, d2, 4, &total); }, {"settle", "poll", "QueryStore::radius"});
    full_log_then_each_failing([&] { return c.t.box_search(c.side(), lo, hi, idx, d2, 1, &total); }, {"settle", "poll", "QueryStore::box"});
    Ctx e;   // an unbuilt map is the store's call to answer as well
    const size_t t = mark();
    CHECK(e.t.knn(e.side(), e.ret, 12, 1, 1, 1.f, idx, d2, found) == LV_OK);
    SAME(calls(t), "settle", "poll", "QueryStore::knn");
}

void normals() {
    Ctx c;
    float n[9], curv[3], mean[3];
    int32_t used[3];
    size_t t = mark();
    lv_surface_params bad = c.sp;
    bad.k = 1;
    REFUSED(c.t.normals(c.side(), &bad, n, curv, mean, used, 3), LV_EINVAL, fmt("k = %d: must be in 2..%d", 1, SURF_MAX_K));
    REFUSED(c.t.normals(c.side(), nullptr, n, curv, mean, used, 3), LV_EINVAL, "null argument");
    CHECK(calls(t).empty());   // neither settle nor poll
    // an unbuilt map, and an empty one: LV_OK without ensure_rank
    CHECK(c.t.normals(c.side(), &c.sp, n, curv, mean, used, 0) == LV_OK);
    SAME(calls(t), "settle", "poll");
    c.living(0, 5);
    t = mark();
    CHECK(c.t.normals(c.side(), &c.sp, n, curv, mean, used, 0) == LV_OK);
    SAME(calls(t), "settle", "poll");
    c.living(3, 5);
    t = mark();
    REFUSED(c.t.normals(c.side(), &c.sp, n, curv, mean, used, 2), LV_EINVAL, fmt(CAPACITY, (size_t)2, (size_t)3));
    SAME(calls(t), "settle", "poll");
    full_log_then_each_failing([&] { return c.t.normals(c.side(), &c.sp, n, curv, mean, used, 3); },
                               {"settle", "poll", "ensure_rank", "SurfaceStore::ensure(n_ids=5,m=3,job=0)", "surface_search(job=0,k=10,rank=1)", "surface_finish(rank=1)",
                                "hipMemcpyAsync", "hipMemcpyAsync", "hipMemcpyAsync", "hipMemcpyAsync", "hipStreamSynchronize"});
    // surface_finish only for normals or curvature; only the outputs asked for travel
    full_log_then_each_failing([&] { return c.t.normals(c.side(), &c.sp, nullptr, nullptr, mean, nullptr, 3); },
                               {"settle", "poll", "ensure_rank", "SurfaceStore::ensure(n_ids=5,m=3,job=0)", "surface_search(job=0,k=10,rank=1)", "hipMemcpyAsync",
                                "hipStreamSynchronize"});
    full_log_then_each_failing([&] { return c.t.normals(c.side(), &c.sp, nullptr, curv, nullptr, nullptr, 3); },
                               {"settle", "poll", "ensure_rank", "SurfaceStore::ensure(n_ids=5,m=3,job=0)", "surface_search(job=0,k=10,rank=1)", "surface_finish(rank=1)",
                                "hipMemcpyAsync", "hipStreamSynchronize"});
    c.living(5, 5);   // no dead id: ranks are ids
    t = mark();
    CHECK(c.t.normals(c.side(), &c.sp, nullptr, nullptr, nullptr, nullptr, 5) == LV_OK);
    SAME(calls(t), "settle", "poll", "ensure_rank", "SurfaceStore::ensure(n_ids=5,m=5,job=0)", "surface_search(job=0,k=10,rank=0)", "hipStreamSynchronize");
}

void cluster() {
    Ctx c;
    int32_t labels[4] = {-9, -9, -9, -9};
    uint32_t sizes[4] = {0, 0, 0, 0};
    const uint8_t mask[3] = {1, 1, 0};
    size_t C = 77;
    size_t t = mark();
    lv_cluster_params bad = c.cp;
    bad.min_size = 0;
    REFUSED(c.t.cluster_map(c.side(), &bad, nullptr, labels, 3, sizes, 4, &C), LV_EINVAL, "min_size = 0: must be >= 1");
    CHECK(calls(t).empty() && C == 77);
    // an accepted call on an unbuilt or empty map zeroes the count and ends there
    CHECK(c.t.cluster_map(c.side(), &c.cp, nullptr, labels, 0, sizes, 4, &C) == LV_OK && C == 0);
    SAME(calls(t), "settle", "poll");
    c.living(0, 5);
    C = 77;
    t = mark();
    CHECK(c.t.cluster_map(c.side(), &c.cp, nullptr, labels, 0, sizes, 4, &C) == LV_OK && C == 0);
    SAME(calls(t), "settle", "poll");
    // a refused capacity leaves it untouched; without labels the capacity is not judged
    c.living(3, 5);
    C = 77;
    t = mark();
    REFUSED(c.t.cluster_map(c.side(), &c.cp, nullptr, labels, 2, sizes, 4, &C), LV_EINVAL, fmt(CAPACITY, (size_t)2, (size_t)3));
    SAME(calls(t), "settle", "poll");
    CHECK(C == 77);
    full_log_then_each_failing([&] { return c.t.cluster_map(c.side(), &c.cp, nullptr, nullptr, 0, sizes, 4, &C); },
                               {"settle", "poll", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "cluster_components(seeded=0,rank=1,mask=0)",
                                "cluster_labels(rank=1,labels=0)", "hipMemcpyAsync", "hipStreamSynchronize"});
    CHECK(C == 3 && sizes[0] == 40 && sizes[1] == 30 && sizes[2] == 20 && sizes[3] == 0);
    // with a mask (uploaded and waited for) and labels; the sizes as far as there is room
    sizes[0] = sizes[1] = sizes[2] = 0;
    full_log_then_each_failing([&] { return c.t.cluster_map(c.side(), &c.cp, mask, labels, 3, sizes, 2, &C); },
                               {"settle", "poll", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "hipMemcpyAsync", "hipStreamSynchronize",
                                "cluster_components(seeded=0,rank=1,mask=1)", "cluster_labels(rank=1,labels=1)", "hipMemcpyAsync", "hipMemcpyAsync",
                                "hipStreamSynchronize"});
    CHECK(C == 3 && sizes[0] == 40 && sizes[1] == 30 && sizes[2] == 0 && labels[3] == -9);
    CHECK(std::memcmp(c.t.cluster.d_mask.p, mask, 3) == 0);
    // a failing call has zeroed the count (the rule and the capacity had accepted it)
    arm(2);
    C = 77;
    CHECK(c.t.cluster_map(c.side(), &c.cp, nullptr, nullptr, 0, nullptr, 0, &C) == FAILED && C == 0);
    arm(-1);
    t = mark();
    CHECK(c.t.cluster_map(c.side(), &c.cp, nullptr, nullptr, 0, nullptr, 0, nullptr) == LV_OK);   // (sizes not asked for: no copy)
    SAME(calls(t), "settle", "poll", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "cluster_components(seeded=0,rank=1,mask=0)", "cluster_labels(rank=1,labels=0)",
         "hipStreamSynchronize");
}

void planes() {
    Ctx c;
    int32_t labels[4] = {-9, -9, -9, -9};
    lv_plane out[3];
    std::memset(out, 0, sizeof(out));
    const uint8_t mask[3] = {0, 1, 1};
    size_t P = 77;
    size_t t = mark();
    lv_plane_params bad = c.pp;
    bad.iterations = 0;
    REFUSED(c.t.extract_planes(c.side(), &bad, nullptr, labels, 3, out, 3, &P), LV_EINVAL, fmt("iterations = %u: must be in 1..%u", 0u, PLANE_MAX_ITERATIONS));
    CHECK(calls(t).empty() && P == 77);
    CHECK(c.t.extract_planes(c.side(), &c.pp, nullptr, labels, 0, out, 3, &P) == LV_OK && P == 0);
    SAME(calls(t), "settle", "poll");
    c.living(0, 5);
    P = 77;
    t = mark();
    CHECK(c.t.extract_planes(c.side(), &c.pp, nullptr, labels, 0, out, 3, &P) == LV_OK && P == 0);
    SAME(calls(t), "settle", "poll");
    c.living(3, 5);
    P = 77;
    t = mark();
    REFUSED(c.t.extract_planes(c.side(), &c.pp, nullptr, labels, 2, out, 3, &P), LV_EINVAL, fmt(CAPACITY, (size_t)2, (size_t)3));
    SAME(calls(t), "settle", "poll");
    CHECK(P == 77);
    full_log_then_each_failing([&] { return c.t.extract_planes(c.side(), &c.pp, nullptr, nullptr, 0, out, 1, &P); },
                               {"settle", "poll", "ensure_rank", "PlaneStore::ensure(n_ids=5,m=3,iterations=512)", "planes_extract(rank=1,mask=0,labels=0)"});
    CHECK(P == 2 && out[0].inliers == 100 && out[1].inliers == 0);   // (room for one record)
    full_log_then_each_failing([&] { return c.t.extract_planes(c.side(), &c.pp, mask, labels, 3, out, 3, &P); },
                               {"settle", "poll", "ensure_rank", "PlaneStore::ensure(n_ids=5,m=3,iterations=512)", "hipMemcpyAsync", "hipStreamSynchronize",
                                "planes_extract(rank=1,mask=1,labels=1)", "hipMemcpy"});
    CHECK(P == 2 && out[1].inliers == 101 && out[2].inliers == 0 && labels[3] == -9 && std::memcmp(c.t.planes.d_mask.p, mask, 3) == 0);
}

void paint() {
    Ctx c;
    float rgb[9], depth[3];
    uint8_t seen[4] = {9, 9, 9, 9};
    size_t t = mark();
    lv_paint_params bad = c.ap;
    bad.zbuf_scale = 0;
    REFUSED(c.t.paint_map(c.side(), &c.cam, 1, &bad, rgb, depth, seen), LV_EINVAL, fmt("zbuf_scale = %d: must be in 1..%d", 0, PAINT_MAX_SCALE));
    REFUSED(c.t.paint_map(c.side(), &c.cam, 0, &c.ap, rgb, depth, seen), LV_EINVAL, fmt("n_views = %zu: must be in 1..%d", (size_t)0, PAINT_MAX_VIEWS));
    CHECK(calls(t).empty());
    CHECK(c.t.paint_map(c.side(), &c.cam, 1, &c.ap, rgb, depth, seen) == LV_OK);
    SAME(calls(t), "settle", "poll");
    c.living(0, 5);
    t = mark();
    CHECK(c.t.paint_map(c.side(), &c.cam, 1, &c.ap, rgb, depth, seen) == LV_OK);
    SAME(calls(t), "settle", "poll");
    c.living(3, 5);
    t = mark();
    CHECK(c.t.paint_map(c.side(), &c.cam, 1, &c.ap, nullptr, nullptr, nullptr) == LV_OK);   // nothing asked for: the same
    SAME(calls(t), "settle", "poll");
    full_log_then_each_failing([&] { return c.t.paint_map(c.side(), &c.cam, 1, &c.ap, rgb, depth, seen); },
                               {"settle", "poll", "ensure_rank", "PaintStore::run(n_views=1,rank=1,rgb=1,depth=1,seen=1)", "hipMemcpyAsync", "hipMemcpyAsync",
                                "hipMemcpyAsync", "hipStreamSynchronize"});
    full_log_then_each_failing([&] { return c.t.paint_map(c.side(), &c.cam, 1, &c.ap, nullptr, nullptr, seen); },
                               {"settle", "poll", "ensure_rank", "PaintStore::run(n_views=1,rank=1,rgb=0,depth=0,seen=1)", "hipMemcpyAsync", "hipStreamSynchronize"});
}

void remove_dynamic() {
    Ctx c;
    uint8_t hits[5] = {9, 9, 9, 9, 9};
    size_t nr = 77;
    size_t t = mark();
    // *n_removed is zeroed even when the rule refuses
    lv_visibility_params bad = c.vp;
    bad.min_hits = 2;
    REFUSED(c.t.remove_dynamic(c.side(), &c.view, 1, &bad, hits, &nr), LV_EINVAL, fmt("min_hits = %d: must be in 1..n_views", 2));
    CHECK(calls(t).empty() && nr == 0);
    nr = 77;
    REFUSED(c.t.remove_dynamic(c.side(), nullptr, 1, &c.vp, hits, &nr), LV_EINVAL, "null argument");
    CHECK(calls(t).empty() && nr == 0);
    CHECK(c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, hits, &nr) == LV_OK);   // an unbuilt map: VisStore::build does not run
    SAME(calls(t), "settle", "poll");
    VisRule q{};
    CHECK(visibility_rule(&c.view, 1, &c.vp, &q) == LV_OK);
    const size_t blob = 256 + 8 * 4 * sizeof(float);   // the poses padded to 256 B, one 8 x 4 image
    CHECK(vis_blob_bytes(q) == blob);
    c.living(3, 5);
    // a dry run: neither journal_replay nor order
    c.vp.dry_run = 1;
    full_log_then_each_failing([&] { return c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, nullptr, &nr); },
                               {"settle", "poll", "VisStore::build(n_views=1)", "vis_classify(m=3,blob=1,remove=0,rank=0,hits=0)"});
    full_log_then_each_failing([&] { return c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, hits, &nr); },
                               {"settle", "poll", "VisStore::build(n_views=1)", "ensure_hits(n=3)", "ensure_rank", "vis_classify(m=3,blob=1,remove=0,rank=1,hits=1)",
                                "hipMemcpy"});
    CHECK(nr == 0 && hits[0] == 7 && hits[2] == 7 && hits[3] == 9);   // m bytes come back
    // a removal: build, journal the blob, order on the context's stream, act
    c.vp.dry_run = 0;
    full_log_then_each_failing([&] { return c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, nullptr, nullptr); },
                               {"settle", "poll", "VisStore::build(n_views=1)", fmt("journal_replay(bytes=%zu)", blob), "order",
                                "vis_classify(m=3,blob=1,remove=1,rank=0,hits=0)"});
    g_remove = 2;
    std::memset(hits, 9, sizeof(hits));
    t = mark();
    CHECK(c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, hits, &nr) == LV_OK && nr == 2 && c.map.m == 1);
    SAME(calls(t), "settle", "poll", "VisStore::build(n_views=1)", fmt("journal_replay(bytes=%zu)", blob), "order", "ensure_hits(n=3)", "ensure_rank",
         "vis_classify(m=3,blob=1,remove=1,rank=1,hits=1)", "hipMemcpy");
    CHECK(stream_of(t, "order") == c.s && c.rb.src == c.t.vis.d_blob.p);
    CHECK(hits[0] == 7 && hits[2] == 7 && hits[3] == 9);   // of the map as it stood before the removal
    // the replay, run by the rebuild on the worker's copy and stream: the same rule, removing, no ranks, no hits, no count
    MapStore copy;
    copy.built = true;
    copy.m = 4;
    copy.n_ids = 4;
    hipStream_t ws = emu_hip::new_handle<hipStream_t>();
    g_remove = 1;
    t = mark();
    CHECK(c.rb.replay(copy, ws, c.rb.blob.data()) == LV_OK && copy.m == 3 && c.rb.blob.size() == blob);
    SAME(calls(t), "vis_classify(m=4,blob=1,remove=1,rank=0,hits=0)");
    CHECK(stream_of(t, "vis_classify(m=4,blob=1,remove=1,rank=0,hits=0)") == ws);
    // adoption inside journal_replay (m 3 -> 2, the stamp moves): ensure_hits, the copy-out and vis_classify see 2
    c.living(3, 5);
    c.rb.adopt = [](MapStore& m) { m.m = 2; m.n_ids = 2; ++m.gen; };
    g_remove = 0;
    std::memset(hits, 9, sizeof(hits));
    t = mark();
    CHECK(c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, hits, &nr) == LV_OK && nr == 0);
    SAME(calls(t), "settle", "poll", "VisStore::build(n_views=1)", fmt("journal_replay(bytes=%zu)", blob), "order", "ensure_hits(n=2)", "ensure_rank",
         "vis_classify(m=2,blob=1,remove=1,rank=0,hits=1)", "hipMemcpy");
    CHECK(hits[0] == 7 && hits[1] == 7 && hits[2] == 9);
    g_remove = 0;
}

void remove_outliers() {
    Ctx c;
    uint8_t flags[5] = {9, 9, 9, 9, 9};
    size_t nr = 77;
    double st[3] = {7.0, 7.0, 7.0};
    size_t t = mark();
    // the outputs are untouched when the rule refuses, and zeroed otherwise
    lv_outlier_params bad = c.op;
    bad.mode = 2;
    REFUSED(c.t.remove_outliers(c.side(), &bad, flags, &nr, st), LV_EINVAL, fmt("mode = %d: 0 (statistical) or 1 (radius)", 2));
    CHECK(calls(t).empty() && nr == 77 && st[0] == 7.0 && st[1] == 7.0 && st[2] == 7.0);
    CHECK(c.t.remove_outliers(c.side(), &c.op, flags, &nr, st) == LV_OK && nr == 0 && st[0] == 0.0 && st[1] == 0.0 && st[2] == 0.0);
    SAME(calls(t), "settle", "poll");
    c.living(3, 5);
    // job 1 (statistical) as a dry run: one pass, its statistics
    c.op.dry_run = 1;
    full_log_then_each_failing([&] { return c.t.remove_outliers(c.side(), &c.op, nullptr, &nr, st); },
                               {"settle", "poll", "surface_outliers(m=3,job=1,fixed=0,threshold=0,rank=0,flags=0,remove=0,n_removed=1,stats=1,dry_pass=0)"});
    CHECK(nr == 0 && st[0] == 0.25 && st[1] == 0.5 && st[2] == 1.5);
    full_log_then_each_failing([&] { return c.t.remove_outliers(c.side(), &c.op, flags, nullptr, nullptr); },
                               {"settle", "poll", "ensure_rank", "surface_outliers(m=3,job=1,fixed=0,threshold=0,rank=1,flags=1,remove=0,n_removed=1,stats=1,dry_pass=0)",
                                "hipMemcpy"});
    CHECK(flags[0] == 5 && flags[2] == 5 && flags[3] == 9);
    // job 1 removing: the dry pass resolves the rule, sizeof(SurfRule) bytes of it are journaled out of d_part, the acting call
    // runs on the dry pass's values and the statistics are the dry pass's (a fixed rule reports none)
    c.op.dry_run = 0;
    const std::string journal = fmt("journal_replay(bytes=%zu)", sizeof(SurfRule));
    full_log_then_each_failing([&] { return c.t.remove_outliers(c.side(), &c.op, nullptr, &nr, st); },
                               {"settle", "poll", "surface_outliers(m=3,job=1,fixed=0,threshold=0,rank=0,flags=0,remove=0,n_removed=0,stats=1,dry_pass=0)",
                                "SurfaceStore::ensure(n_ids=5,m=3,job=1)", "hipMemcpyAsync", "hipStreamSynchronize", journal, "order",
                                "surface_outliers(m=3,job=1,fixed=1,threshold=1.5,rank=0,flags=0,remove=1,n_removed=1,stats=1,dry_pass=1)"});
    CHECK(st[0] == 0.25 && st[1] == 0.5 && st[2] == 1.5);
    SurfRule sent;
    std::memcpy(&sent, c.t.surface.d_part.p, sizeof(sent));
    CHECK(c.rb.src == c.t.surface.d_part.p && sent.job == 1 && sent.k == 11 && sent.fixed_threshold == 1 && sent.threshold == 1.5 && c.rb.blob.size() == sizeof(SurfRule) &&
          std::memcmp(c.rb.blob.data(), &sent, sizeof(sent)) == 0);
    g_remove = 1;
    std::memset(flags, 9, sizeof(flags));
    t = mark();
    CHECK(c.t.remove_outliers(c.side(), &c.op, flags, &nr, st) == LV_OK && nr == 1 && c.map.m == 2);
    SAME(calls(t), "settle", "poll", "surface_outliers(m=3,job=1,fixed=0,threshold=0,rank=0,flags=0,remove=0,n_removed=0,stats=1,dry_pass=0)",
         "SurfaceStore::ensure(n_ids=5,m=3,job=1)", "hipMemcpyAsync", "hipStreamSynchronize", journal, "order", "ensure_rank",
         "surface_outliers(m=3,job=1,fixed=1,threshold=1.5,rank=1,flags=1,remove=1,n_removed=1,stats=1,dry_pass=1)", "hipMemcpy");
    CHECK(stream_of(t, "order") == c.s);
    CHECK(flags[0] == 5 && flags[2] == 5 && flags[3] == 9 && st[0] == 0.25 && st[2] == 1.5);
    // the replay: the rule read back from the blob, a SurfaceStore of its own, released on success and on failure
    MapStore copy;
    copy.built = true;
    copy.m = 4;
    copy.n_ids = 4;
    hipStream_t ws = emu_hip::new_handle<hipStream_t>();
    const Calls replayed = {"hipMemcpyAsync", "hipStreamSynchronize",
                            "surface_outliers(m=4,job=1,fixed=1,threshold=1.5,rank=0,flags=0,remove=1,n_removed=0,stats=0,dry_pass=0)", "SurfaceStore::release"};
    long before = live();
    t = mark();
    CHECK(c.rb.replay(copy, ws, c.rb.blob.data()) == LV_OK && copy.m == 3 && live() == before);
    SAME(calls(t), replayed);
    CHECK(stream_of(t, "hipMemcpyAsync") == ws && stream_of(t, replayed[2]) == ws && c.t.surface.d_part.p != nullptr);   // (nothing of the context's SurfaceStore)
    copy.m = 4;
    arm(0);
    t = mark();
    CHECK(c.rb.replay(copy, ws, c.rb.blob.data()) == FAILED && live() == before);
    SAME(calls(t), replayed);
    arm(-1);
    g_remove = 0;
    // job 2 (radius): no dry pass, the statistics stay zero
    c.living(3, 5);
    c.op.mode = 1;
    st[0] = st[1] = st[2] = 7.0;
    full_log_then_each_failing([&] { return c.t.remove_outliers(c.side(), &c.op, nullptr, &nr, st); },
                               {"settle", "poll", "SurfaceStore::ensure(n_ids=5,m=3,job=2)", "hipMemcpyAsync", "hipStreamSynchronize", journal, "order",
                                "surface_outliers(m=3,job=2,fixed=1,threshold=5,rank=0,flags=0,remove=1,n_removed=1,stats=1,dry_pass=0)"});
    CHECK(st[0] == 0.0 && st[1] == 0.0 && st[2] == 0.0);
    c.op.dry_run = 1;
    st[0] = st[1] = st[2] = 7.0;
    full_log_then_each_failing([&] { return c.t.remove_outliers(c.side(), &c.op, nullptr, &nr, st); },
                               {"settle", "poll", "surface_outliers(m=3,job=2,fixed=1,threshold=5,rank=0,flags=0,remove=0,n_removed=1,stats=1,dry_pass=0)"});
    CHECK(st[0] == 0.0 && st[1] == 0.0 && st[2] == 0.0);
    // adoption inside journal_replay: the acting call and the copy-out see the adopted store
    c.op.dry_run = 0;
    c.rb.adopt = [](MapStore& m) { m.m = 2; m.n_ids = 2; ++m.gen; };
    std::memset(flags, 9, sizeof(flags));
    t = mark();
    CHECK(c.t.remove_outliers(c.side(), &c.op, flags, &nr, st) == LV_OK);
    SAME(calls(t), "settle", "poll", "SurfaceStore::ensure(n_ids=5,m=3,job=2)", "hipMemcpyAsync", "hipStreamSynchronize", journal, "order", "ensure_rank",
         "surface_outliers(m=2,job=2,fixed=1,threshold=5,rank=0,flags=1,remove=1,n_removed=1,stats=1,dry_pass=0)", "hipMemcpy");
    CHECK(flags[0] == 5 && flags[1] == 5 && flags[2] == 9);
}

void remove_clusters() {
    Ctx c;
    uint8_t flags[5] = {9, 9, 9, 9, 9};
    const uint8_t mask[3] = {1, 0, 1}, seeds[3] = {0, 0, 1};
    size_t nr = 77;
    size_t t = mark();
    lv_cluster_params bad = c.cp;
    bad.radius = 0.f;
    REFUSED(c.t.remove_clusters(c.side(), &bad, nullptr, nullptr, flags, &nr), LV_EINVAL, fmt("radius = %g: finite and > 0", 0.0));
    CHECK(calls(t).empty() && nr == 77);   // untouched when the rule refuses
    CHECK(c.t.remove_clusters(c.side(), &c.cp, nullptr, nullptr, flags, &nr) == LV_OK && nr == 0);
    SAME(calls(t), "settle", "poll");
    c.living(3, 5);
    // a removal waits for a rebuild in flight to land before it looks at ranks; a dry run does not
    full_log_then_each_failing([&] { return c.t.remove_clusters(c.side(), &c.cp, nullptr, nullptr, nullptr, &nr); },
                               {"settle", "poll", "status(wait=1,out=0)", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)",
                                "cluster_components(seeded=0,rank=1,mask=0)", "cluster_remove(m=3,seeded=0,rank=1,seeds=1,flags=0,remove=1)"});
    c.cp.dry_run = 1;
    full_log_then_each_failing([&] { return c.t.remove_clusters(c.side(), &c.cp, nullptr, nullptr, flags, &nr); },
                               {"settle", "poll", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "cluster_components(seeded=0,rank=1,mask=0)",
                                "cluster_remove(m=3,seeded=0,rank=1,seeds=1,flags=1,remove=0)", "hipMemcpy"});
    CHECK(flags[0] == 3 && flags[2] == 3 && flags[3] == 9);
    // seeds set q.seeded; the mask and the seeds travel only when given, each waited for
    c.cp.dry_run = 0;
    full_log_then_each_failing([&] { return c.t.remove_clusters(c.side(), &c.cp, nullptr, seeds, nullptr, &nr); },
                               {"settle", "poll", "status(wait=1,out=0)", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "hipMemcpyAsync", "hipStreamSynchronize",
                                "cluster_components(seeded=1,rank=1,mask=0)", "cluster_remove(m=3,seeded=1,rank=1,seeds=1,flags=0,remove=1)"});
    CHECK(std::memcmp(c.t.cluster.d_seeds.p, seeds, 3) == 0);
    full_log_then_each_failing([&] { return c.t.remove_clusters(c.side(), &c.cp, mask, seeds, nullptr, &nr); },
                               {"settle", "poll", "status(wait=1,out=0)", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "hipMemcpyAsync", "hipStreamSynchronize",
                                "hipMemcpyAsync", "hipStreamSynchronize", "cluster_components(seeded=1,rank=1,mask=1)",
                                "cluster_remove(m=3,seeded=1,rank=1,seeds=1,flags=0,remove=1)"});
    CHECK(std::memcmp(c.t.cluster.d_mask.p, mask, 3) == 0 && std::memcmp(c.t.cluster.d_seeds.p, seeds, 3) == 0);
    full_log_then_each_failing([&] { return c.t.remove_clusters(c.side(), &c.cp, mask, nullptr, nullptr, &nr); },
                               {"settle", "poll", "status(wait=1,out=0)", "ensure_rank", "ClusterStore::ensure(n_ids=5,m=3)", "hipMemcpyAsync", "hipStreamSynchronize",
                                "cluster_components(seeded=0,rank=1,mask=1)", "cluster_remove(m=3,seeded=0,rank=1,seeds=1,flags=0,remove=1)"});
    // the copy adopted inside status(wait): everything after it sees that store, the flags of the map before the removal
    c.rb.adopt = [](MapStore& m) { m.m = 2; m.n_ids = 2; ++m.gen; };
    g_remove = 1;
    std::memset(flags, 9, sizeof(flags));
    t = mark();
    CHECK(c.t.remove_clusters(c.side(), &c.cp, nullptr, nullptr, flags, &nr) == LV_OK && nr == 1 && c.map.m == 1);
    SAME(calls(t), "settle", "poll", "status(wait=1,out=0)", "ensure_rank", "ClusterStore::ensure(n_ids=2,m=2)", "cluster_components(seeded=0,rank=0,mask=0)",
         "cluster_remove(m=2,seeded=0,rank=0,seeds=1,flags=1,remove=1)", "hipMemcpy");
    CHECK(flags[0] == 3 && flags[1] == 3 && flags[2] == 9);
    g_remove = 0;
}

void map_source() {
    Ctx c;
    const float4* d = reinterpret_cast<const float4*>(&c);
    uint32_t n_ids = 9, m = 9;
    // with pts given the map is not touched: no settle, no poll
    size_t t = mark();
    CHECK(c.side().source(c.ret, &d, &n_ids, &m) == LV_OK && d == nullptr && n_ids == 0 && m == 0);
    CHECK(calls(t).empty());
    // without them: settle, poll, points().  An unbuilt map and an empty one: null and zeros
    d = reinterpret_cast<const float4*>(&c);
    n_ids = m = 9;
    CHECK(c.side().source(nullptr, &d, &n_ids, &m) == LV_OK && d == nullptr && n_ids == 0 && m == 0);
    SAME(calls(t), "settle", "poll");
    c.living(0, 5);
    d = reinterpret_cast<const float4*>(&c);
    n_ids = m = 9;
    CHECK(!c.side().points(&d, &n_ids, &m) && d == nullptr && n_ids == 0 && m == 0);
    t = mark();
    n_ids = m = 9;
    CHECK(c.side().source(nullptr, &d, &n_ids, &m) == LV_OK && d == nullptr && n_ids == 0 && m == 0);
    SAME(calls(t), "settle", "poll");
    c.living(3, 5);
    c.map.built = false;   // (points left over from before a failed build are no map)
    CHECK(!c.side().points(&d, &n_ids, &m) && d == nullptr && n_ids == 0 && m == 0);
    c.map.built = true;
    CHECK(c.side().points(&d, &n_ids, &m) && d == c.map.d_orig.p && n_ids == 5 && m == 3);
    t = mark();
    d = nullptr;
    n_ids = m = 9;
    CHECK(c.side().source(nullptr, &d, &n_ids, &m) == LV_OK && d == c.map.d_orig.p && n_ids == 5 && m == 3);
    SAME(calls(t), "settle", "poll");
    // the copy a poll adopts is the one whose points are handed on
    // a failure of either ends it with nothing handed on
    for (int k = 0; k < 2; ++k) {
        arm(k);
        t = mark();
        d = reinterpret_cast<const float4*>(&c);
        n_ids = m = 9;
        CHECK(c.side().source(nullptr, &d, &n_ids, &m) == FAILED && d == nullptr && n_ids == 0 && m == 0);
        CHECK(calls(t).size() == (size_t)k + 1);
    }
    arm(-1);
    t = mark();
    CHECK(c.side().source(c.ret, &d, &n_ids, &m) == LV_OK && d == nullptr && n_ids == 0 && m == 0 && calls(t).empty());
}

void release() {
    Tools idle;
    {
        Ctx c;
        c.living(3, 5);
        uint8_t out8[3];
        float f[9];
        int32_t labels[3];
        lv_plane pl[1];
        size_t n = 0;
        c.vp.dry_run = c.op.dry_run = c.cp.dry_run = 1;
        CHECK(c.t.remove_dynamic(c.side(), &c.view, 1, &c.vp, out8, &n) == LV_OK && c.t.normals(c.side(), &c.sp, f, nullptr, nullptr, nullptr, 3) == LV_OK);
        CHECK(c.t.remove_outliers(c.side(), &c.op, out8, &n, nullptr) == LV_OK && c.t.cluster_map(c.side(), &c.cp, nullptr, labels, 3, nullptr, 0, &n) == LV_OK);
        CHECK(c.t.extract_planes(c.side(), &c.pp, nullptr, labels, 3, pl, 1, &n) == LV_OK && c.t.paint_map(c.side(), &c.cam, 1, &c.ap, f, nullptr, nullptr) == LV_OK);
        CHECK(c.t.query.d_rank.p && c.t.vis.d_blob.p && c.t.paint.d_rgb.p && c.t.surface.d_flags.p && c.t.cluster.d_labels.p && c.t.planes.d_labels.p);
        const size_t t = mark();
        c.t.release();
        // lv_destroy's order
        SAME(calls(t), "QueryStore::release", "VisStore::release", "PaintStore::release", "SurfaceStore::release", "ClusterStore::release", "PlaneStore::release");
        CHECK(live() == 1);   // (the map's points, which are not the tools')
        c.t.release();        // a second one is harmless
        CHECK(live() == 1);
    }
    CHECK(live() == 0);
    idle.release();   // of tools that never held anything
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: maptools_emu <scenario>\n"); return 2; }
    const std::string s = argv[1];
    if (s == "ready") ready();
    else if (s == "queries") queries();
    else if (s == "normals") normals();
    else if (s == "cluster") cluster();
    else if (s == "planes") planes();
    else if (s == "paint") paint();
    else if (s == "remove_dynamic") remove_dynamic();
    else if (s == "remove_outliers") remove_outliers();
    else if (s == "remove_clusters") remove_clusters();
    else if (s == "map_source") map_source();
    else if (s == "release") release();
    else { fprintf(stderr, "unknown scenario %s\n", s.c_str()); return 2; }
    const emu_hip::State& st = emu_hip::state();
    CHECK(st.mallocs == st.frees);
    printf("ok %s\n", s.c_str());
    return 0;
}
