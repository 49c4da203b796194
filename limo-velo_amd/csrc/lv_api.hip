// lv_api.hip — the C-ABI of include/limovelo_hip.h on top of the HIP kernels.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "lv_filter.hpp"
#include "lv_host.hpp"
#include "lv_knobs.hpp"
#include "lv_rebuild.hpp"
#include "lv_maptools.hpp"
#include "lv_place.hpp"
#include "lv_graph.hpp"
#include "lv_traj.hpp"
#include "lv_ndt.hpp"
#include "lv_mcl_filter.hpp"
#include "lv_elevation.hpp"
#include "lv_volumes.hpp"
#include "lv_tsdf_ray.hpp"
#include "lv_surf_align.hpp"
#include "lv_depth.hpp"
#include "lv_surf_occ.hpp"
#include "lv_surf_merge.hpp"

#include <chrono>

namespace lv {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace lv

using namespace lv;

struct lv_ctx {
    lv_params prm;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t side_stream = nullptr;   // lv_map_add_scan's insert runs here, beside the next cycle's prediction / window (see there)
    hipEvent_t ev_staged = nullptr;
    bool overlap_insert = true;          // lv_set_option "overlap_insert" / LV_OVERLAP_INSERT=0: the insert stays on the context's stream
    hipStream_t stream = nullptr;

    MapStore map;
    MapTools<MapRebuild<MapStore>> tools;   // the tools on the point map, their buffers and their order against inserts and rebuilds (lv_maptools.hpp)
    PlaceStore place;   // lv_place_*: the place database and its buffers (lv_place.hip)
    GraphStore graph;   // lv_graph_*: the pose graph and the solver's vectors (lv_graph.hip); nothing allocated before lv_graph_set
    TrajStore traj;     // lv_traj_*: the trajectory's knots, their interval records and the staging of a register call (lv_traj.hip); nothing allocated before lv_traj_set
    NdtStore ndt;       // lv_ndt_*: the target's Gaussians and the buffers of an alignment (lv_ndt.hip); nothing allocated before the first build
    MclFilterStore mclf;   // lv_occ_mcl_filter_*: the resident particles and their buffers (lv_mcl_filter.hip); nothing allocated before lv_occ_mcl_filter_set
    VolumeTools vol;    // lv_occ_*, lv_tsdf_*, lv_volume_*: the two volumes, what is built from them and what keeps those honest (lv_volumes.hpp)
    ElevStore elev;     // lv_elev_*: the elevation map and its classes (lv_elevation.hip); nothing allocated before the first build
    BatchStore batch;   // lv_iterate_batch / lv_update_batch: their own buffers (lv_batch.hip)
    MapRebuild<MapStore> rebuild;   // the background re-linearisation of `map` (lv_rebuild.hpp)

    ScanStore scan;
    CloudStore cloud;   // row f-4: device-resident LiDAR buffer
    PinBuf<float4> h_stage;     // pinned upload staging (doubling from 4096 points: ensure_stage)
    PinBuf<MotionState> h_states_ring;      // pinned: the motion states of lv_scan_deskew_window, 8 slots of 64 (a copy out of the
    int states_slot = 0;                    // caller's pageable memory blocks the host; every cycle synchronises at least once, so
                                            // a slot is free again long before its turn comes round)

    ResidentFilter filter;   // x, P resident between lv_filter_set / lv_predict / lv_correct / lv_filter_get (lv_filter.hpp)
    DevBuf<lv_observe_result> d_obs;      // lv_observe: the records of the last call (LV_OBSERVE_BATCH), and how many
    int n_obs = 0;
    RankExchange ranks;   // multi-GPU: how the partials of every pass reach every rank (lv_exchange.hpp)
    UpdateDriver upd{prm, filter, ranks};   // the iterated update: kf, the mailbox, its buffers, routes and profiling (lv_update.hpp)
};

namespace {

// LV_SLOW_CALL_MS=<ms> in the environment: every entry point that lasted longer than that reports itself on stderr (a
// diagnostic for latency hiccups: which call of a cycle stalled, profiles/experiments_r05/async_rebuild.txt)
struct SlowCall {
    const char* name;
    std::chrono::steady_clock::time_point t0;
    static double limit_ms() { static const double v = [] { const char* e = getenv("LV_SLOW_CALL_MS"); return e ? atof(e) : 0.0; }(); return v; }
    explicit SlowCall(const char* n) : name(n) { if (limit_ms() > 0.0) t0 = std::chrono::steady_clock::now(); }
    ~SlowCall() {
        if (limit_ms() > 0.0) {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms > limit_ms()) fprintf(stderr, "[limovelo_hip] slow call: %s took %.3f ms\n", name, ms);
        }
    }
};
#define LV_CHECK_CTX(ctx)                        \
    SlowCall _slow_call(__func__);               \
    do {                                         \
        if (!(ctx)) {                            \
            set_error("null context");           \
            return LV_EINVAL;                    \
        }                                        \
        hipError_t _e = hipSetDevice((ctx)->device); \
        if (_e != hipSuccess) {                  \
            set_error("hipSetDevice(%d): %s", (ctx)->device, hipGetErrorString(_e)); \
            return LV_EHIP;                      \
        }                                        \
    } while (0)

// an incremental insert leaves its outcome in flight (MapStore::settle): pick it up before the map's bookkeeping is used.  Only
// for the calls that settle WITHOUT polling the background rebuild (lv_maptools.hpp lists them); every other call: map_side(c).ready()
#define LV_SETTLE_MAP(c)                               \
    do {                                               \
        int _rs = (c)->map.settle((c)->stream);        \
        if (_rs) return _rs;                           \
    } while (0)

int ensure_stage(lv_ctx* c, size_t n) {
    if (n <= c->h_stage.cap) return LV_OK;
    // a copy out of the old buffer may still be pending on the (possibly caller-supplied, non-blocking) stream
    LV_HIP(hipStreamSynchronize(c->stream));
    return c->h_stage.need_pow2(n, 4096);
}

inline void read_xyz(const void* base, size_t stride, size_t i, float& x, float& y, float& z) {
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + i * stride);
    x = p[0]; y = p[1]; z = p[2];
}

// what the update driver works on (lv_update.hpp): the context's stream, the map's view and the current scan
UpdateInputs inputs(const lv_ctx* c) {
    return {c->stream, &c->map.view, c->scan.d_sorted, c->scan.n, c->scan.d_tile_order, c->scan.n_tiles, c->scan.tile_points};
}

// a new scan is on its way: nothing captured, handed over or told about the one before holds any longer
void new_scan(lv_ctx* c) {
    c->upd.new_scan();
    c->scan.n = 0, c->scan.route = LV_SCAN_ROUTE_NONE;   // (until a chain says what produced it)
    c->ranks.shard_max = 0;               // (the caller tells its largest shard again)
}

enum class StageW { Zero, Index };
// repack n caller points into the pinned staging buffer (float4; w = 0 or the point's index as bits), optionally keeping the
// smallest coordinates seen in bmin and each point's f64 time stamp (time_offset bytes into it) in times.  The caller has made
// room (ensure_stage) and synchronised the stream since the last use.
void stage_points(lv_ctx* c, const void* points, size_t stride, size_t n, StageW w_rule, float* bmin = nullptr, double* times = nullptr,
                  size_t time_offset = 0) {
    for (size_t i = 0; i < n; ++i) {
        float x, y, z, w = 0.f;
        read_xyz(points, stride, i, x, y, z);
        if (w_rule == StageW::Index) {
            const uint32_t ui = (uint32_t)i;
            std::memcpy(&w, &ui, 4);
        }
        c->h_stage[i] = make_float4(x, y, z, w);
        if (times) std::memcpy(&times[i], reinterpret_cast<const char*>(points) + i * stride + time_offset, sizeof(double));
        if (bmin) bmin[0] = x < bmin[0] ? x : bmin[0], bmin[1] = y < bmin[1] ? y : bmin[1], bmin[2] = z < bmin[2] ? z : bmin[2];
    }
}

// lv_create, once the context exists: the knobs out of the environment, then streams, events and buffers
int create_in(lv_ctx* c) {
    c->scan.tile_points = 256u / (uint32_t)c->prm.lanes_per_query;
    c->map.cell = c->prm.voxel_size;
    hipDeviceProp_t prop;
    LV_HIP(hipGetDeviceProperties(&prop, c->device));
    LV_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    LV_HIP(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    c->rebuild.create_streams(c->device, /*quiet=*/true);   // (a failure is retried by the first background rebuild)
    LV_HIP(hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming));
    if (int rk = Knobs<lv_ctx>::read_environment(*c)) return rk;
    if (int ru = c->upd.alloc(prop.multiProcessorCount)) return ru;
    if (int rf = c->filter.alloc()) return rf;
    LV_TRY(c->h_states_ring.need(8 * 64));
    LV_TRY(c->d_obs.need(LV_OBSERVE_BATCH));
    LV_HIP(hipMemset(c->d_obs, 0, LV_OBSERVE_BATCH * sizeof(lv_observe_result)));
    return LV_OK;
}

}  // namespace

extern "C" {

void lv_default_params(lv_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->MAX_NUM_ITERS = 3;           // config/params.yaml:46
    p->NUM_MATCH_POINTS = 5;        // :48
    p->MAX_DIST_PLANE = 2.0;        // :49
    p->PLANES_THRESHOLD = 5.e-2f;   // :50
    p->estimate_extrinsics = 0;     // :13
    p->LiDAR_noise = 0.001;         // :32
    for (int i = 0; i < LV_STATE_DOF; ++i) p->LIMITS[i] = 0.001;  // src/main.cpp:145
    p->degeneracy_threshold = 5.0;  // :52 (applied by degeneracy_mode 2 only)
    p->degeneracy_mode = 0;
    p->print_degeneracy_values = 0; // :53
    p->voxel_size = 0.5f;
    p->lanes_per_query = 8;
}

const char* lv_last_error(void) { return lv::g_err; }
const char* lv_version(void) { return "limovelo_hip 0.1 (gfx950)"; }

int lv_create(const lv_params* params, int device, lv_ctx** out) {
    if (!params || !out) { set_error("null argument"); return LV_EINVAL; }
    *out = nullptr;
    if (params->NUM_MATCH_POINTS < KNN_MIN || params->NUM_MATCH_POINTS > KNN_MAX) {
        set_error("NUM_MATCH_POINTS=%d unsupported (%d..%d)", params->NUM_MATCH_POINTS, KNN_MIN, KNN_MAX);
        return LV_EINVAL;
    }
    if (params->NUM_MATCH_POINTS != KNN && params->lanes_per_query != 8) {
        set_error("NUM_MATCH_POINTS=%d runs the general build: lanes_per_query must be 8", params->NUM_MATCH_POINTS);
        return LV_EINVAL;
    }
    if (params->MAX_NUM_ITERS < 0 || params->MAX_NUM_ITERS + 1 > MAX_PASSES) { set_error("MAX_NUM_ITERS out of range"); return LV_EINVAL; }
    if (!(params->voxel_size > 0.f)) { set_error("voxel_size must be > 0"); return LV_EINVAL; }
    const int S = params->lanes_per_query;
    if (!(S == 1 || S == 2 || S == 4 || S == 8 || S == 16)) { set_error("lanes_per_query must be 1,2,4,8,16"); return LV_EINVAL; }
    if (params->degeneracy_mode < 0 || params->degeneracy_mode > 2) { set_error("degeneracy_mode must be 0, 1 or 2"); return LV_EINVAL; }
    if (params->degeneracy_mode == 0 && params->degeneracy_threshold != 5.0) {
        static bool warned = false;
        if (!warned) {
            warned = true;
            fprintf(stderr, "limovelo_hip: degeneracy_threshold = %g is set but has no effect: the degeneracy stage of the fork's "
                            "update_iterated_dyn_share_modified is not part of the reference mount; degeneracy_mode = 2 enables a "
                            "documented restatement, degeneracy_mode = 1 reports the eigenvalues (include/limovelo_hip.h)\n",
                    params->degeneracy_threshold);
        }
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { set_error("no HIP device available (%s)", hipGetErrorString(e)); return LV_ENODEV; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return LV_EINVAL; }
    LV_HIP(hipSetDevice(device));
    lv_ctx* c = new (std::nothrow) lv_ctx();
    if (!c) { set_error("out of host memory"); return LV_EINVAL; }
    c->prm = *params;
    c->device = device;
    if (int rc = create_in(c)) {   // (what was created so far goes; *out stays null)
        lv_destroy(c);
        return rc;
    }
    *out = c;
    return LV_OK;
}

// the context's streams as the background map rebuild takes them (lv_rebuild.hpp)
static CtxStreams ctx_streams(lv_ctx* c) {
    return {c->stream, c->side_stream, c->ev_staged, c->overlap_insert && c->side_stream && c->stream == c->own_stream};
}
// ... and what a call that reads or edits the map sees of the context (lv_maptools.hpp): ready() is "settle the insert in flight,
// then adopt or drop a finished background rebuild"
static MapSide<MapRebuild<MapStore>> map_side(lv_ctx* c) { return {c->map, c->rebuild, ctx_streams(c), c->stream}; }

void lv_destroy(lv_ctx* c) {   // (also of a context lv_create gave up on part of the way: everything here takes what is not there)
    if (!c) return;
    hipSetDevice(c->device);
    c->cloud.release();
    c->ranks.release_comm(c->stream);
    c->rebuild.release(c->map, ctx_streams(c));   // (joins its worker and waits for the device before anything is freed)
    c->map.release();
    c->tools.release();
    c->place.release();
    c->graph.release();
    c->traj.release();
    c->ndt.release();
    c->mclf.release();
    c->elev.release();
    c->vol.release();
    c->batch.release();
    c->scan.release();
    c->h_stage.release();
    c->filter.release();
    c->d_obs.release();
    c->h_states_ring.release();
    c->ranks.release();
    c->upd.release();
    if (c->side_stream) { hipStreamSynchronize(c->side_stream); hipStreamDestroy(c->side_stream); }
    if (c->ev_staged) hipEventDestroy(c->ev_staged);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

int lv_set_stream(lv_ctx* c, void* hip_stream) {
    LV_CHECK_CTX(c);
    if (int rp = c->filter.flush(c->stream, c->upd.d_kf)) return rp;
    // whatever is still tied to the OLD stream is settled on it: a remembered Buffer::clear (CloudStore keeps the stream it was
    // issued on: the caller may destroy that stream after this call) and the outcome of an incremental map insert
    { int rs = c->cloud.settle(); if (rs) return rs; }
    LV_SETTLE_MAP(c);
    LV_HIP(hipStreamSynchronize(c->stream));
    if (c->side_stream) LV_HIP(hipStreamSynchronize(c->side_stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return LV_OK;
}
void* lv_get_stream(lv_ctx* c) { return c ? (void*)c->stream : nullptr; }
int lv_synchronize(lv_ctx* c) {
    LV_CHECK_CTX(c);
    if (int rp = c->filter.flush(c->stream, c->upd.d_kf)) return rp;
    LV_HIP(hipStreamSynchronize(c->stream));
    if (c->side_stream) LV_HIP(hipStreamSynchronize(c->side_stream));
    return LV_OK;
}

// repack caller points into the pinned staging buffer (float4) and upload them to `dst` (device)
static int stage_map_points(lv_ctx* c, const void* points, size_t stride, size_t n, float4* dst) {
    if (int rc = ensure_stage(c, n)) return rc;
    LV_HIP(hipStreamSynchronize(c->stream));  // staging buffer reuse
    stage_points(c, points, stride, n, StageW::Zero);
    if (n) LV_HIP(hipMemcpyAsync(dst, c->h_stage, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return LV_OK;
}

static int check_map_points(const void* points, size_t stride, size_t n) {
    if (n && (!points || stride < 12)) { set_error("bad point array (stride %zu)", stride); return LV_EINVAL; }
    if (n > 0xFFFFFFF0ull) { set_error("map too large"); return LV_EINVAL; }
    for (size_t i = 0; i < n; ++i) {
        float x, y, z;
        read_xyz(points, stride, i, x, y, z);
        if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) { set_error("non-finite map point at %zu", i); return LV_EINVAL; }
    }
    return LV_OK;
}

// the stream an incremental insert runs on: the context's side stream, ordered behind what the context's stream holds so far
// (the staged points), whenever the overlap applies (see lv_map_add_scan); the context's stream otherwise
static hipStream_t insert_stream(lv_ctx* c) {
    return c->map.built && c->map.m > 0 ? ctx_streams(c).side_behind() : c->stream;
}

int lv_map_build(lv_ctx* c, const void* points, size_t stride, size_t n) {
    LV_CHECK_CTX(c);
    c->rebuild.cancel(c->map, ctx_streams(c));
    LV_SETTLE_MAP(c);
    int rc = check_map_points(points, stride, n);   // bad input leaves the previous map untouched
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(c->stream));
    c->map.n_ids = 0;
    c->map.m = 0;
    c->map.built = false;
    c->map.refresh_view();
    rc = c->map.reserve(n);
    if (rc) return rc;
    rc = stage_map_points(c, points, stride, n, c->map.d_orig);
    if (rc) return rc;
    c->map.n_ids = (uint32_t)n;
    c->map.origin_set = false;
    c->map.cell = c->prm.voxel_size;
    return c->map.rebuild(c->stream);
}

int lv_map_add(lv_ctx* c, const void* points, size_t stride, size_t n, int downsample) {
    LV_CHECK_CTX(c);
    if (int rr = map_side(c).ready()) return rr;
    if (n == 0) return LV_OK;
    int rc = check_map_points(points, stride, n);
    if (rc) return rc;
    if ((uint64_t)c->map.n_ids + n > 0xFFFFFFF0ull) { set_error("map too large"); return LV_EINVAL; }
    rc = c->rebuild.maybe_start(c->map, n);
    if (rc) return rc;
    rc = c->map.reserve_batch(n);
    if (rc) return rc;
    rc = stage_map_points(c, points, stride, n, c->map.d_new);
    if (rc) return rc;
    rc = c->rebuild.journal_add(c->map, ctx_streams(c), (uint32_t)n, downsample, 0.2f, false);
    if (rc) return rc;
    hipStream_t is = insert_stream(c);
    rc = c->rebuild.order(ctx_streams(c), is);
    if (rc) return rc;
    return c->map.add_staged(is, (uint32_t)n, downsample, 0.2f, false);  // box_length of KD_TREE(0.3, 0.6, 0.2), Mapper.cpp:65
}

namespace {
// `Xt2 * Xt2.I_Rt_L() * p` (src/main.cpp:92; State.cpp:51-62,83-85; RotTransl.cpp:36-48) for every point of the
// current scan, in scan order, with the state taken from the device (the resident filter or the last update)
__global__ void scan_to_world_kernel(const double* __restrict__ x, const float4* __restrict__ scan, uint32_t n, float4* __restrict__ out) {
    __shared__ PoseConsts s_pc;
    if (threadIdx.x == 0) compute_pose_consts(x, &s_pc);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = scan[i];
    float4 o;
    rt_apply(s_pc.Tc, p.x, p.y, p.z, o.x, o.y, o.z);
    o.w = 0.f;
    out[i] = o;
}
}  // namespace

int lv_map_add_scan(lv_ctx* c, int downsample) {
    LV_CHECK_CTX(c);
    if (int rr = map_side(c).ready()) return rr;
    const uint32_t n = c->scan.n;
    if (n == 0) return LV_OK;   // Mapper::add returns on an empty cloud (Mapper.cpp:20)
    if (int rp = c->filter.flush(c->stream, c->upd.d_kf)) return rp;
    int rc = c->rebuild.maybe_start(c->map, n);
    if (rc) return rc;
    rc = c->map.reserve_batch(n);
    if (rc) return rc;
    if (int ru = c->filter.upload(c->stream)) return ru;
    const double* x = c->filter.scan_x(c->upd.d_kf);
    hipLaunchKernelGGL(scan_to_world_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, x, c->scan.d_raw, n, c->map.d_new);
    LV_HIP(hipGetLastError());
    // The insert depends on nothing but the world points just staged, and nothing depends on it until the next search: it runs
    // on the context's SIDE stream, beside whatever the caller enqueues next (in the reference's loop, src/main.cpp:52-128: the
    // next cycle's IMU propagation, LiDAR window, de-skew and voxel grid — ~100 us of small launches while the insert's chain
    // of ~150 us occupies a handful of CUs).  Everything that touches the map settles the insert first (MapSide::ready, LV_SETTLE_MAP: the
    // host waits for the note the chain's last kernel posts), so no other ordering is needed.  Only with the context's own
    // stream: a caller-provided stream keeps everything on that stream.
    rc = c->rebuild.journal_add(c->map, ctx_streams(c), n, downsample, 0.2f, true);
    if (rc) return rc;
    hipStream_t is = insert_stream(c);
    rc = c->rebuild.order(ctx_streams(c), is);
    if (rc) return rc;
    return c->map.add_staged(is, n, downsample, 0.2f, true);   // Mapper::add: an empty map is built from the cloud
}

int lv_map_evict_box(lv_ctx* c, const float lo[3], const float hi[3], int keep_inside, size_t* n_evicted) {
    LV_CHECK_CTX(c);
    if (!lo || !hi) { set_error("null argument"); return LV_EINVAL; }
    uint32_t ne = 0;
    if (int rr = map_side(c).ready()) return rr;
    int rc = c->rebuild.journal_evict(c->map, ctx_streams(c), 2, lo, hi, keep_inside, 0);
    if (!rc) rc = c->rebuild.order(ctx_streams(c), c->stream);
    if (!rc) rc = c->map.evict_box(c->stream, lo, hi, keep_inside, &ne);
    if (n_evicted) *n_evicted = ne;
    return rc;
}

int lv_map_evict_oldest(lv_ctx* c, size_t n_oldest, size_t* n_evicted) {
    LV_CHECK_CTX(c);
    uint32_t ne = 0;
    if (int rr = map_side(c).ready()) return rr;
    int rc = c->rebuild.journal_evict(c->map, ctx_streams(c), 3, nullptr, nullptr, 0, (uint32_t)(n_oldest > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : n_oldest));
    if (!rc) rc = c->rebuild.order(ctx_streams(c), c->stream);
    if (!rc) rc = c->map.evict_oldest(c->stream, (uint32_t)(n_oldest > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : n_oldest), &ne);
    if (n_evicted) *n_evicted = ne;
    return rc;
}

void lv_default_visibility_params(lv_visibility_params* p) { default_visibility_params(p); }

// ---- The tools on the point map (lv_maptools.hpp: what each call asks for and in which order, and what a removal does to the
// background rebuild).  An entry point checks the context and makes one call into c->tools.
int lv_map_remove_dynamic(lv_ctx* c, const lv_view* views, size_t n_views, const lv_visibility_params* p, uint8_t* hits, size_t* n_removed) {
    LV_CHECK_CTX(c);
    return c->tools.remove_dynamic(map_side(c), views, n_views, p, hits, n_removed);
}

void lv_default_surface_params(lv_surface_params* p) { default_surface_params(p); }
void lv_default_outlier_params(lv_outlier_params* p) { default_outlier_params(p); }

int lv_map_normals(lv_ctx* c, const lv_surface_params* p, float* normals, float* curvature, float* mean_dist, int32_t* n_used, size_t capacity) {
    LV_CHECK_CTX(c);
    return c->tools.normals(map_side(c), p, normals, curvature, mean_dist, n_used, capacity);
}

int lv_map_remove_outliers(lv_ctx* c, const lv_outlier_params* p, uint8_t* flags, size_t* n_removed, double* stats) {
    LV_CHECK_CTX(c);
    return c->tools.remove_outliers(map_side(c), p, flags, n_removed, stats);
}

void lv_default_cluster_params(lv_cluster_params* p) { default_cluster_params(p); }

int lv_map_cluster(lv_ctx* c, const lv_cluster_params* p, const uint8_t* mask, int32_t* labels, size_t capacity, uint32_t* sizes,
                   size_t sizes_capacity, size_t* n_clusters) {
    LV_CHECK_CTX(c);
    return c->tools.cluster_map(map_side(c), p, mask, labels, capacity, sizes, sizes_capacity, n_clusters);
}

int lv_map_remove_clusters(lv_ctx* c, const lv_cluster_params* p, const uint8_t* mask, const uint8_t* seeds, uint8_t* flags, size_t* n_removed) {
    LV_CHECK_CTX(c);
    return c->tools.remove_clusters(map_side(c), p, mask, seeds, flags, n_removed);
}

void lv_default_plane_params(lv_plane_params* p) { default_plane_params(p); }

int lv_map_planes(lv_ctx* c, const lv_plane_params* p, const uint8_t* mask, int32_t* labels, size_t capacity, lv_plane* planes,
                  size_t planes_capacity, size_t* n_planes) {
    LV_CHECK_CTX(c);
    return c->tools.extract_planes(map_side(c), p, mask, labels, capacity, planes, planes_capacity, n_planes);
}

void lv_default_paint_params(lv_paint_params* p) { default_paint_params(p); }

int lv_map_paint(lv_ctx* c, const lv_camera_view* views, size_t n_views, const lv_paint_params* p, float* rgb, float* depth, uint8_t* n_seen) {
    LV_CHECK_CTX(c);
    return c->tools.paint_map(map_side(c), views, n_views, p, rgb, depth, n_seen);
}

// ---- Place recognition (lv_place.hip)
void lv_default_place_params(lv_place_params* p) { default_place_params(p); }

int lv_place_configure(lv_ctx* c, const lv_place_params* p) {
    LV_CHECK_CTX(c);
    int rc = place_params_ok(p);
    if (rc) return rc;
    c->place.prm = *p;
    c->place.clear();
    return LV_OK;
}

// the current scan's descriptor at state x into the store's query buffer
static int place_describe_scan(lv_ctx* c, const lv_state* x, PlaceFrame* f, double centre[3]) {
    int rc = place_state_ok(x);
    if (rc) return rc;
    if (c->scan.n == 0) { set_error("no scan: call lv_scan_set first"); return LV_ESTATE; }
    place_frame(*x, f, centre);
    rc = c->place.reserve(c->stream, c->place.n);
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(c->place.d_q, 0, (size_t)c->place.bins() * sizeof(uint32_t), c->stream));
    return c->place.describe(c->scan, c->stream, *f, c->place.d_q);
}

int lv_place_describe(lv_ctx* c, const lv_state* x, float* desc) {
    LV_CHECK_CTX(c);
    if (!desc) { set_error("null argument"); return LV_EINVAL; }
    PlaceFrame f;
    double centre[3];
    int rc = place_describe_scan(c, x, &f, centre);
    if (rc) return rc;
    LV_HIP(hipMemcpyAsync(desc, c->place.d_q, (size_t)c->place.bins() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    LV_HIP(hipStreamSynchronize(c->stream));
    return LV_OK;
}

int lv_place_add_scan(lv_ctx* c, const lv_state* x, uint32_t* id) {
    LV_CHECK_CTX(c);
    int rc = place_state_ok(x);
    if (rc) return rc;
    if (c->scan.n == 0) { set_error("no scan: call lv_scan_set first"); return LV_ESTATE; }
    if (c->place.n + 1 > PLACE_MAX_COUNT) { set_error("the place database holds 2^20 places"); return LV_ERANGE; }
    PlaceFrame f;
    double centre[3];
    place_frame(*x, &f, centre);
    return c->place.add_scan(c->scan, c->stream, f, centre, id);
}

// read-only on the map and ordered like the map tools (lv_maptools.hpp "the map source")
int lv_place_add_map(lv_ctx* c, const double* centres, size_t n, uint32_t* first_id) {
    LV_CHECK_CTX(c);
    if (!centres) { set_error("null argument"); return LV_EINVAL; }
    if (n < 1 || n > PLACE_MAX_MAP_CENTRES) { set_error("n = %zu: must be in 1..%zu", n, PLACE_MAX_MAP_CENTRES); return LV_EINVAL; }
    if (int rc = place_centres_ok(centres, n)) return rc;
    if (c->place.n + n > PLACE_MAX_COUNT) { set_error("the place database holds 2^20 places"); return LV_ERANGE; }
    if (int rr = map_side(c).ready()) return rr;
    return c->place.add_map(c->map, c->stream, centres, n, first_id);
}

int lv_place_query(lv_ctx* c, const lv_state* x, int k, uint32_t* ids, int32_t* shifts, float* dist, size_t* n_out) {
    LV_CHECK_CTX(c);
    if (k < 1 || k > PLACE_MAX_K) { set_error("k = %d: must be in 1..%d", k, PLACE_MAX_K); return LV_EINVAL; }
    int rc = place_state_ok(x);
    if (rc) return rc;
    if (c->place.n == 0) { set_error("the place database is empty"); return LV_ESTATE; }
    PlaceFrame f;
    double centre[3];
    rc = place_describe_scan(c, x, &f, centre);
    if (rc) return rc;
    const int kk = (size_t)k < c->place.n ? k : (int)c->place.n;
    rc = c->place.query(c->stream, kk, ids, shifts, dist);
    if (rc) return rc;
    if (n_out) *n_out = (size_t)kk;
    return LV_OK;
}

size_t lv_place_count(lv_ctx* c) { return c ? c->place.n : 0; }

int lv_place_clear(lv_ctx* c) {
    LV_CHECK_CTX(c);
    c->place.clear();
    return LV_OK;
}

int lv_place_fetch(lv_ctx* c, float* desc, double* centres, size_t capacity) {
    LV_CHECK_CTX(c);
    if (capacity < c->place.n) { set_error("capacity %zu < %zu places", capacity, c->place.n); return LV_EINVAL; }
    return c->place.fetch(c->stream, desc, centres);
}

int lv_place_load(lv_ctx* c, const float* desc, const double* centres, size_t n) {
    LV_CHECK_CTX(c);
    if (n == 0) return LV_OK;
    if (!desc || !centres) { set_error("null argument"); return LV_EINVAL; }
    const size_t nb = n * (size_t)c->place.bins();
    for (size_t i = 0; i < nb; ++i)
        if (!(std::isfinite(desc[i]) && desc[i] >= 0.f)) { set_error("descriptor value %zu: must be finite and >= 0", i); return LV_EINVAL; }
    if (int rc = place_centres_ok(centres, n)) return rc;
    if (c->place.n + n > PLACE_MAX_COUNT) { set_error("the place database holds 2^20 places"); return LV_ERANGE; }
    return c->place.load(c->stream, desc, centres, n);
}

// ---- Pose graph (lv_graph.hip)
void lv_default_graph_params(lv_graph_params* p) { default_graph_params(p); }

#define LV_GRAPH_SET(c) LV_REQUIRE((c)->graph.set, LV_ESTATE, "no pose graph: call lv_graph_set first")

int lv_graph_set(lv_ctx* c, const lv_graph_pose* poses, size_t n, const uint8_t* fixed, const lv_graph_edge* edges, size_t n_edges,
                 const lv_graph_prior* priors, size_t n_priors) {
    if (int rc = graph_check(poses, n, fixed, edges, n_edges, priors, n_priors)) return rc;   // (before the context: "null context" comes last)
    LV_CHECK_CTX(c);
    return c->graph.assign(c->stream, poses, n, fixed, edges, n_edges, priors, n_priors);
}

int lv_graph_optimise(lv_ctx* c, const lv_graph_params* params, lv_graph_info* info) {
    lv_graph_params prm;
    default_graph_params(&prm);
    if (params) prm = *params;
    if (int rc = graph_params_ok(&prm)) return rc;
    LV_CHECK_CTX(c);
    LV_GRAPH_SET(c);
    const int rc = c->graph.optimise(c->stream, prm);
    if (!rc && info) *info = c->graph.info;
    return rc;
}

int lv_graph_fetch(lv_ctx* c, lv_graph_pose* poses, size_t capacity) {
    if (!poses) { set_error("null poses"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_GRAPH_SET(c);
    if (capacity < c->graph.n) { set_error("capacity %zu < %zu nodes", capacity, c->graph.n); return LV_EINVAL; }
    return c->graph.fetch(c->stream, poses);
}

int lv_graph_chi2(lv_ctx* c, double* edge_s, double* prior_s) {
    LV_CHECK_CTX(c);
    LV_GRAPH_SET(c);
    return c->graph.chi2(c->stream, edge_s, prior_s);
}

int lv_graph_warp_points(lv_ctx* c, const void* pts, size_t stride, const uint32_t* keys, size_t n, float* out) {
    if (n > GRAPH_MAX_WARP) { set_error("n = %zu above 2^28", n); return LV_EINVAL; }
    if (n && (!pts || !keys || !out)) { set_error("null argument"); return LV_EINVAL; }
    if (n && stride < 12) { set_error("stride %zu below 12", stride); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_GRAPH_SET(c);
    for (size_t k = 0; k < n; ++k)
        if (keys[k] >= c->graph.n) { set_error("key %zu = %u: the graph holds %zu nodes", k, keys[k], c->graph.n); return LV_EINVAL; }
    return c->graph.warp(c->stream, pts, stride, keys, n, out);
}

int lv_graph_get_info(lv_ctx* c, lv_graph_info* info) {
    if (!info) { set_error("null info"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    *info = c->graph.info;
    if (!c->graph.set) info->status = -1;
    return LV_OK;
}

int lv_graph_clear(lv_ctx* c) {
    LV_CHECK_CTX(c);
    LV_GRAPH_SET(c);
    c->graph.clear();
    return LV_OK;
}

// ---- Trajectory (lv_traj.hip)
void lv_default_traj_smooth_params(lv_traj_smooth_params* p) { default_traj_smooth_params(p); }
void lv_default_traj_register_params(lv_traj_register_params* p) { default_traj_register_params(p); }

#define LV_TRAJ_SET(c) LV_REQUIRE((c)->traj.set, LV_ESTATE, "no trajectory: call lv_traj_set first")

int lv_traj_set(lv_ctx* c, const lv_traj_knot* knots, size_t n) {
    if (int rc = traj_check(knots, n, "trajectory")) return rc;   // (before the context: "null context" comes last)
    LV_CHECK_CTX(c);
    return c->traj.assign(c->stream, knots, n);
}

int lv_traj_fetch(lv_ctx* c, lv_traj_knot* knots, size_t capacity) {
    if (!knots) { set_error("null knots"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_TRAJ_SET(c);
    if (capacity < c->traj.n) { set_error("capacity %zu < %zu knots", capacity, c->traj.n); return LV_EINVAL; }
    return c->traj.fetch(c->stream, knots);
}

int lv_traj_get_info(lv_ctx* c, lv_traj_info* info) {
    if (!info) { set_error("null info"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    *info = c->traj.info;
    return LV_OK;
}

int lv_traj_clear(lv_ctx* c) {
    LV_CHECK_CTX(c);
    LV_TRAJ_SET(c);
    c->traj.clear();
    return LV_OK;
}

int lv_traj_sample(lv_ctx* c, const double* times, size_t n, int extrapolate, lv_graph_pose* out, uint8_t* status) {
    if (n > TRAJ_MAX_ITEMS) { set_error("trajectory sample: n = %zu above 2^28", n); return LV_EINVAL; }
    if (n && !times) { set_error("trajectory sample: null times"); return LV_EINVAL; }
    if (int rc = traj_extrapolate_ok(extrapolate)) return rc;
    LV_CHECK_CTX(c);
    LV_TRAJ_SET(c);
    return c->traj.sample(c->stream, times, n, extrapolate, out, status);
}

int lv_traj_smooth(lv_ctx* c, const lv_traj_smooth_params* params, const uint8_t* fixed) {
    if (int rc = traj_smooth_params_ok(params)) return rc;
    LV_CHECK_CTX(c);
    LV_TRAJ_SET(c);
    return c->traj.smooth(c->stream, *params, fixed);
}

int lv_traj_correct(lv_ctx* c, const lv_traj_knot* corr, size_t m) {
    if (int rc = traj_check(corr, m, "correction")) return rc;
    LV_CHECK_CTX(c);
    LV_TRAJ_SET(c);
    return c->traj.correct(c->stream, corr, m);
}

int lv_traj_register(lv_ctx* c, const lv_traj_register_params* params, const void* pts, size_t stride, size_t time_offset, size_t n, float* out,
                     uint8_t* status, uint64_t stats[4]) {
    lv_traj_register_params prm;
    default_traj_register_params(&prm);
    if (params) prm = *params;
    if (int rc = traj_register_params_ok(&prm)) return rc;
    if (int rc = traj_register_layout_ok(pts, stride, time_offset, n)) return rc;
    LV_CHECK_CTX(c);
    LV_TRAJ_SET(c);
    if (prm.frame == LV_TRAJ_FRAME_AT)
        if (int rc = traj_frame_time_ok(prm.frame_time, c->traj.info.t_first, c->traj.info.t_last)) return rc;
    return c->traj.register_host(c->stream, prm, pts, stride, time_offset, n, out, status, stats);
}

int lv_traj_register_cloud(lv_ctx* c, const lv_traj_register_params* params, double t1, double t2, float* out, uint8_t* status, size_t capacity,
                           size_t* n, uint64_t stats[4]) {
    lv_traj_register_params prm;
    default_traj_register_params(&prm);
    if (params) prm = *params;
    if (int rc = traj_register_params_ok(&prm)) return rc;
    if (!n) { set_error("trajectory register: null n"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    *n = 0;
    LV_TRAJ_SET(c);
    if (prm.frame == LV_TRAJ_FRAME_AT)
        if (int rc = traj_frame_time_ok(prm.frame_time, c->traj.info.t_first, c->traj.info.t_last)) return rc;
    uint32_t lo = 0, hi = 0;
    if (int rc = c->cloud.window(c->stream, t1, t2, &lo, &hi)) return rc;   // (what lv_cloud_fetch cuts)
    const size_t cnt = hi - lo;
    *n = cnt;
    if (!out) return LV_OK;
    if (capacity < cnt) { set_error("capacity %zu too small for %zu points", capacity, cnt); return LV_EINVAL; }
    const CloudPoint* first = c->cloud.d_buf + lo;
    const TrajPoints in{&first->x, &first->time, (uint32_t)(sizeof(CloudPoint) / sizeof(float)), (uint32_t)(sizeof(CloudPoint) / sizeof(double))};
    return c->traj.register_device(c->stream, prm, in, cnt, out, status, stats);
}

int lv_map_relinearise(lv_ctx* c) {
    LV_CHECK_CTX(c);
    c->rebuild.cancel(c->map, ctx_streams(c));   // (a background rebuild in flight is superseded by this synchronous one)
    LV_SETTLE_MAP(c);
    if (!c->map.built) return LV_OK;
    return c->map.relinearise(c->stream);
}

int lv_map_relinearise_async(lv_ctx* c) {
    LV_CHECK_CTX(c);
    if (int rr = map_side(c).ready()) return rr;
    if (!c->map.built || c->map.m == 0) return LV_OK;
    return c->rebuild.start(c->map);
}

// every allocation a background rebuild needs, made at set-up time (MapRebuild::reserve)
int lv_map_reserve_rebuild(lv_ctx* c) {
    LV_CHECK_CTX(c);
    if (int rr = map_side(c).ready()) return rr;
    return c->rebuild.reserve(c->map, ctx_streams(c));
}

int lv_map_rebuild_status(lv_ctx* c, int wait, uint64_t out[4]) {
    LV_CHECK_CTX(c);
    return c->rebuild.status(c->map, ctx_streams(c), wait, out);
}

int lv_map_get_stats(lv_ctx* c, lv_map_stats* out) {
    LV_CHECK_CTX(c);
    if (int rr = map_side(c).ready()) return rr;
    if (!out) { set_error("null argument"); return LV_EINVAL; }
    static_assert(sizeof(lv_map_stats) == sizeof(MapStats), "lv_map_stats layout");
    MapStats st;
    if (c->map.h_cnt && c->map.d_cnt && c->map.built) {   // (the pools' cursors live on the device: fetch them for the statistics)
        LV_HIP(hipMemcpyAsync(c->map.h_cnt, c->map.d_cnt, BUCKET_LEVELS * sizeof(MapCounters), hipMemcpyDeviceToHost, c->stream));
        LV_HIP(hipStreamSynchronize(c->stream));
    }
    c->map.stats(&st);
    std::memcpy(out, &st, sizeof(st));
    return LV_OK;
}

size_t lv_map_size(lv_ctx* c) {
    if (!c) return 0;
    c->map.settle(c->stream);
    c->rebuild.poll(c->map, ctx_streams(c));
    return c->map.m;
}

// the living points in map order (ids ascending): the index space of lv_fetch_knn
int lv_map_fetch(lv_ctx* c, float* xyz_out, size_t capacity) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    const size_t m = c->map.m, ids = c->map.n_ids;
    if (capacity < m || (!xyz_out && capacity)) { set_error("capacity too small"); return LV_EINVAL; }
    if (m == 0) return LV_OK;
    std::vector<float4> tmp(ids);
    LV_HIP(hipStreamSynchronize(c->stream));
    LV_HIP(hipMemcpy(tmp.data(), c->map.d_orig, ids * sizeof(float4), hipMemcpyDeviceToHost));
    size_t o = 0;
    for (size_t i = 0; i < ids && o < m; ++i) {
        if (!std::isfinite(tmp[i].x)) continue;
        xyz_out[3 * o] = tmp[i].x; xyz_out[3 * o + 1] = tmp[i].y; xyz_out[3 * o + 2] = tmp[i].z;
        ++o;
    }
    if (o != m) { set_error("map bookkeeping: %zu living points found, %zu expected", o, m); return LV_ESTATE; }
    return LV_OK;
}

// Map queries (lv_query.hip): ordered behind every earlier map mutation like the tools above, they read the active store
int lv_map_knn(lv_ctx* c, const void* q, size_t stride, size_t n, int k, float max_dist, uint32_t* idx, float* d2, int32_t* found) {
    LV_CHECK_CTX(c);
    return c->tools.knn(map_side(c), q, stride, n, k, max_dist, idx, d2, found);
}

int lv_map_radius_search(lv_ctx* c, const void* q, size_t stride, size_t n, float radius, size_t* offsets, uint32_t* idx, float* d2,
                         size_t capacity, size_t* total) {
    LV_CHECK_CTX(c);
    return c->tools.radius_search(map_side(c), q, stride, n, radius, offsets, idx, d2, capacity, total);
}

int lv_map_box_search(lv_ctx* c, const float lo[3], const float hi[3], uint32_t* idx, float* xyz, size_t capacity, size_t* n_out) {
    LV_CHECK_CTX(c);
    return c->tools.box_search(map_side(c), lo, hi, idx, xyz, capacity, n_out);
}

// Multi-hypothesis passes / updates (lv_batch.hip): ordered behind every earlier map mutation like the map queries, the
// context's scan; the resident filter, the update's KfDev / mailbox / capture and the timing records are left alone
static int batch_common(lv_ctx* c, const lv_state* xs, size_t m, const double* P, bool solve, lv_state* x_out, double* P_out, int* passes,
                        lv_sums* out) {
    if (c->ranks.multi_rank()) { set_error("multi-hypothesis updates run on one GPU: this context has a multi-GPU communicator"); return LV_ESTATE; }
    if (c->upd.in_update) { set_error("multi-hypothesis update inside lv_update_begin / lv_update_end"); return LV_ESTATE; }
    if (passes) std::memset(passes, 0, m * sizeof(int));
    if (out) std::memset(out, 0, m * sizeof(lv_sums));
    if (P_out) for (size_t i = 0; i < m; ++i) std::memcpy(P_out + i * NS * NS, P, sizeof(double) * NS * NS);
    if (c->map.view.m == 0 || c->scan.n == 0) return LV_OK;   // every state unchanged, passes 0, n_valid 0
    std::vector<double> recs(out ? m * SUMS_LEN : 0);
    int rc = c->batch.run(c->prm, c->upd.max_blocks, c->map.view, c->scan.d_sorted, c->scan.n, c->stream, xs, m, P, solve, x_out, P_out, passes,
                          out ? recs.data() : nullptr);
    if (rc) return rc;
    if (out) for (size_t i = 0; i < m; ++i) unpack_sums(recs.data() + i * SUMS_LEN, &out[i]);
    return LV_OK;
}

int lv_iterate_batch(lv_ctx* c, const lv_state* xs, size_t m, lv_sums* out) {
    LV_CHECK_CTX(c);
    if (m == 0) return LV_OK;
    if (!xs || !out) { set_error("null argument"); return LV_EINVAL; }
    if (int rr = map_side(c).ready()) return rr;
    return batch_common(c, xs, m, nullptr, false, nullptr, nullptr, nullptr, out);
}

int lv_update_batch(lv_ctx* c, lv_state* xs, size_t m, const double* P, double* P_out, int* passes, lv_sums* last) {
    LV_CHECK_CTX(c);
    if (m == 0) return LV_OK;
    if (!xs || !P) { set_error("null argument"); return LV_EINVAL; }
    if (int rr = map_side(c).ready()) return rr;
    return batch_common(c, xs, m, P, true, xs, P_out, passes, last);
}

int lv_scan_set(lv_ctx* c, const void* points, size_t stride, size_t n) {
    LV_CHECK_CTX(c);
    if (n && (!points || stride < 12)) { set_error("bad point array (stride %zu)", stride); return LV_EINVAL; }
    if (n > 0xFFFFFFF0ull) { set_error("scan too large"); return LV_EINVAL; }
    if (int rc = ensure_stage(c, n)) return rc;
    if (int rc = c->scan.reserve(n)) return rc;
    LV_HIP(hipStreamSynchronize(c->stream));  // staging buffer reuse
    float bmin[3] = {INFINITY, INFINITY, INFINITY};
    stage_points(c, points, stride, n, StageW::Index, bmin);
    new_scan(c);
    c->scan.n = (uint32_t)n;   // (uploaded as it is: no voxel grid ran, the route stays "none")
    if (n == 0) return LV_OK;
    LV_HIP(hipMemcpyAsync(c->scan.d_raw, c->h_stage, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return c->scan.sort(c->stream, bmin, c->prm.voxel_size);
}

int lv_scan_deskew(lv_ctx* c, const void* points, size_t stride, size_t time_offset, size_t n, const lv_motion_state* states,
                   size_t n_states, const lv_motion_state* Xt2, float downsample_prec) {
    LV_CHECK_CTX(c);
    static_assert(sizeof(lv_motion_state) == sizeof(MotionState), "lv_motion_state layout");
    if (n && (!points || stride < 12 || time_offset + 8 > stride)) { set_error("bad point array (stride %zu, time offset %zu)", stride, time_offset); return LV_EINVAL; }
    if (!states || n_states < 2 || !Xt2) { set_error("need >= 2 surrounding states and Xt2"); return LV_EINVAL; }
    if (n > 0xFFFFFFF0ull) { set_error("scan too large"); return LV_EINVAL; }
    new_scan(c);
    if (n == 0) return LV_OK;
    if (int rc = ensure_stage(c, n + (n + 1) / 2)) return rc;  // float4 xyz + packed doubles behind them
    if (int rc = c->scan.reserve_raw(n, n_states)) return rc;
    LV_HIP(hipStreamSynchronize(c->stream));  // staging buffer reuse
    double* h_times = reinterpret_cast<double*>(c->h_stage + n);
    stage_points(c, points, stride, n, StageW::Zero, nullptr, h_times, time_offset);
    LV_HIP(hipMemcpyAsync(c->scan.d_in, c->h_stage, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    LV_HIP(hipMemcpyAsync(c->scan.d_times, h_times, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LV_HIP(hipMemcpyAsync(c->scan.d_states, states, n_states * sizeof(MotionState), hipMemcpyHostToDevice, c->stream));
    MotionState xt2;
    std::memcpy(&xt2, Xt2, sizeof(xt2));
    return c->scan.deskew_downsample(c->stream, (uint32_t)n, (uint32_t)n_states, xt2, downsample_prec, c->prm.voxel_size);
}

// Compensator::downsample(points) on its own (Compensator.cpp:104-107, 148-163): the voxel grid of lv_scan_deskew
// applied to points that are already compensated; the result becomes the current scan
int lv_scan_downsample(lv_ctx* c, const void* points, size_t stride, size_t n, float downsample_prec) {
    LV_CHECK_CTX(c);
    if (n && (!points || stride < 12)) { set_error("bad point array (stride %zu)", stride); return LV_EINVAL; }
    if (n > 0xFFFFFFF0ull) { set_error("scan too large"); return LV_EINVAL; }
    new_scan(c);
    if (n == 0) return LV_OK;
    if (int rc = ensure_stage(c, n)) return rc;
    if (int rc = c->scan.reserve_raw(n, 2)) return rc;
    if (int rc = c->scan.reserve(n)) return rc;
    LV_HIP(hipStreamSynchronize(c->stream));  // staging buffer reuse
    stage_points(c, points, stride, n, StageW::Index);
    float4* dst = downsample_prec > 0.f ? c->scan.d_desk : c->scan.d_raw;
    LV_HIP(hipMemcpyAsync(dst, c->h_stage, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return c->scan.voxel_and_sort(c->stream, (uint32_t)n, downsample_prec, c->prm.voxel_size, true);
}

// ---- row f-4: LiDAR wire formats ----------------------------------------------------------------------------
int lv_cloud_format_preset(int lidar_type, lv_cloud_format* out) {
    if (!out) { set_error("null argument"); return LV_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    out->off_x = 0; out->off_y = 4; out->off_z = 8;   // PCL_ADD_POINT4D
    switch (lidar_type) {
        case LV_LIDAR_VELODYNE:   // velodyne_ros::Point, Common.hpp:109-117
            out->point_step = 32; out->off_intensity = 16; out->intensity_type = LV_ATTR_F32;
            out->off_time = 20; out->time_type = LV_TIME_F32_SEC; out->relative_time = 1;
            break;
        case LV_LIDAR_HESAI:      // hesai_ros::Point, :119-127
            out->point_step = 48; out->off_intensity = 16; out->intensity_type = LV_ATTR_U8;
            out->off_time = 24; out->time_type = LV_TIME_F64_SEC; out->relative_time = 0;
            break;
        case LV_LIDAR_OUSTER:     // ouster_ros::Point, :155-165 (intensity <- reflectivity, range <- range: Point.cpp:173-176)
            out->point_step = 32; out->off_intensity = 24; out->intensity_type = LV_ATTR_U16;
            out->off_time = 20; out->time_type = LV_TIME_U32_NSEC; out->relative_time = 1;
            out->off_range = 28; out->range_type = LV_ATTR_U32;
            break;
        case LV_LIDAR_CUSTOM:     // custom::Point == full_info::Point, :129-153
            out->point_step = 48; out->off_intensity = 20; out->intensity_type = LV_ATTR_F32;
            out->off_time = 32; out->time_type = LV_TIME_F64_SEC; out->relative_time = 0;
            break;
        default: set_error("unknown LiDAR type %d", lidar_type); return LV_EINVAL;
    }
    return LV_OK;
}

namespace {
double microsec_to_sec(uint64_t t) {   // Conversions::microsec2Sec (src/Utils/Utils.cpp:18-23): int arithmetic as there
    const int order = 1000000;
    const int secs = (int)(t / (uint64_t)order);
    const int musecs = (int)(t % (uint64_t)order);
    return secs + musecs * 1e-6;
}
double nanosec_to_sec_host(uint32_t t) {   // Conversions::nanosec2Sec (:25-30)
    const int order = 1000000000;
    const int secs = (int)(t / (uint32_t)order);
    const int nsecs = (int)(t % (uint32_t)order);
    return secs + nsecs * 1e-9;
}
double raw_time(const unsigned char* rec, const lv_cloud_format& f) {
    if (f.time_type == LV_TIME_F32_SEC) { float v; std::memcpy(&v, rec + f.off_time, 4); return (double)v; }
    if (f.time_type == LV_TIME_U32_NSEC) { uint32_t v; std::memcpy(&v, rec + f.off_time, 4); return nanosec_to_sec_host(v); }
    double v; std::memcpy(&v, rec + f.off_time, 8); return v;
}
}  // namespace

int lv_cloud_ingest(lv_ctx* c, const void* data, size_t n, const lv_cloud_format* f, const lv_ingest_params* prm, size_t* n_kept) {
    LV_CHECK_CTX(c);
    static_assert(sizeof(lv_cloud_format) == sizeof(CloudFormat) && sizeof(lv_ingest_params) == sizeof(IngestParams), "f-4 struct layouts");
    if (n_kept) *n_kept = 0;
    if (!f || !prm || (n && !data)) { set_error("null argument"); return LV_EINVAL; }
    const uint32_t tsz = f->time_type == LV_TIME_F64_SEC ? 8u : 4u;
    if (f->point_step < 12 || f->off_x + 4 > f->point_step || f->off_y + 4 > f->point_step || f->off_z + 4 > f->point_step ||
        f->off_time + tsz > f->point_step || f->time_type < 0 || f->time_type > 2 ||
        (f->intensity_type != LV_ATTR_NONE && f->off_intensity + 4 > f->point_step + 3) || f->off_range + 4 > f->point_step + 4) {
        set_error("bad cloud format (point_step %u)", f->point_step);
        return LV_EINVAL;
    }
    if (n > 0x7FFFFFF0ull) { set_error("message too large"); return LV_EINVAL; }
    if (n == 0) return LV_OK;
    // PointCloudProcessor::get_begin_time (PointCloudProcessor.cpp:43-47,57-60,70-74,84-91)
    double begin = 0.0;
    if (f->relative_time) {
        const unsigned char* raw = static_cast<const unsigned char*>(data);
        const double front = raw_time(raw, *f), back = raw_time(raw + (n - 1) * (size_t)f->point_step, *f);
        begin = microsec_to_sec(prm->header_stamp_usec) + front;
        if (!prm->stamp_beginning) begin = begin - back;
    }
    CloudFormat cf;
    IngestParams ip;
    std::memcpy(&cf, f, sizeof(cf));
    std::memcpy(&ip, prm, sizeof(ip));
    return c->cloud.ingest(c->stream, data, n, cf, ip, begin, n_kept);
}

int lv_cloud_reserve(lv_ctx* c, size_t max_points_per_message, size_t point_step, size_t buffer_points) {
    LV_CHECK_CTX(c);
    if (point_step < 12 || max_points_per_message > 0x7FFFFFF0ull || buffer_points > 0x7FFFFFF0ull) { set_error("bad sizes"); return LV_EINVAL; }
    int rc = c->cloud.init();
    if (rc) return rc;
    if (max_points_per_message) rc = c->cloud.reserve_msg(max_points_per_message, max_points_per_message * point_step);
    if (rc) return rc;
    rc = c->cloud.settle();
    if (rc) return rc;
    return buffer_points ? c->cloud.reserve_buffer(c->stream, (size_t)c->cloud.size + buffer_points) : LV_OK;
}

int lv_reserve_stream(lv_ctx* c, size_t max_window_points, size_t max_scan_points) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    if (max_window_points > 0x7FFFFFF0ull || max_scan_points > 0x7FFFFFF0ull) { set_error("bad sizes"); return LV_EINVAL; }
    LV_HIP(hipStreamSynchronize(c->stream));
    int rc = LV_OK;
    if (max_window_points) {
        rc = c->scan.reserve_raw(max_window_points, 64);
        if (!rc) rc = c->scan.reserve(max_window_points);
        if (!rc && c->scan.tile_points) rc = c->scan.reserve_tiles((uint32_t)((max_window_points + c->scan.tile_points - 1) / c->scan.tile_points));
        if (rc) return rc;
        LV_HIP(note_alloc(c->scan.notes));
    }
    if (max_scan_points) {
        rc = c->scan.reserve(max_scan_points);
        if (!rc) rc = c->map.reserve_batch(max_scan_points);
        if (rc) return rc;
        LV_HIP(note_alloc(c->map.notes));
        if (int rg = c->upd.grow_records(c->stream, max_scan_points)) return rg;
    }
    return LV_OK;
}

size_t lv_cloud_size(lv_ctx* c) {
    if (!c) return 0;
    c->cloud.settle();
    return (size_t)(c->cloud.size - c->cloud.head);
}

int lv_cloud_fetch(lv_ctx* c, double t1, double t2, void* out, size_t capacity, size_t* n) {
    LV_CHECK_CTX(c);
    if (n) *n = 0;
    uint32_t lo = 0, hi = 0;
    int rc = c->cloud.window(c->stream, t1, t2, &lo, &hi);
    if (rc) return rc;
    const size_t cnt = hi - lo;
    if (n) *n = cnt;
    if (cnt == 0) return LV_OK;
    if (!out || capacity < cnt) { set_error("capacity %zu too small for %zu points", capacity, cnt); return LV_EINVAL; }
    LV_HIP(hipMemcpy(out, c->cloud.d_buf + lo, cnt * sizeof(CloudPoint), hipMemcpyDeviceToHost));
    return LV_OK;
}

int lv_cloud_clear(lv_ctx* c, double t) {
    LV_CHECK_CTX(c);
    return c->cloud.clear_before(c->stream, t);
}

int lv_scan_deskew_window(lv_ctx* c, double t1, double t2, const lv_motion_state* states, size_t n_states, const lv_motion_state* Xt2,
                          float downsample_prec, size_t* n_window) {
    LV_CHECK_CTX(c);
    if (n_window) *n_window = 0;
    if (!states || n_states < 2 || !Xt2) { set_error("need >= 2 surrounding states and Xt2"); return LV_EINVAL; }
    new_scan(c);
    uint32_t lo = 0, hi = 0;
    int rc = c->scan.reserve_raw(1, n_states);   // (the bounds words exist: the window kernel resets them on the way)
    if (rc) return rc;
    rc = c->cloud.window(c->stream, t1, t2, &lo, &hi, c->scan.d_bounds);
    if (rc) return rc;
    const uint32_t n = hi - lo;
    if (n_window) *n_window = n;
    if (n == 0) return LV_OK;   // Compensator::compensate returns no points (Compensator.cpp:24)
    rc = c->scan.reserve_raw(n, n_states);
    if (rc) return rc;
    if (n_states <= 64) {
        MotionState* slot = c->h_states_ring + (size_t)c->states_slot * 64;
        c->states_slot = (c->states_slot + 1) & 7;
        std::memcpy(slot, states, n_states * sizeof(MotionState));
        LV_HIP(hipMemcpyAsync(c->scan.d_states, slot, n_states * sizeof(MotionState), hipMemcpyHostToDevice, c->stream));
    } else {
        LV_HIP(hipMemcpyAsync(c->scan.d_states, states, n_states * sizeof(MotionState), hipMemcpyHostToDevice, c->stream));
    }
    MotionState xt2;
    std::memcpy(&xt2, Xt2, sizeof(xt2));
    if (!c->scan.small_window_applies(n) && c->scan.large_window_applies(n, (uint32_t)n_states, downsample_prec)) {
        bool fell_back = false;   // (more points out than the one-workgroup tail takes: the general chain, from the raw points)
        rc = c->scan.window_large(c->stream, c->cloud.d_buf + lo, n, (uint32_t)n_states, xt2, downsample_prec, c->prm.voxel_size, &fell_back);
        if (rc || !fell_back) return rc;
    }
    rc = c->cloud.unpack(c->stream, lo, n, c->scan.d_in, c->scan.d_times);
    if (rc) return rc;
    return c->scan.deskew_downsample(c->stream, n, (uint32_t)n_states, xt2, downsample_prec, c->prm.voxel_size);
}

size_t lv_scan_size(lv_ctx* c) { return c ? c->scan.n : 0; }
int lv_scan_route(lv_ctx* c) { return c ? c->scan.route : LV_SCAN_ROUTE_NONE; }

int lv_scan_fetch(lv_ctx* c, float* xyz_out, size_t capacity) {
    LV_CHECK_CTX(c);
    const size_t n = c->scan.n;
    if (capacity < n || (!xyz_out && capacity)) { set_error("capacity too small"); return LV_EINVAL; }
    if (n == 0) return LV_OK;
    std::vector<float4> tmp(n);
    LV_HIP(hipStreamSynchronize(c->stream));
    LV_HIP(hipMemcpy(tmp.data(), c->scan.d_raw, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { xyz_out[3 * i] = tmp[i].x; xyz_out[3 * i + 1] = tmp[i].y; xyz_out[3 * i + 2] = tmp[i].z; }
    return LV_OK;
}

int lv_set_capture(lv_ctx* c, int enabled) {
    LV_CHECK_CTX(c);
    c->upd.capture = enabled != 0;
    return LV_OK;
}

int lv_set_record_dump(lv_ctx* c, int enabled) {
    LV_CHECK_CTX(c);
    c->upd.record_dump = enabled != 0;
    return LV_OK;
}

int lv_last_update_fused(lv_ctx* c) { return (c && c->upd.last_update_fused) ? 1 : 0; }
int lv_last_passes(lv_ctx* c) { return c ? c->upd.h_io->passes : 0; }

int lv_pass_geometry(size_t n_scan, int n_cus, int out[4]) {
    if (!out || n_cus < 1 || n_scan > 0xFFFFFFF0ull) { set_error("lv_pass_geometry: bad arguments"); return LV_EINVAL; }
    pass_grid_size((uint32_t)n_scan, n_cus, &out[0], &out[1], &out[2], &out[3]);
    return LV_OK;
}

int lv_set_fused_pass(lv_ctx* c, int enabled) {
    LV_CHECK_CTX(c);
    c->upd.fused_pass = enabled != 0;
    return LV_OK;
}

int lv_set_option(lv_ctx* c, const char* name, int value) {
    LV_CHECK_CTX(c);
    if (!name) { set_error("null argument"); return LV_EINVAL; }
    if (int rb = c->upd.busy("lv_set_option")) return rb;
    if (!std::strcmp(name, "traj_tile")) { c->traj.tile = value != 0; return LV_OK; }   // (the trajectory stands beside the update's table)
    return Knobs<lv_ctx>::set_option(*c, name, value);   // (the table: lv_knobs.hpp)
}

int lv_get_pass_clocks(lv_ctx* c, long long* out, int capacity_wg, int* n_wg) {
    LV_CHECK_CTX(c);
    if (!c->upd.d_pclk) { set_error("no pass clocks: create the context with LV_PASS_CLK=1 in the environment"); return LV_ESTATE; }
    // layout: [launch 0 .. MAX_NUM_ITERS + 1][pass_max_wg + 1 workgroup slots][pass_clock_words()]; slot n_wg - 1 of a launch is
    // its bookkeeping workgroup (stamp 10 = books done); the closing launch has one workgroup (slot 0)
    const int slots = c->upd.pass_max_wg + 1;
    if (!out) {   // size query: *n_wg = workgroup slots per launch (the stride of the layout)
        if (n_wg) *n_wg = slots;
        return LV_OK;
    }
    if (capacity_wg < slots) { set_error("lv_get_pass_clocks: capacity %d < %d workgroup slots per launch", capacity_wg, slots); return LV_EINVAL; }
    LV_HIP(hipStreamSynchronize(c->stream));
    LV_HIP(hipMemcpy(out, c->upd.d_pclk, (size_t)(c->prm.MAX_NUM_ITERS + 2) * slots * pass_clock_words() * sizeof(long long), hipMemcpyDeviceToHost));
    if (n_wg) *n_wg = c->upd.pclk_wg;
    return LV_OK;
}

int lv_iterate(lv_ctx* c, const lv_state* x, lv_sums* out) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    if (!x || !out) { set_error("null argument"); return LV_EINVAL; }
    return c->upd.iterate(inputs(c), x, out);
}

int lv_update_begin(lv_ctx* c, const lv_state* x, const double* P) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    if (!x || !P) { set_error("null argument"); return LV_EINVAL; }
    return c->upd.update_begin(inputs(c), x, P);
}

int lv_pass_reduce(lv_ctx* c) {
    LV_CHECK_CTX(c);
    return c->upd.split_reduce(inputs(c));
}

// ---- multi-GPU (row e): RCCL issued from the library on the context stream ------------------------------
int lv_comm_unique_id(const char* rccl_library, void* id128) {
    if (!id128) { set_error("null argument"); return LV_EINVAL; }
    return comm_unique_id(rccl_library, id128);
}

int lv_comm_init(lv_ctx* c, const char* rccl_library, const void* id128, int rank, int world) {
    LV_CHECK_CTX(c);
    if (!id128 || world < 1 || rank < 0 || rank >= world) { set_error("lv_comm_init: bad arguments (rank %d, world %d)", rank, world); return LV_EINVAL; }
    if (int rb = c->upd.busy("lv_comm_init")) return rb;
    return c->ranks.init_rccl(rccl_library, id128, rank, world);
}

int lv_comm_destroy(lv_ctx* c) {
    LV_CHECK_CTX(c);
    if (int rb = c->upd.busy("lv_comm_destroy")) return rb;
    return c->ranks.destroy(c->stream);
}

int lv_comm_set_host_gather(lv_ctx* c, int rank, int world, lv_gather_fn fn, void* user) {
    LV_CHECK_CTX(c);
    if (int rb = c->upd.busy("lv_comm_set_host_gather")) return rb;
    return c->ranks.set_host_gather(c->stream, rank, world, fn, user);
}

int lv_comm_peer_export(lv_ctx* c, void* handle_blob) {
    LV_CHECK_CTX(c);
    if (!handle_blob) { set_error("null argument"); return LV_EINVAL; }
    if (int rb = c->upd.busy("lv_comm_peer_export")) return rb;
    return c->ranks.peer_export(c->stream, c->upd.pass_max_wg, handle_blob);
}

int lv_comm_peer_init(lv_ctx* c, int rank, int world, const void* handles) {
    LV_CHECK_CTX(c);
    if (!handles) { set_error("null argument"); return LV_EINVAL; }
    if (int rb = c->upd.busy("lv_comm_peer_init")) return rb;
    return c->ranks.peer_init(c->stream, rank, world, handles);
}

int lv_comm_world(lv_ctx* c) { return c ? c->ranks.world : 0; }

int lv_comm_set_shard_max(lv_ctx* c, size_t n_max) {
    LV_CHECK_CTX(c);
    if (int rb = c->upd.busy("lv_comm_set_shard_max")) return rb;
    if (n_max > 0xFFFFFFF0ull) { set_error("shard too large"); return LV_EINVAL; }
    c->ranks.shard_max = n_max;
    if (!c->ranks.multi_rank() || n_max == 0) return LV_OK;
    int nwg = 0, rounds = 0, steps = 0, dedicated = 0;
    pass_grid_size((uint32_t)n_max, c->upd.pass_max_wg, &nwg, &steps, &rounds, &dedicated);
    return c->ranks.reserve(c->stream, (size_t)nwg * c->upd.partial_width());
}

int lv_set_comm_fused(lv_ctx* c, int enabled) {
    LV_CHECK_CTX(c);
    c->ranks.fused = enabled != 0;
    return LV_OK;
}

void* lv_sums_device_ptr(lv_ctx* c) { return c ? (void*)c->upd.d_sums : nullptr; }

int lv_set_sums_buffer(lv_ctx* c, void* device_ptr) {
    LV_CHECK_CTX(c);
    return c->upd.set_sums_buffer(c->stream, device_ptr);
}

int lv_pass_solve(lv_ctx* c) {
    LV_CHECK_CTX(c);
    return c->upd.split_solve(c->stream);
}

int lv_update_end(lv_ctx* c, lv_state* x, double* P, int* passes) {
    LV_CHECK_CTX(c);
    return c->upd.update_end(c->stream, x, P, passes);
}

int lv_update(lv_ctx* c, lv_state* x, double* P, int* passes, lv_sums* per_pass, double* trace) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    if (!x || !P) { set_error("null argument"); return LV_EINVAL; }
    return c->upd.update(inputs(c), x, P, passes, per_pass, trace);
}

// ---- resident filter (row f-3) ---------------------------------------------------------------------
int lv_filter_set(lv_ctx* c, const lv_state* x, const double* P) {
    LV_CHECK_CTX(c);
    if (!x || !P) { set_error("null argument"); return LV_EINVAL; }
    return c->filter.set(x, P);
}

int lv_filter_get(lv_ctx* c, lv_state* x, double* P) {
    LV_CHECK_CTX(c);
    return c->upd.filter_get(c->stream, x, P);
}

int lv_predict(lv_ctx* c, double dt, const double* Q, const double acc[3], const double gyro[3]) {
    LV_CHECK_CTX(c);
    if (!Q || !acc || !gyro) { set_error("null argument"); return LV_EINVAL; }
    return c->filter.predict(c->stream, c->upd.d_kf, dt, Q, acc, gyro);
}

// ---- aiding observations (lv_observe.hip; the argument rules: lv_observe.hpp) --------------------------
void lv_default_observation(lv_observation* o, int kind) { default_observation(o, kind); }

int lv_observe_results(lv_ctx* c, lv_observe_result* out, size_t capacity, size_t* n) {
    LV_CHECK_CTX(c);
    if (c->n_obs == 0) { set_error("lv_observe_results before lv_observe"); return LV_ESTATE; }
    if (n) *n = (size_t)c->n_obs;
    if (!out || capacity < (size_t)c->n_obs) { set_error("lv_observe_results: room for %zu of %d results", out ? capacity : (size_t)0, c->n_obs); return LV_EINVAL; }
    LV_HIP(hipMemcpyAsync(out, c->d_obs, (size_t)c->n_obs * sizeof(lv_observe_result), hipMemcpyDeviceToHost, c->stream));
    LV_HIP(hipStreamSynchronize(c->stream));
    return LV_OK;
}

int lv_observe(lv_ctx* c, const lv_observation* obs, size_t n, lv_observe_result* out) {
    LV_CHECK_CTX(c);
    if (int r = c->filter.observe(c->stream, c->upd.d_kf, obs, n, c->d_obs)) return r;
    c->n_obs = (int)n;
    return out ? lv_observe_results(c, out, n, nullptr) : LV_OK;
}

int lv_correct(lv_ctx* c, int* passes) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    return c->upd.correct(inputs(c), passes);
}

static int fetch_check(lv_ctx* c) {
    if (!c->upd.dbg_valid || !c->upd.dbg.knn_idx) { set_error("no captured pass: call lv_iterate (or lv_set_capture(1) before lv_update)"); return LV_ESTATE; }
    LV_HIP(hipStreamSynchronize(c->stream));
    return LV_OK;
}

int lv_fetch_knn(lv_ctx* c, uint32_t* idx, float* d2) {
    LV_CHECK_CTX(c);
    LV_SETTLE_MAP(c);
    int rc = fetch_check(c);
    if (rc) return rc;
    const size_t n = c->scan.n, K = (size_t)c->prm.NUM_MATCH_POINTS;
    if (idx) {
        LV_HIP(hipMemcpy(idx, c->upd.dbg.knn_idx, n * K * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (c->map.n_ids != c->map.m) {   // the kernels report point ids; the API's index space is the rank among the living
            const size_t ids = c->map.n_ids;
            std::vector<float4> pts(ids);
            LV_HIP(hipMemcpy(pts.data(), c->map.d_orig, ids * sizeof(float4), hipMemcpyDeviceToHost));
            std::vector<uint32_t> rank(ids);
            uint32_t r = 0;
            for (size_t i = 0; i < ids; ++i) { rank[i] = r; r += std::isfinite(pts[i].x) ? 1u : 0u; }
            for (size_t i = 0; i < n * K; ++i)
                if (idx[i] != 0xFFFFFFFFu && idx[i] < ids) idx[i] = rank[idx[i]];
        }
    }
    if (d2) LV_HIP(hipMemcpy(d2, c->upd.dbg.knn_d2, n * K * sizeof(float), hipMemcpyDeviceToHost));
    return LV_OK;
}

int lv_fetch_matches(lv_ctx* c, uint8_t* valid, float* p_world, float* abcd, float* dist) {
    LV_CHECK_CTX(c);
    int rc = fetch_check(c);
    if (rc) return rc;
    const size_t n = c->scan.n;
    if (valid) LV_HIP(hipMemcpy(valid, c->upd.dbg.valid, n, hipMemcpyDeviceToHost));
    if (p_world) LV_HIP(hipMemcpy(p_world, c->upd.dbg.p_world, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (abcd) LV_HIP(hipMemcpy(abcd, c->upd.dbg.abcd, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (dist) LV_HIP(hipMemcpy(dist, c->upd.dbg.dist, n * sizeof(float), hipMemcpyDeviceToHost));
    return LV_OK;
}

int lv_fetch_neighbors(lv_ctx* c, float* nbr_xyz, float* d2, float* p_world, int32_t* found) {
    LV_CHECK_CTX(c);
    const size_t n = c->scan.n;
    if (n == 0) return LV_OK;
    if (!c->upd.qrec_valid || !c->upd.d_qrec || c->upd.qstride < n) { set_error("no pass has run on the current scan"); return LV_ESTATE; }
    LV_HIP(hipStreamSynchronize(c->stream));
    const int K = c->prm.NUM_MATCH_POINTS, NSL = qrec_slots(K);
    std::vector<float4> rec((size_t)NSL * n);
    for (int sl = 0; sl < NSL; ++sl)
        LV_HIP(hipMemcpy(rec.data() + (size_t)sl * n, c->upd.d_qrec + (size_t)sl * c->upd.qstride, n * sizeof(float4), hipMemcpyDeviceToHost));
    const float inf = std::numeric_limits<float>::infinity();
    const auto dword = [&](size_t q, int w) {   // word w of the distance slots: distance of neighbour w, then `found`
        const float4& v = rec[(size_t)(K + 1 + w / 4) * n + q];
        return (w & 3) == 0 ? v.x : (w & 3) == 1 ? v.y : (w & 3) == 2 ? v.z : v.w;
    };
    for (size_t q = 0; q < n; ++q) {   // records are in the scan's Morton order: slot K carries the original index
        uint32_t oq;
        std::memcpy(&oq, &rec[(size_t)K * n + q].w, 4);
        if (oq >= n) { set_error("corrupt hand-over record %zu", q); return LV_ESTATE; }
        int32_t fnd;
        const float fw = dword(q, K);
        std::memcpy(&fnd, &fw, 4);
        for (int j = 0; j < K; ++j) {
            const bool have = j < fnd;
            if (nbr_xyz) {
                nbr_xyz[((size_t)oq * K + j) * 3 + 0] = have ? rec[(size_t)j * n + q].x : 0.f;
                nbr_xyz[((size_t)oq * K + j) * 3 + 1] = have ? rec[(size_t)j * n + q].y : 0.f;
                nbr_xyz[((size_t)oq * K + j) * 3 + 2] = have ? rec[(size_t)j * n + q].z : 0.f;
            }
            if (d2) d2[(size_t)oq * K + j] = have ? dword(q, j) : inf;
        }
        if (p_world) { const float4& w = rec[(size_t)K * n + q]; p_world[(size_t)oq * 3] = w.x; p_world[(size_t)oq * 3 + 1] = w.y; p_world[(size_t)oq * 3 + 2] = w.z; }
        if (found) found[oq] = fnd;
    }
    return LV_OK;
}

int lv_fetch_rows(lv_ctx* c, double* H, double* h) {
    LV_CHECK_CTX(c);
    int rc = fetch_check(c);
    if (rc) return rc;
    const size_t n = c->scan.n;
    if (H) LV_HIP(hipMemcpy(H, c->upd.dbg.rows, n * 12 * sizeof(double), hipMemcpyDeviceToHost));
    if (h) LV_HIP(hipMemcpy(h, c->upd.dbg.h, n * sizeof(double), hipMemcpyDeviceToHost));
    return LV_OK;
}

int lv_calculate_H(lv_ctx* c, const lv_state* x, const float* p_world, const float* abcd, const float* dist, size_t n,
                   double* H, double* h) {
    LV_CHECK_CTX(c);
    if (!x || (n && (!p_world || !abcd || !dist || !H || !h))) { set_error("null argument"); return LV_EINVAL; }
    if (n == 0) return LV_OK;
    return c->upd.calculate_H(inputs(c), x, p_world, abcd, dist, n, H, h);
}

int lv_get_degeneracy_values(lv_ctx* c, double* eig, int capacity_passes, int* n_passes) {
    LV_CHECK_CTX(c);
    if (n_passes) *n_passes = 0;
    if (!eig || capacity_passes < 0) { set_error("null argument"); return LV_EINVAL; }
    if (c->prm.degeneracy_mode == 0) { set_error("degeneracy_mode is 0: no eigenvalues are computed"); return LV_ESTATE; }
    return c->upd.degeneracy_values(c->stream, eig, capacity_passes, n_passes);
}

int lv_get_level_histogram(lv_ctx* c, int out[8]) {
    LV_CHECK_CTX(c);
    if (!out) { set_error("null argument"); return LV_EINVAL; }
    LV_HIP(hipStreamSynchronize(c->stream));
    LV_HIP(hipMemcpy(out, c->upd.d_kf->level_hist, 8 * sizeof(int), hipMemcpyDeviceToHost));
    return LV_OK;
}

int lv_get_solve_clocks(lv_ctx* c, long long* out, int capacity) {
    LV_CHECK_CTX(c);
    if (!out || capacity < MAX_PASSES * 16) { set_error("capacity must be >= %d", MAX_PASSES * 16); return LV_EINVAL; }
    LV_HIP(hipStreamSynchronize(c->stream));
    LV_HIP(hipMemcpy(out, c->upd.d_kf->solve_clk, sizeof(long long) * MAX_PASSES * 16, hipMemcpyDeviceToHost));
    return LV_OK;
}

int lv_get_timing(lv_ctx* c, lv_timing* out) {
    if (!c || !out) { set_error("null argument"); return LV_EINVAL; }
    *out = c->upd.timing;
    out->mailbox_resyncs = (int)c->upd.mailbox_resyncs;
    return LV_OK;
}

int lv_set_profiling(lv_ctx* c, int enabled) {
    if (!c) { set_error("null context"); return LV_EINVAL; }
    c->upd.profiling = enabled == 1;
    c->upd.phase_clocks = enabled == 2;
    return LV_OK;
}

int lv_get_phase_clocks(lv_ctx* c, long long* out, int capacity_blocks, int* n_blocks) {
    LV_CHECK_CTX(c);
    if (!c->upd.d_clk) { set_error("no phase clocks captured: lv_set_profiling(ctx, 2) first"); return LV_ESTATE; }
    // layout: grid x 8 shader-clock stamps, then grid x 8 records whose first two entries are wall_clock64()
    // (100 MHz, chip-global) at workgroup start / end
    const int nb = 2 * c->upd.grid < capacity_blocks ? 2 * c->upd.grid : capacity_blocks;
    LV_HIP(hipStreamSynchronize(c->stream));
    LV_HIP(hipMemcpy(out, c->upd.d_clk, (size_t)nb * 8 * sizeof(long long), hipMemcpyDeviceToHost));
    if (n_blocks) *n_blocks = nb;
    return LV_OK;
}

// ---- The volume tools (lv_volumes.hpp: what each call asks for, and what makes what stale).  An entry point judges here what it
// judges before the context (what is wrong with those arguments is reported whatever else is), then the context, then c->vol.
// ---- Occupancy grid (lv_occupancy.hip)
void lv_default_occupancy_params(lv_occupancy_params* p) { default_occupancy_params(p); }

int lv_occ_configure(lv_ctx* c, const lv_occupancy_params* p) {
    if (const char* why = occ_check_params(p)) { set_error("lv_occ_configure: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.occ_configure(c->stream, *p);
}

// (these judge nothing before the context: the grid comes first, then their arguments, in VolumeTools)
int lv_occ_integrate(lv_ctx* c, const lv_view* views, size_t n_views, uint64_t stats[4]) { LV_CHECK_CTX(c); return c->vol.occ_integrate(c->stream, views, n_views, stats); }
int lv_occ_query(lv_ctx* c, const void* pts, size_t stride, size_t n, float* logodds) { LV_CHECK_CTX(c); return c->vol.occ_query(c->stream, pts, stride, n, logodds); }
int lv_occ_project(lv_ctx* c, int k_lo, int k_hi, int8_t* grid2d, size_t capacity) { LV_CHECK_CTX(c); return c->vol.occ_project(c->stream, k_lo, k_hi, grid2d, capacity); }
int lv_occ_fetch(lv_ctx* c, float* logodds, size_t capacity) { LV_CHECK_CTX(c); return c->vol.occ_fetch(c->stream, logodds, capacity); }
int lv_occ_load(lv_ctx* c, const float* logodds, size_t n) { LV_CHECK_CTX(c); return c->vol.occ_load(c->stream, logodds, n); }
int lv_occ_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.occ_clear(c->stream); }
int lv_occ_get_params(lv_ctx* c, lv_occupancy_params* out) { LV_CHECK_CTX(c); return c->vol.occ_get_params(out); }

void lv_default_occ_mark_params(lv_occ_mark_params* p) { default_occ_mark_params(p); }

// The map source (lv_maptools.hpp) is read only once there is a box to mark.
int lv_occ_mark(lv_ctx* c, const lv_occ_mark_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]) {
    if (!p) { set_error("lv_occ_mark: null params"); return LV_EINVAL; }
    if (p->min_points < 1 || p->min_points > (1 << 20)) { set_error("lv_occ_mark: min_points = %d: must be in 1..2^20", p->min_points); return LV_EINVAL; }
    if (!(std::isfinite(p->l_mark) && p->l_mark != 0.f)) { set_error("lv_occ_mark: l_mark: finite and not zero"); return LV_EINVAL; }
    if (pts && stride < 12) { set_error("lv_occ_mark: bad point array (stride %zu)", stride); return LV_EINVAL; }
    if (pts && n >= ((size_t)1 << 31)) { set_error("lv_occ_mark: too many points"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    int lo[3], hi[3];
    bool any_box = false;
    if (int rc = c->vol.occ_mark_box(*p, lo, hi, stats, &any_box)) return rc;
    if (!any_box) return LV_OK;
    const float4* d_orig;
    uint32_t n_ids, m;
    if (int rc = map_side(c).source(pts, &d_orig, &n_ids, &m)) return rc;
    return c->vol.occ_mark(c->stream, *p, lo, hi, d_orig, n_ids, pts, stride, n, stats);
}

// ---- Occupancy from the surface (lv_surf_occ.hip)
void lv_default_occ_surface_params(lv_occ_surface_params* p) { default_occ_surface_params(p); }

int lv_occ_from_surface(lv_ctx* c, const lv_occ_surface_params* p, uint64_t stats[4]) {
    char why[96];
    if (!surf_occ_check_params(p, why, sizeof(why))) { set_error("lv_occ_from_surface: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.occ_from_surface(c->stream, *p, stats);
}

// ---- Distance field (lv_distance.hip)
void lv_default_distance_params(lv_distance_params* p) { default_distance_params(p); }

int lv_occ_distance_build(lv_ctx* c, const lv_distance_params* p, uint64_t stats[4]) {
    if (const char* why = dist_check_params(p)) { set_error("lv_occ_distance_build: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.distance_build(c->stream, *p, stats);
}

int lv_occ_distance_build_cells(lv_ctx* c, const lv_distance_params* p, const int8_t* cells, size_t n, uint64_t stats[4]) {
    if (const char* why = dist_check_params_cells(p, cells)) { set_error("lv_occ_distance_build_cells: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.distance_build_cells(c->stream, *p, cells, n, stats);
}

int lv_occ_distance_fetch(lv_ctx* c, int32_t* s2, float* metres, size_t capacity) {
    if (!s2 && !metres) { set_error("lv_occ_distance_fetch: s2 and metres are both null"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.distance_fetch(c->stream, s2, metres, capacity);
}

int lv_occ_distance_query(lv_ctx* c, const void* pts, size_t stride, size_t n, float* dist, float* grad) { LV_CHECK_CTX(c); return c->vol.distance_query(c->stream, pts, stride, n, dist, grad); }
int lv_occ_distance_info(lv_ctx* c, lv_distance_info* out) { LV_CHECK_CTX(c); return c->vol.distance_info(out); }
int lv_occ_distance_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.distance_clear(c->stream); }

// ---- Planner (lv_plan.hip)
void lv_default_plan_params(lv_plan_params* p) { default_plan_params(p); }

int lv_occ_plan_build(lv_ctx* c, const lv_plan_params* p, const uint8_t* cost, size_t n_cost, const void* goals, size_t stride, size_t n_goals,
                      uint64_t stats[4]) {
    if (const char* why = plan_check(p, cost, n_cost, goals, stride, n_goals)) { set_error("lv_occ_plan_build: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.plan_build(c->stream, *p, cost, n_cost, goals, stride, n_goals, stats);
}

int lv_occ_plan_fetch(lv_ctx* c, uint32_t* potential, uint8_t* cell_cost, size_t capacity) {
    if (!potential && !cell_cost) { set_error("lv_occ_plan_fetch: potential and cell_cost are both null"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.plan_fetch(c->stream, potential, cell_cost, capacity);
}

int lv_occ_plan_paths(lv_ctx* c, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets, int32_t* cells,
                      size_t capacity, size_t* total) {
    LV_CHECK_CTX(c);
    return c->vol.plan_paths(c->stream, starts, stride, n, status, cost, offsets, cells, capacity, total);
}

int lv_occ_plan_info(lv_ctx* c, lv_plan_info* out) { LV_CHECK_CTX(c); return c->vol.plan_info(out); }
int lv_occ_plan_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.plan_clear(c->stream); }

// ---- Lattice planner (lv_lattice.hip)
void lv_default_lattice_params(lv_lattice_params* p) { default_lattice_params(p); }

int lv_occ_lattice_build(lv_ctx* c, const lv_lattice_params* p, const lv_lattice_prim* prims, size_t n_prims, const void* goals, size_t stride,
                         size_t n_goals, uint64_t stats[4]) {
    size_t rec = LAT_NO_RECORD;
    if (const char* why = lattice_check(p, prims, n_prims, goals, stride, n_goals, &rec)) {
        if (rec == LAT_NO_RECORD) set_error("lv_occ_lattice_build: %s", why);
        else set_error("lv_occ_lattice_build: record %zu (heading %zu, primitive %zu): %s", rec, rec / (size_t)p->P, rec % (size_t)p->P, why);
        return LV_EINVAL;
    }
    LV_CHECK_CTX(c);
    return c->vol.lattice_build(c->stream, *p, prims, goals, stride, n_goals, stats);
}

int lv_occ_lattice_fetch(lv_ctx* c, uint32_t* V, size_t capacity) {
    if (!V) { set_error("lv_occ_lattice_fetch: null V"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.lattice_fetch(c->stream, V, capacity);
}

int lv_occ_lattice_paths(lv_ctx* c, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets, int32_t* states,
                         uint8_t* prims, size_t capacity, size_t* total) {
    LV_CHECK_CTX(c);
    return c->vol.lattice_paths(c->stream, starts, stride, n, status, cost, offsets, states, prims, capacity, total);
}

int lv_occ_lattice_info(lv_ctx* c, lv_lattice_info* out) { LV_CHECK_CTX(c); return c->vol.lattice_info(out); }
int lv_occ_lattice_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.lattice_clear(c->stream); }

// ---- Frontiers (lv_frontier.hip)
void lv_default_frontier_params(lv_frontier_params* p) { default_frontier_params(p); }

int lv_occ_frontier_build(lv_ctx* c, const lv_frontier_params* p, uint64_t stats[4]) {
    if (const char* why = fr_check_params(p)) { set_error("lv_occ_frontier_build: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.frontier_build(c->stream, *p, stats);
}

int lv_occ_frontier_fetch(lv_ctx* c, int32_t* labels, size_t capacity) {
    if (!labels) { set_error("lv_occ_frontier_fetch: null labels"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.frontier_fetch(c->stream, labels, capacity);
}

int lv_occ_frontier_clusters(lv_ctx* c, lv_frontier_cluster* out, size_t capacity, size_t* n) {
    if (!n) { set_error("lv_occ_frontier_clusters: null count"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.frontier_clusters(c->stream, out, capacity, n);
}

int lv_occ_frontier_rank(lv_ctx* c, int reach, uint32_t* best_p, int32_t* best_cell, size_t capacity) {
    if (reach < 0 || reach > FR_MAX_REACH) { set_error("lv_occ_frontier_rank: reach %d: 0..%d", reach, FR_MAX_REACH); return LV_EINVAL; }
    if (!best_p && !best_cell) { set_error("lv_occ_frontier_rank: best_p and best_cell are both null"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.frontier_rank(c->stream, reach, best_p, best_cell, capacity);
}

int lv_occ_frontier_info(lv_ctx* c, lv_frontier_info* out) { LV_CHECK_CTX(c); return c->vol.frontier_info(out); }
int lv_occ_frontier_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.frontier_clear(c->stream); }

// ---- Ray casting (lv_ray.hip)
void lv_default_ray_params(lv_ray_params* p) { default_ray_params(p); }

int lv_occ_raycast(lv_ctx* c, const lv_ray_params* p, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                   lv_ray_result* out) {
    if (!p) { set_error("lv_occ_raycast: null params"); return LV_EINVAL; }
    if (n >= RAY_MAX_N) { set_error("lv_occ_raycast: too many rays"); return LV_EINVAL; }
    if (n && (!from || !to || !out || from_stride < 12 || to_stride < 12)) {
        set_error("lv_occ_raycast: bad point arrays (strides %zu, %zu) or null output", from_stride, to_stride);
        return LV_EINVAL;
    }
    LV_CHECK_CTX(c);
    return c->vol.raycast(c->stream, *p, from, from_stride, to, to_stride, n, out);
}

int lv_occ_view_gain(lv_ctx* c, const lv_view* views, size_t n_views, uint64_t* gain) {
    if (!views || !gain) { set_error("lv_occ_view_gain: null argument"); return LV_EINVAL; }
    if (n_views < 1 || n_views > (size_t)OCC_MAX_VIEWS) { set_error("lv_occ_view_gain: n_views = %zu: must be in 1..%d", n_views, OCC_MAX_VIEWS); return LV_EINVAL; }
    if (int rc = views_ok(views, n_views, "lv_occ_view_gain: ", false, 0xFFFFFFF0ull / 4)) return rc;   // (t is not judged: lv_rules.hpp)
    LV_CHECK_CTX(c);
    return c->vol.view_gain(c->stream, views, n_views, gain);
}

// ---- Rollouts (lv_rollout.hip)
void lv_default_rollout_params(lv_rollout_params* p) { default_rollout_params(p); }

int lv_occ_rollout(lv_ctx* c, const lv_rollout_params* p, const float* start, const float* controls, size_t K, const float* footprint, size_t n_fp,
                   lv_rollout_result* results, float* poses, uint64_t* score, int64_t* best) {
    if (const char* why = rollout_check(p, start, controls, K, footprint, n_fp, results, poses, score, best)) {
        set_error("lv_occ_rollout: %s", why);
        return LV_EINVAL;
    }
    LV_CHECK_CTX(c);
    return c->vol.rollout_run(c->stream, *p, start, controls, K, footprint, n_fp, results, poses, score, best);
}

// ---- Localisation (lv_mcl.hip)
void lv_default_mcl_params(lv_mcl_params* p) { default_mcl_params(p); }

int lv_occ_mcl_weigh(lv_ctx* c, const lv_mcl_params* p, const float* poses, size_t K, const float* beams, size_t B, const uint32_t* table,
                     size_t n_table, uint64_t* score, uint32_t* n_in, int64_t* best) {
    if (const char* why = mcl_check(p, poses, K, beams, B, table, n_table, score, n_in, best)) {
        set_error("lv_occ_mcl_weigh: %s", why);
        return LV_EINVAL;
    }
    LV_CHECK_CTX(c);
    return c->vol.mcl_weigh(c->stream, *p, poses, K, beams, B, table, n_table, score, n_in, best);
}

// ---- Resident localisation filter (lv_mcl_filter.hip).  The particles are world poses: they belong to no grid and no field, so
// the store stands beside the volume tools and the entry points ask for the grid and the field themselves.
void lv_default_mcl_resample_params(lv_mcl_resample_params* p) { default_mcl_resample_params(p); }

#define LV_MCLF_GRID(c) LV_REQUIRE((c)->vol.occ.configured, LV_ESTATE, "no occupancy grid: call lv_occ_configure first")
#define LV_MCLF_FIELD(c) LV_REQUIRE((c)->vol.dist.built, LV_ESTATE, "no distance field: call lv_occ_distance_build first")
#define LV_MCLF_SET(c) LV_REQUIRE((c)->mclf.set, LV_ESTATE, "no particles: call lv_occ_mcl_filter_set first")
#define LV_MCLF_EINVAL(name, why) \
    do {                          \
        if (const char* _w = (why)) { set_error(name ": %s", _w); return LV_EINVAL; } \
    } while (0)
#define LV_MCLF_ESTATE(name, why) \
    do {                          \
        if (const char* _w = (why)) { set_error(name ": %s", _w); return LV_ESTATE; } \
    } while (0)

int lv_occ_mcl_filter_set(lv_ctx* c, const float* poses, size_t K, uint64_t seed) {
    LV_MCLF_EINVAL("lv_occ_mcl_filter_set", mclf_check_set(poses, K));
    LV_CHECK_CTX(c);
    LV_MCLF_GRID(c);
    return c->mclf.set_poses(c->stream, poses, K, seed);
}

int lv_occ_mcl_filter_move(lv_ctx* c, const float* delta, const float* sigma) {
    LV_MCLF_EINVAL("lv_occ_mcl_filter_move", mclf_check_move(delta, sigma));
    LV_CHECK_CTX(c);
    LV_MCLF_GRID(c);
    LV_MCLF_SET(c);
    LV_MCLF_ESTATE("lv_occ_mcl_filter_move", mclf_state_epoch(c->mclf.epoch));
    return c->mclf.move(c->stream, delta, sigma);
}

int lv_occ_mcl_filter_weigh(lv_ctx* c, const lv_mcl_params* p, const float* beams, size_t B, const uint32_t* table, size_t n_table, int64_t* best) {
    LV_MCLF_EINVAL("lv_occ_mcl_filter_weigh", mclf_check_weigh(p, beams, B, table, n_table));
    LV_CHECK_CTX(c);
    LV_MCLF_GRID(c);
    LV_MCLF_FIELD(c);
    LV_MCLF_SET(c);
    LV_MCLF_EINVAL("lv_occ_mcl_filter_weigh", mclf_check_pairs(c->mclf.K, B));
    LV_MCLF_ESTATE("lv_occ_mcl_filter_weigh", mclf_state_since(c->mclf.since));
    return c->mclf.weigh(c->stream, c->vol.dist, *p, beams, B, table, n_table, best);
}

int lv_occ_mcl_filter_resample(lv_ctx* c, const lv_mcl_resample_params* p, const uint32_t* wtable, size_t n_w, lv_mcl_filter_stats* stats,
                               uint32_t* ancestors) {
    LV_MCLF_EINVAL("lv_occ_mcl_filter_resample", mclf_check_resample(p, wtable, n_w, stats));
    LV_CHECK_CTX(c);
    LV_MCLF_GRID(c);
    LV_MCLF_FIELD(c);
    LV_MCLF_SET(c);
    LV_MCLF_ESTATE("lv_occ_mcl_filter_resample", mclf_state_epoch(c->mclf.epoch));
    return c->mclf.resample(c->stream, c->vol.dist, *p, wtable, n_w, stats, ancestors);
}

int lv_occ_mcl_filter_get(lv_ctx* c, float* poses, uint64_t* acc, uint32_t* n_in, size_t capacity) {
    LV_MCLF_EINVAL("lv_occ_mcl_filter_get", mclf_check_get(poses, acc, n_in));
    LV_CHECK_CTX(c);
    LV_MCLF_GRID(c);
    LV_MCLF_SET(c);
    if (capacity < c->mclf.K) { set_error("lv_occ_mcl_filter_get: room for K = %zu particles needed", c->mclf.K); return LV_EINVAL; }
    return c->mclf.get(c->stream, poses, acc, n_in);
}

int lv_occ_mcl_filter_info(lv_ctx* c, lv_mcl_filter_info* out) {
    if (!out) { set_error("lv_occ_mcl_filter_info: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    *out = lv_mcl_filter_info{};
    if (c->mclf.set) {
        out->set = 1;
        out->K = (uint64_t)c->mclf.K;
        out->seed = c->mclf.seed;
        out->epoch = c->mclf.epoch;
        out->since_resample = c->mclf.since;
    }
    return LV_OK;
}

int lv_occ_mcl_filter_clear(lv_ctx* c) {
    LV_CHECK_CTX(c);
    LV_HIP(hipStreamSynchronize(c->stream));
    c->mclf.release();
    return LV_OK;
}

// ---- TSDF and mesh (lv_tsdf.hip)
void lv_default_tsdf_params(lv_tsdf_params* p) { default_tsdf_params(p); }

int lv_tsdf_configure(lv_ctx* c, const lv_tsdf_params* p) {
    if (const char* why = tsdf_check_params(p)) { set_error("lv_tsdf_configure: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.tsdf_configure(c->stream, *p);
}

// (these judge nothing before the context: the volume comes first, then their arguments, in VolumeTools)
int lv_tsdf_integrate(lv_ctx* c, const lv_view* views, size_t n_views, uint64_t stats[4]) { LV_CHECK_CTX(c); return c->vol.tsdf_integrate(c->stream, views, n_views, stats); }
int lv_tsdf_query(lv_ctx* c, const void* pts, size_t stride, size_t n, float* metres, int32_t* weight) { LV_CHECK_CTX(c); return c->vol.tsdf_query(c->stream, pts, stride, n, metres, weight); }
int lv_tsdf_fetch(lv_ctx* c, int32_t* S, int32_t* W, float* metres, size_t capacity) { LV_CHECK_CTX(c); return c->vol.tsdf_fetch(c->stream, S, W, metres, capacity); }
int lv_tsdf_load(lv_ctx* c, const int32_t* S, const int32_t* W, size_t n) { LV_CHECK_CTX(c); return c->vol.tsdf_load(c->stream, S, W, n); }
int lv_tsdf_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.tsdf_clear(c->stream); }
int lv_tsdf_get_params(lv_ctx* c, lv_tsdf_params* out) { LV_CHECK_CTX(c); return c->vol.tsdf_get_params(out); }
int lv_tsdf_mesh_build(lv_ctx* c, int min_weight, uint64_t counts[4]) { LV_CHECK_CTX(c); return c->vol.mesh_build(c->stream, min_weight, counts); }
int lv_tsdf_mesh_fetch(lv_ctx* c, float* xyz, int32_t* sub, uint32_t* tri, size_t cap_vertices, size_t cap_triangles) {
    LV_CHECK_CTX(c);
    return c->vol.mesh_fetch(c->stream, xyz, sub, tri, cap_vertices, cap_triangles);
}
int lv_tsdf_mesh_info(lv_ctx* c, lv_mesh_info* out) { LV_CHECK_CTX(c); return c->vol.mesh_info(out); }
int lv_tsdf_mesh_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.mesh_clear(c->stream); }

// ---- Depth fusion (lv_depth.hip): the arguments are judged before the context, as lv_colour_integrate's are
void lv_default_depth_params(lv_depth_params* p) { default_depth_params(p); }

int lv_depth_integrate(lv_ctx* c, const lv_depth_view* views, size_t n_views, const lv_depth_params* p, uint64_t stats[4]) {
    DepthRule q;
    DepthCam cams[DEPTH_MAX_VIEWS];
    if (int rc = depth_rule(views, n_views, p, &q, cams)) return rc;
    LV_CHECK_CTX(c);
    return c->vol.depth_integrate(c->stream, views, cams, q, stats);
}

// ---- Colour layer (lv_colour.hip): what needs no context is judged before it, the rest in VolumeTools
void lv_default_colour_params(lv_colour_params* p) { default_colour_params(p); }

int lv_colour_integrate(lv_ctx* c, const lv_camera_view* views, size_t n_views, const lv_colour_params* p, uint64_t stats[4]) {
    PaintRule q;
    PaintCam cams[PAINT_MAX_VIEWS];
    if (int rc = colour_rule(views, n_views, p, &q, cams)) return rc;
    LV_CHECK_CTX(c);
    return c->vol.colour_integrate(c->stream, views, cams, q, *p, stats);
}

int lv_colour_fetch(lv_ctx* c, uint32_t* sums, uint8_t* rgba, size_t capacity) {
    if (!sums && !rgba) { set_error("lv_colour_fetch: sums and rgba are both null"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.colour_fetch(c->stream, sums, rgba, capacity);
}

int lv_colour_load(lv_ctx* c, const uint32_t* sums, size_t n) {
    if (!sums) { set_error("lv_colour_load: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.colour_load(c->stream, sums, n);
}

int lv_colour_query(lv_ctx* c, const void* pts, size_t stride, size_t n, uint8_t* rgba) {
    if (n && (!pts || !rgba || stride < 12)) { set_error("lv_colour_query: bad point array (stride %zu) or null output", stride); return LV_EINVAL; }
    if (n > 0xFFFFFFF0ull / 4) { set_error("lv_colour_query: too many points"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.colour_query(c->stream, pts, stride, n, rgba);
}

int lv_colour_clear(lv_ctx* c) { LV_CHECK_CTX(c); return c->vol.colour_clear(c->stream); }

int lv_colour_info(lv_ctx* c, struct lv_colour_info* out) {
    if (!out) { set_error("lv_colour_info: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.colour_info(c->stream, out);
}

int lv_mesh_colours(lv_ctx* c, uint8_t* rgba, size_t cap_vertices) {
    if (!rgba) { set_error("lv_mesh_colours: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.mesh_colours(c->stream, rgba, cap_vertices);
}

// ---- Surface ray casting (lv_tsdf_ray.hip): the arguments are judged before the context, as lv_occ_raycast's are
void lv_default_surf_ray_params(lv_tsdf_ray_params* p) { default_tsdf_ray_params(p); }

int lv_surf_raycast(lv_ctx* c, const lv_tsdf_ray_params* p, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                    lv_tsdf_ray_result* out, float* normals, uint8_t* rgba) {
    if (const char* why = surf_check_params(p)) { set_error("lv_surf_raycast: %s", why); return LV_EINVAL; }
    if (n >= SURF_MAX_N) { set_error("lv_surf_raycast: too many rays"); return LV_EINVAL; }
    if (n && (!from || !to || !out || from_stride < 12 || to_stride < 12)) {
        set_error("lv_surf_raycast: bad point arrays (strides %zu, %zu) or null output", from_stride, to_stride);
        return LV_EINVAL;
    }
    LV_CHECK_CTX(c);
    return c->vol.tsdf_raycast(c->stream, *p, from, from_stride, to, to_stride, n, out, normals, rgba);
}

int lv_surf_raycast_views(lv_ctx* c, const lv_tsdf_ray_params* p, const lv_view* views, size_t n_views, lv_tsdf_ray_result* out, float* normals,
                          uint8_t* rgba, size_t capacity, uint64_t stats[4]) {
    if (const char* why = surf_check_params(p)) { set_error("lv_surf_raycast_views: %s", why); return LV_EINVAL; }
    if (!views || !out) { set_error("lv_surf_raycast_views: null argument"); return LV_EINVAL; }
    if (n_views < 1 || n_views > (size_t)OCC_MAX_VIEWS) { set_error("lv_surf_raycast_views: n_views = %zu: must be in 1..%d", n_views, OCC_MAX_VIEWS); return LV_EINVAL; }
    if (int rc = views_ok(views, n_views, "lv_surf_raycast_views: ", false, TSDF_MAX_RETURNS)) return rc;   // (t is not judged: lv_rules.hpp)
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) total += views[v].n;
    if (capacity < total) { set_error("lv_surf_raycast_views: room for %zu results needed", total); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.tsdf_raycast_views(c->stream, *p, views, n_views, out, normals, rgba, stats);
}

// ---- Surface registration (lv_surf_align.hip): the arguments are judged before the context, as the surface rays' are
void lv_default_surf_align_params(lv_surf_align_params* p) { default_surf_align_params(p); }

int lv_surf_sample(lv_ctx* c, int min_weight, const void* pts, size_t stride, size_t n, double* out, uint8_t* status) {
    if (int rc = surf_check_sample_args(min_weight, pts, stride, n, out, status)) return rc;
    LV_CHECK_CTX(c);
    return c->vol.surf_sample(c->stream, min_weight, pts, stride, n, out, status);
}

int lv_surf_align(lv_ctx* c, const lv_surf_align_params* params, const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses, size_t K,
                  lv_surf_align_result* results, int32_t best[2]) {
    lv_surf_align_params prm;
    default_surf_align_params(&prm);
    if (params) prm = *params;
    if (const char* why = surf_check_align_params(&prm)) { set_error("lv_surf_align: %s", why); return LV_EINVAL; }
    if (int rc = surf_check_align_args(src, stride, n_src, guesses, K, results, best)) return rc;
    LV_CHECK_CTX(c);
    return c->vol.surf_align(c->stream, prm, src, stride, n_src, guesses, K, results, best);
}

// ---- Submap merging (lv_surf_merge.hip)
void lv_default_surf_merge_params(lv_surf_merge_params* p) { default_surf_merge_params(p); }

int lv_surf_merge(lv_ctx* c, const lv_surf_submap* sub, const lv_graph_pose* pose, const lv_surf_merge_params* p, uint64_t stats[4]) {
    SurfMergeRule q;
    if (int rc = surf_merge_rule(sub, pose, p, &q)) return rc;
    LV_CHECK_CTX(c);
    return c->vol.surf_merge(c->stream, *sub, q, stats);
}

// ---- Rolling volumes (lv_grid.hpp's rule; lv_occupancy.hip, lv_tsdf.hip)
int lv_volume_recentre(lv_ctx* c, int volume, const int32_t shift[3], uint64_t stats[4]) {
    if (volume != LV_VOLUME_OCC && volume != LV_VOLUME_SURFACE) { set_error("lv_volume_recentre: volume %d: LV_VOLUME_OCC or LV_VOLUME_SURFACE", volume); return LV_EINVAL; }
    if (!shift) { set_error("lv_volume_recentre: null shift"); return LV_EINVAL; }
    for (int a = 0; a < 3; ++a)
        if (shift[a] < -GRID_SHIFT_LIMIT || shift[a] > GRID_SHIFT_LIMIT) { set_error("lv_volume_recentre: shift: each component within +-2^20 voxels"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return c->vol.recentre(c->stream, volume, shift, stats);
}

int lv_volume_shift_info(lv_ctx* c, lv_volume_shifts* out) {
    if (!out) { set_error("lv_volume_shift_info: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    c->vol.shift_info(out);
    return LV_OK;
}

// ---- NDT registration (lv_ndt.hip)
void lv_default_ndt_params(lv_ndt_params* p) { default_ndt_params(p); }
void lv_default_ndt_align_params(lv_ndt_align_params* p) { default_ndt_align_params(p); }

#define LV_NDT_BUILT(c) LV_REQUIRE((c)->ndt.built, LV_ESTATE, "no NDT target: call lv_ndt_build first")

// a build (p given) or an add (p NULL) once the arguments have been judged, from the caller's points or the map source (lv_maptools.hpp)
static int ndt_build_or_add(lv_ctx* c, const lv_ndt_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]) {
    const float4* d_orig;
    uint32_t n_ids, m;
    if (int rc = map_side(c).source(pts, &d_orig, &n_ids, &m)) return rc;
    const uint64_t more = pts ? (uint64_t)n : (uint64_t)n_ids;
    if (!p && c->ndt.n_given + more > NDT_MAX_POINTS) { set_error("lv_ndt_add: the target would hold more than 2^31 - 1 points"); return LV_EINVAL; }
    if (!pts) return c->ndt.build(c->stream, p, d_orig, n_ids, nullptr, 0, 0, stats);
    return c->ndt.build(c->stream, p, nullptr, 0, pts, stride, n, stats);
}

int lv_ndt_build(lv_ctx* c, const lv_ndt_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]) {
    if (const char* why = ndt_check_params(p)) { set_error("lv_ndt_build: %s", why); return LV_EINVAL; }
    if (const char* why = ndt_check_points(pts, stride, n)) { set_error("lv_ndt_build: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    return ndt_build_or_add(c, p, pts, stride, n, stats);
}

int lv_ndt_add(lv_ctx* c, const void* pts, size_t stride, size_t n, uint64_t stats[4]) {
    if (const char* why = ndt_check_points(pts, stride, n)) { set_error("lv_ndt_add: %s", why); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_NDT_BUILT(c);
    return ndt_build_or_add(c, nullptr, pts, stride, n, stats);
}

int lv_ndt_fetch(lv_ctx* c, int layer, void* out, size_t capacity) {
    if (!ndt_layer_width(layer)) { set_error("lv_ndt_fetch: layer %d: LV_NDT_COUNT .. LV_NDT_ICOV", layer); return LV_EINVAL; }
    if (!out) { set_error("lv_ndt_fetch: null output"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_NDT_BUILT(c);
    if (capacity < c->ndt.n_cells) { set_error("lv_ndt_fetch: room for nx * ny * nz = %zu voxels needed", c->ndt.n_cells); return LV_EINVAL; }
    return c->ndt.fetch(c->stream, layer, out);
}

int lv_ndt_align(lv_ctx* c, const lv_ndt_align_params* params, const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses, size_t K,
                 lv_ndt_result* results, int32_t best[2]) {
    lv_ndt_align_params prm;
    default_ndt_align_params(&prm);
    if (params) prm = *params;
    if (const char* why = ndt_check_align_params(&prm)) { set_error("lv_ndt_align: %s", why); return LV_EINVAL; }
    if (int rc = ndt_check_align_args(src, stride, n_src, guesses, K, results, best)) return rc;
    LV_CHECK_CTX(c);
    LV_NDT_BUILT(c);
    return c->ndt.align(c->stream, prm, src, stride, n_src, guesses, K, results, best);
}

int lv_ndt_info(lv_ctx* c, lv_ndt_target_info* out) {
    if (!out) { set_error("lv_ndt_info: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    *out = lv_ndt_target_info{};
    if (c->ndt.built) *out = c->ndt.info;
    return LV_OK;
}

int lv_ndt_clear(lv_ctx* c) {
    LV_CHECK_CTX(c);
    LV_HIP(hipStreamSynchronize(c->stream));
    c->ndt.release();
    return LV_OK;
}

// ---- Elevation map (lv_elevation.hip)
void lv_default_elevation_params(lv_elevation_params* p) { default_elevation_params(p); }

#define LV_ELEV_BUILT(c) LV_REQUIRE((c)->elev.built, LV_ESTATE, "no elevation map: call lv_elev_build first")

// (the arguments are judged before the context, as lv_occ_raycast's are).  The caller's points, or the map source (lv_maptools.hpp).
int lv_elev_build(lv_ctx* c, const lv_elevation_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]) {
    if (const char* why = elev_check_params(p)) { set_error("lv_elev_build: %s", why); return LV_EINVAL; }
    if (pts && stride < 12) { set_error("lv_elev_build: bad point array (stride %zu)", stride); return LV_EINVAL; }
    if (pts && n >= ELEV_MAX_N) { set_error("lv_elev_build: too many points"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    const float4* d_orig;
    uint32_t n_ids, m;
    if (int rc = map_side(c).source(pts, &d_orig, &n_ids, &m)) return rc;
    if (!pts) return c->elev.build(c->stream, *p, d_orig, n_ids, m, nullptr, 0, 0, stats);
    return c->elev.build(c->stream, *p, nullptr, 0, 0, pts, stride, n, stats);
}

int lv_elev_fetch(lv_ctx* c, int layer, void* out, size_t capacity) {
    if (!elev_layer_size(layer)) { set_error("lv_elev_fetch: layer %d: LV_ELEV_LO .. LV_ELEV_HEIGHT", layer); return LV_EINVAL; }
    if (!out) { set_error("lv_elev_fetch: null output"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_ELEV_BUILT(c);
    if (capacity < c->elev.n_cells) { set_error("lv_elev_fetch: room for nx * ny = %zu values needed", c->elev.n_cells); return LV_EINVAL; }
    return c->elev.fetch(c->stream, layer, out);
}

int lv_elev_query(lv_ctx* c, const void* pts, size_t stride, size_t n, float* height, int8_t* cls) {
    if (!height && !cls) { set_error("lv_elev_query: height and cls are both null"); return LV_EINVAL; }
    if (n && (!pts || stride < 12)) { set_error("lv_elev_query: bad point array (stride %zu)", stride); return LV_EINVAL; }
    if (n >= ELEV_MAX_N) { set_error("lv_elev_query: too many points"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    LV_ELEV_BUILT(c);
    return c->elev.query(c->stream, pts, stride, n, height, cls);
}

int lv_elev_info(lv_ctx* c, lv_elevation_info* out) {
    if (!out) { set_error("lv_elev_info: null argument"); return LV_EINVAL; }
    LV_CHECK_CTX(c);
    *out = lv_elevation_info{};
    if (!c->elev.built) return LV_OK;
    out->built = 1;
    out->nx = c->elev.grid.nx;
    out->ny = c->elev.grid.ny;
    out->from_map = c->elev.from_map;
    out->n_points = c->elev.n_points;
    out->params = c->elev.prm;
    return LV_OK;
}

int lv_elev_clear(lv_ctx* c) {
    LV_CHECK_CTX(c);
    LV_HIP(hipStreamSynchronize(c->stream));
    c->elev.release();
    return LV_OK;
}

}  // extern "C"
