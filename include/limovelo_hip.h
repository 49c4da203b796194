/*
 * limovelo_hip.h — C-ABI of the MI355X-native LIMO-Velo iterated-KF-update hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each
 * entry point names the reference interface it replaces (paths relative to the reference repo
 * Huguet57/LIMO-Velo).  The C++ shim classes `Mapper` / `Localizator` in
 * limo-velo_amd/host/ keep the reference's method names on top of these calls; INTEGRATION.md shows
 * the binding a maintainer adds to the ROS node.
 *
 * Conventions
 *   - every function returns an int status: LV_OK (0) or a negative LV_E* code; lv_last_error()
 *     returns a thread-local message for the last failure.  "No map yet" and "fewer than k map
 *     points" are NOT errors: they yield n_valid = 0, mirroring Mapper::match returning an empty
 *     vector (src/Modules/Mapper.cpp:42) and Localizator::correct returning early
 *     (src/Modules/Localizator.cpp:24).
 *   - point arrays are passed as (base pointer, stride in bytes, count); x,y,z are three consecutive
 *     floats at the start of each record.  stride = 32 accepts the reference's `Point` records
 *     (include/Headers/Objects.hpp:20-28: float x,y,z; double time; float intensity, range) as they
 *     lie in a PointVector; stride = 12 accepts packed xyz.
 *   - a context is single-caller and non-reentrant (the reference modules are singletons driven from
 *     one thread: src/main.cpp:52,128).  All device work of a context is issued on one HIP stream.
 *   - the HIP extension is mandatory: there is no CPU fallback behind this ABI.
 */
#ifndef LIMOVELO_HIP_H
#define LIMOVELO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LV_OK 0
#define LV_EINVAL (-1)   /* bad argument */
#define LV_EHIP (-2)     /* HIP runtime error (message in lv_last_error) */
#define LV_ENODEV (-3)   /* no usable GPU */
#define LV_ESTATE (-4)   /* call out of order (e.g. iterate before scan_set) */
#define LV_ERANGE (-5)   /* coordinates outside the supported voxel range */

#define LV_STATE_DOF 23
#define LV_SUMS_LEN 96   /* doubles in the per-pass reduction record (see lv_sums_layout below) */

typedef struct lv_ctx lv_ctx;

/* Hot-path keys of `struct Params` (include/Headers/Common.hpp:56-107; defaults from
 * config/params.yaml:32,46-53 and src/main.cpp:145), same names. */
typedef struct lv_params {
    int    MAX_NUM_ITERS;        /* 3  -> esekf maximum_iter; up to MAX_NUM_ITERS+1 measurement passes */
    int    NUM_MATCH_POINTS;     /* 5  (k of Nearest_Search and rows of the plane fit, Mapper.cpp:85-86, Utils.cpp:33; 3..8: every tuned
                                  *     path — one launch per pass, the benchmark — is built for 5, other values run a general build of
                                  *     the three-kernel pass with lanes_per_query 8; LV_EINVAL outside 3..8) */
    double MAX_DIST_PLANE;       /* 2.0 */
    float  PLANES_THRESHOLD;     /* 0.05 */
    int    estimate_extrinsics;  /* 0 */
    double LiDAR_noise;          /* 0.001 */
    double LIMITS[LV_STATE_DOF]; /* 23 x 0.001 */
    double degeneracy_threshold; /* 5.0 (config/params.yaml:52; kitti.yaml:46 = 400): used by degeneracy_mode 2 */
    /* ---- structure tuning (no reference counterpart) ---- */
    float  voxel_size;           /* level-0 cell edge of the voxel hash in metres (default 0.5) */
    int    lanes_per_query;      /* 1,2,4,8,16: lanes of a wavefront cooperating on one scan point (default 8) */
    /* ---- degeneracy stage of the fork's update_iterated_dyn_share_modified(R, degeneracy_threshold, solve_time,
     * print_degeneracy_values) (src/Modules/Localizator.cpp:132).  The fork's IKFoM source is absent, so
     * the stage is a HOOK with an opt-in restatement, off by default:
     *   0  off: esekf's plain iterated update (every parity and benchmark run); lv_create warns once on stderr if
     *      degeneracy_threshold was changed from its default, because it then has no effect;
     *   1  the eigenvalues of the 6x6 pose block of H^T H are computed every pass and kept for
     *      lv_get_degeneracy_values ("print the degeneracy eigenvalues to guess what the threshold must be",
     *      config/params.yaml:53); the update itself is unchanged;
     *   2  [UNKNOWN-FORK, plausible restatement] solution remapping (Zhang, Kaess, Singh, ICRA 2016) in information
     *      form: measurement information along pose eigen-directions whose eigenvalue is below degeneracy_threshold is
     *      removed before the gain is formed; those directions keep their propagated value.
     * print_degeneracy_values != 0 (with mode >= 1) also prints the eigenvalues of every pass to stderr. */
    int    degeneracy_mode;
    int    print_degeneracy_values;
} lv_params;

/* state_ikfom of the IKFoM fork (field order evidenced by src/Objects/State.cpp:53-61 and
 * src/Modules/Localizator.cpp:137-150).  Quaternions in Eigen coefficient order x,y,z,w.
 * 26 doubles, no padding. */
typedef struct lv_state {
    double pos[3];
    double rot[4];
    double offset_R_L_I[4];
    double offset_T_L_I[3];
    double vel[3];
    double bg[3];
    double ba[3];
    double grav[3];
} lv_state;

/* Result of one measurement-model evaluation: what esekf needs from the N-sized data
 * (SURVEY §8 a-8): H^T H (12x12 row-major), H^T h, sum h^2, number of chosen matches. */
typedef struct lv_sums {
    double  HTH[144];
    double  HTh[12];
    double  sum_h2;
    int64_t n_valid;
} lv_sums;

/* Device-side record layout of the LV_SUMS_LEN doubles that lv_pass_reduce() produces and that is
 * all-reduced (sum) across GPUs: [0..77] upper triangle of H^T H row by row, [78..89] H^T h,
 * [90] n_valid (as double), [91] sum h^2, [92..95] zero padding. */

void        lv_default_params(lv_params* p);
const char* lv_last_error(void);
const char* lv_version(void);

/* ---- context -------------------------------------------------------------------------------- */
/* device = HIP device ordinal.  Replaces the construction of the Mapper / Localizator singletons
 * (include/Headers/Mapper.hpp:35-38, src/Modules/Localizator.cpp:100-117 init_IKFoM). */
int  lv_create(const lv_params* params, int device, lv_ctx** out);
void lv_destroy(lv_ctx* ctx);
/* Issue all work on an existing hipStream_t (e.g. torch's current stream); NULL = context's own. */
int  lv_set_stream(lv_ctx* ctx, void* hip_stream);
void* lv_get_stream(lv_ctx* ctx);
int  lv_synchronize(lv_ctx* ctx);

/* ---- Mapper side ---------------------------------------------------------------------------- */
/* KD_TREE<Point>::Build(PointVector)              — call site src/Modules/Mapper.cpp:68-71 */
int    lv_map_build(lv_ctx* ctx, const void* points, size_t stride, size_t n);
/* Mapper::add(points, time, downsample) — src/Modules/Mapper.cpp:19-30: on an empty map the points BUILD it
 * (KD_TREE::Build, no down-sampling), otherwise KD_TREE<Point>::Add_Points(PointVector&, bool) — call site
 * src/Modules/Mapper.cpp:73-76.  downsample != 0 applies ikd-Tree's box rule with box_length 0.2 m (Mapper.cpp:65),
 * evaluated exactly as upstream's sequential loop would: in every 0.2 m box touched by new points only the point
 * nearest to the box centre survives (occupants must be strictly closer to beat a new point).  The map afterwards is
 * [surviving old points, old order] + [surviving new points, input order] — the index space of lv_fetch_knn.
 * INCREMENTAL: only the neighbourhood buckets / voxel lists that contain a new or a deleted point are touched
 * (appends into slack, tombstones); the structure is re-linearised (ids compacted, everything rebuilt) when a pool,
 * a table or the share of dead ids runs high — see lv_map_get_stats. */
int    lv_map_add(lv_ctx* ctx, const void* points, size_t stride, size_t n, int downsample);
/* The mapping step of the main loop without leaving the device (src/main.cpp:92,102):
 *     Points global_ds_compensated = Xt2 * Xt2.I_Rt_L() * ds_compensated;   map.add(global_ds_compensated, t2, true);
 * the current scan (lv_scan_set / lv_scan_deskew*) is moved to the world with the state the device holds — the
 * resident filter's (lv_filter_set / lv_predict / lv_correct) if there is one, otherwise the result of the last
 * lv_update — in f32 exactly as State::State(const state_ikfom&) + RotTransl do (rows a-1), and inserted in scan
 * order.  Non-finite points are skipped.  The insert is enqueued and runs BESIDE whatever the caller enqueues next (on a
 * second stream of the context, when the context owns its stream): every call that touches the map waits for it first, so
 * the only visible effect is that lv_map_add / lv_map_add_scan return before the map has changed. */
int    lv_map_add_scan(lv_ctx* ctx, int downsample);
/* Rolling window (BASELINE configs[4]; ikd-Tree's Delete_Point_Boxes, which the reference never calls —
 * README.md:127 — but a bounded map needs): keep_inside != 0 removes every point OUTSIDE the axis-aligned box
 * [lo, hi], keep_inside == 0 every point INSIDE it.  lv_map_evict_oldest removes the n_oldest oldest living points
 * (map order = age).  Indices of the survivors shift down as in any deletion (lv_fetch_knn reports ranks among
 * the living). */
int    lv_map_evict_box(lv_ctx* ctx, const float lo[3], const float hi[3], int keep_inside, size_t* n_evicted);
int    lv_map_evict_oldest(lv_ctx* ctx, size_t n_oldest, size_t* n_evicted);
/* Force the periodic re-linearisation now (compaction of the ids + rebuild of every bucket). */
int    lv_map_relinearise(lv_ctx* ctx);
/* The same compaction + rebuild WITHOUT stopping the world (round 5).  ikd-Tree rebuilds unbalanced sub-trees on a second thread
 * while searches go on (the tree the reference constructs with delete / balance criteria 0.3 / 0.6, src/Modules/Mapper.cpp:65);
 * here a compacted copy of the living points is rebuilt by a worker thread on a stream of its own while searches and inserts
 * keep using the active structure, the inserts / evictions of the meantime are replayed on the copy, and the two are swapped
 * at the first map call after the worker has caught up (a cycle boundary of src/main.cpp:75-103).  Point set, id order and
 * every search result are those of lv_map_relinearise.  lv_map_add / lv_map_add_scan start one by themselves when a third of
 * the id space is dead and the map holds >= 200 000 points (lv_set_option "async_relinearise" 0: always the stop-the-world
 * form; "async_relinearise_min": the size threshold).  Returns at once. */
int    lv_map_relinearise_async(lv_ctx* ctx);
/* Set-up time (round 6): allocate — and touch — everything a background rebuild of the map as it stands needs (the second store's
 * id buffers, pools and tables at the sizes a rebuild takes, the journal arena), by one synchronous rebuild of a snapshot that is
 * then discarded.  Without it the FIRST background rebuild of a context spends its opening ~80 cycles of a 100 Hz stream in
 * hipMalloc on the worker thread (a 10 M-point map: ~20 GB); later ones find the previous active store waiting either way.  The
 * price is the second store's memory from the start instead of from the first rebuild.  Blocks; LV_ESTATE while a rebuild is in
 * flight.  (The reference's counterpart: ikd-Tree's rebuild thread allocates its Rebuild_PCL_Storage on demand.) */
int    lv_map_reserve_rebuild(lv_ctx* ctx);
/* out = {state, rebuilds started, rebuilds adopted, journaled operations not yet replayed}; wait != 0: block until a rebuild in
 * flight has been adopted.  States: 0 idle; 4 the worker is allocating the second store; 5 allocated, waiting for the snapshot the
 * next map call enqueues; 1 rebuilding / replaying the journal; 2 rebuilt and waiting to be adopted; 3 failed (the next map call
 * reports it on stderr, keeps the map as it is and switches this context to stop-the-world re-linearisations).  "In flight" is any
 * state other than 0 and 3. */
int    lv_map_rebuild_status(lv_ctx* ctx, int wait, uint64_t out[4]);
/* KD_TREE<Point>::size()                          — src/Modules/Mapper.cpp:33,79 */
size_t lv_map_size(lv_ctx* ctx);
/* Copy the current map points (xyz packed, map order = the index space of lv_fetch_knn). */
int    lv_map_fetch(lv_ctx* ctx, float* xyz_out, size_t capacity);
typedef struct lv_map_stats {
    uint64_t living, ids, capacity;          /* points alive / ids handed out since the last re-linearisation / id slots allocated */
    uint64_t pool_used[4], pool_cap[4];      /* entries of [0] the level-0 bucket pool, [1] the voxel-list pool ([2], [3] unused since the
                                                single-replicated-level map of round 6; rounds 1-5: three bucket pools + the lists) */
    uint64_t slots_used[4], slots_cap[4];    /* occupied / total slots of [0] the bucket table, [1] the voxel-list table */
    uint64_t tombstones, dropped;            /* dead bucket entries since the last rebuild; points refused (non-finite / out of range) */
    uint64_t relinearisations, incremental_adds;
    uint64_t bytes;                          /* device memory held by the map */
} lv_map_stats;
int    lv_map_get_stats(lv_ctx* ctx, lv_map_stats* out);

/* ---- Map queries ------------------------------------------------------------------------------
 * ikd-Tree's search calls on the device map, for arbitrary points (the KF update's own search stays inside lv_update /
 * lv_iterate).  Common rules: queries are map-frame points, f32 x,y,z at offset 0 of each record (stride >= 12, as lv_map_add);
 * results go to host pointers and are written when the call returns; a call is ordered behind every earlier map mutation (an
 * insert still in flight on the side stream included) and, during a background rebuild, reads the active store.  Indices are
 * ranks among the living points (the index space of lv_map_fetch / lv_fetch_knn); distances are the reference's calc_dist
 * (f32 squared distance, summed left to right, unfused).  An empty map gives LV_OK with nothing found. */
/* KD_TREE<Point>::Nearest_Search(point, k, Nearest_Points, Point_Distance, max_dist), batched over n queries.  k in 1..32;
 * row i of idx / d2 (n x k) holds query i's neighbours in ascending (d2, index) order, unfilled slots idx = 0xFFFFFFFF and
 * d2 = +inf; found[i] = the filled slots.  A point is admitted iff d2 <= max_dist * max_dist (f32 product; +inf: no limit;
 * negative or NaN: LV_EINVAL).  A query with a non-finite coordinate finds nothing.  Exact for every query (beyond the voxel
 * range by brute force).  d2 and found may be NULL. */
int lv_map_knn(lv_ctx* ctx, const void* q, size_t stride, size_t n, int k, float max_dist, uint32_t* idx, float* d2, int32_t* found);
/* KD_TREE<Point>::Radius_Search(point, radius, Storage), batched, CSR output: query i's points are idx[offsets[i] ..
 * offsets[i + 1]) in ascending index order, every living point with d2 <= radius * radius (f32).  offsets holds n + 1 entries,
 * *total = offsets[n].  idx == NULL: count only (offsets and *total are written).  capacity < *total: LV_EINVAL, offsets and
 * *total still written.  Offsets are 64-bit: the count-only call reports any total; one fill returns at most 2^31 - 1 results
 * (a larger total is LV_EINVAL, offsets and *total still written: split the queries).  n < 2^31 - 1.  d2 may be NULL. */
int lv_map_radius_search(lv_ctx* ctx, const void* q, size_t stride, size_t n, float radius, size_t* offsets, uint32_t* idx, float* d2,
                         size_t capacity, size_t* total);
/* KD_TREE<Point>::Box_Search(BoxPointType, Storage): the living points inside [lo, hi] with lv_map_evict_box's predicate (both
 * faces inclusive) in ascending index order — exactly what lv_map_evict_box(lo, hi, keep_inside = 0) would remove.  xyz: 3
 * floats per point, may be NULL; idx and xyz both NULL: count only.  Capacity as in lv_map_radius_search (*n_out = the count). */
int lv_map_box_search(lv_ctx* ctx, const float lo[3], const float hi[3], uint32_t* idx, float* xyz, size_t capacity, size_t* n_out);

/* ---- Multi-hypothesis updates ----------------------------------------------------------------
 * Prelocalisation in a previously saved map (the reference's work in progress, README.md:64-67, and its TODO "Saving and loading
 * HD-Maps", README.md:117): many candidate poses evaluated or refined against the current scan in one call, in a number of launches
 * per pass that does not depend on m.  Hypothesis i is exactly the single-pose call from xs[i] (Localizator.cpp:132 per
 * hypothesis: same lv_params, same convergence rule, its own number of passes).  Both calls use the context's current scan, are
 * ordered behind every earlier map mutation, read the active store during a background rebuild, and return once the host arrays
 * are written.  m == 0 is a no-op; no map or an empty scan leaves every state unchanged (passes 0, n_valid 0); a context with a
 * multi-GPU communicator gives LV_ESTATE.  The resident filter, the per-point capture of the last single-pose call,
 * lv_last_passes, the degeneracy values and the timing records are left as they were.  Large batches run in chunks of
 * hypotheses (lv_set_option "batch_chunk_hypotheses" caps a chunk); results do not depend on the chunking. */
/* m measurement-model evaluations (lv_iterate) of the current scan, one per state, in one call. */
int lv_iterate_batch(lv_ctx* ctx, const lv_state* xs, size_t m, lv_sums* out);
/* m independent iterated updates (lv_update), each from prior xs[i] with the shared prior covariance P (23x23 row-major).
 * xs is updated in place.  P_out (NULL or m x 529), passes (NULL or m) and last (NULL or m: the sums of each hypothesis'
 * last pass, i.e. lv_update's per_pass[passes-1], the fitness a caller ranks by) are optional. */
int lv_update_batch(lv_ctx* ctx, lv_state* xs, size_t m, const double* P, double* P_out, int* passes, lv_sums* last);

/* ---- Dynamic-point removal -------------------------------------------------------------------
 * The reference's open TODO (README.md, "Fixes to investigate": "Try to add a module for removing dynamic objects such as people
 * or vehicles", "Erase unused (potentially dangerous) points in the map"): map points that a sensor has seen THROUGH leave the map.
 * A view is one sweep: its pose sensor -> world (R 3x3 row-major, t; the caller forms Xt2 * Xt2.I_Rt_L() as lv_map_add_scan does)
 * and its raw returns in the sensor frame (f32 x,y,z at offset 0 of each record, stride >= 12).  Per view:
 *   1. range image of height x width pixels: column from atan2f(y, x), width equal bins over [-pi, pi); row from
 *      atan2f(z, sqrtf(x*x + y*y)), height equal bins over [v_min_deg, v_max_deg]; a pixel keeps the minimum range
 *      sqrtf(x*x + y*y + z*z) of its returns.  Returns that are non-finite, at range <= min_range or outside the rows are ignored;
 *      an empty pixel is +inf.
 *   2. every pixel becomes the minimum over the (2 window + 1)^2 pixels around it (columns wrap at +-pi, rows are clipped); an
 *      all-empty window stays +inf: no evidence.
 *   3. a living map point p, in the sensor frame p_s = R^T (p - t), at range r = |p_s| inside [min_range, max_range] and inside the
 *      rows, is SEEN THROUGH iff r_img - r > fmaxf(margin_abs, margin_rel * r), r_img the filtered pixel it falls in.
 * A point leaves the map iff it was seen through in at least min_hits views: a pure function of its coordinates and the call's
 * inputs.  Survivors keep their order (as with lv_map_evict_box).  The call is ordered behind every earlier map mutation, acts on
 * the active store (a background rebuild in flight replays it on its copy) and returns once its host outputs are written. */
typedef struct lv_view {            /* one sweep: pose sensor -> world, returns in the sensor frame */
    float R[9]; float t[3];
    const void* points; size_t stride; size_t n;    /* n = 0: the view gives no evidence */
} lv_view;
typedef struct lv_visibility_params {
    int   width, height;            /* image columns over [-pi, pi), rows over [v_min_deg, v_max_deg]; width * height <= 2^20 */
    float v_min_deg, v_max_deg;     /* v_min_deg < v_max_deg, both in [-90, 90] */
    float min_range, max_range;     /* map points judged only inside; scan returns <= min_range ignored; 0 < min_range < max_range */
    float margin_abs, margin_rel;   /* finite, > 0 */
    int   window;                   /* half-width w of the window-min, 0..8 */
    int   min_hits;                 /* 1..n_views */
    int   dry_run;                  /* != 0: classify only, the map is not touched */
} lv_visibility_params;
/* Defaults for a 64-ring spinning LiDAR: 2048 x 64 pixels over -25..+3 deg, ranges 1..80 m, margins 0.3 m and 2 %, window 1,
 * min_hits 1, dry_run 0. */
void lv_default_visibility_params(lv_visibility_params* p);
/* n_views 1..32.  hits: NULL, or lv_map_size() entries in map order (the index space of lv_map_fetch / lv_map_knn): the number of
 * views each point was seen through in, as the map stood BEFORE the removal.  *n_removed (may be NULL): the points that left the
 * map (0 with dry_run).  Arguments outside the limits above give LV_EINVAL and change nothing; an empty map gives LV_OK, 0 removed. */
int  lv_map_remove_dynamic(lv_ctx* ctx, const lv_view* views, size_t n_views, const lv_visibility_params* p, uint8_t* hits,
                           size_t* n_removed);

/* ---- Map painting ----------------------------------------------------------------------------
 * The reference's open TODO (README.md, "Fixes to investigate": "Add vision buffer and ability to paint the map's points"): every
 * living map point takes the colour of the camera images that see it.  A view is one image with its pinhole camera and its pose
 * camera -> world (R row-major, t; camera frame x right, y down, z forward).  For every living point p and every view:
 *   1. p_c = R^T (p - t), each component summed left to right without fusing (as lv_map_remove_dynamic); z = p_c.z.  The point is
 *      judged only if min_depth <= z <= max_depth.
 *   2. x = X / z, y = Y / z; only if x*x + y*y <= max_norm_radius^2 (f32; outside it plumb_bob may fold over).
 *   3. plumb_bob as OpenCV's projectPoints: r2 = x*x + y*y, c = 1 + k1 r2 + k2 r2^2 + k3 r2^3,
 *      xd = x c + 2 p1 x y + p2 (r2 + 2 x^2), yd = y c + p1 (r2 + 2 y^2) + 2 p2 x y; u = fx xd + cx, v = fy yd + cy; only if
 *      0 <= u <= width - 1 and 0 <= v <= height - 1 (integer pixel coordinates are pixel centres).
 *   4. occlusion buffer of ceil(width / s) x ceil(height / s) cells, s = zbuf_scale: a point falls in cell
 *      (floor((u + 0.5) / s), floor((v + 0.5) / s)); a cell keeps the minimum z of the map's own points that pass 1-3 (empty: +inf).
 *      Then every cell becomes the minimum over the (2 window + 1)^2 cells around it, clipped at the buffer's edge.
 *   5. the point is SEEN by the view iff z - zbuf(cell) <= fmaxf(margin_abs, margin_rel * z): the foremost point of a cell always is.
 *   6. its sample: the image bilinearly at (u, v) in f32, per channel 0..255, taps clamped to the image (MONO8: r = g = b).
 * A pure function of the living points' coordinates and the call's inputs: no float atomics, bitwise reproducible. */
enum { LV_IMAGE_RGB8 = 0, LV_IMAGE_BGR8 = 1, LV_IMAGE_MONO8 = 2 };   /* the ROS encodings rgb8 / bgr8 / mono8 */
typedef struct lv_camera_view {
    float R[9]; float t[3];          /* pose camera -> world, R row-major; camera frame x right, y down, z forward (OpenCV) */
    float fx, fy, cx, cy;            /* pinhole, pixels; integer pixel coordinates are pixel centres */
    float dist[5];                   /* k1, k2, p1, p2, k3 (OpenCV plumb_bob); all zero: no distortion */
    int   width, height;             /* 1..8192 each, width * height <= 2^24; all views of a call together <= 2^26 pixels */
    int   format;                    /* LV_IMAGE_* */
    const void* image; size_t row_stride;   /* bytes between rows, >= width * channels */
} lv_camera_view;
typedef struct lv_paint_params {
    float min_depth, max_depth;      /* 0 < min_depth < max_depth: only points with z in [min_depth, max_depth] are judged */
    float max_norm_radius;           /* > 0: points whose undistorted sqrt(x^2 + y^2) (x = X/Z, y = Y/Z) exceeds it are not projected */
    int   zbuf_scale;                /* 1..16: one occlusion cell per zbuf_scale x zbuf_scale pixels */
    int   window;                    /* 0..8: half-width of the occlusion window-min (clipped at the edges, no wrap) */
    float margin_abs, margin_rel;    /* finite, > 0 */
    int   blend;                     /* 0: mean over the views that see the point, 1: the nearest such view (ties: lower index) */
} lv_paint_params;
/* Defaults: depth 0.3..60 m, max_norm_radius 1.5, zbuf_scale 4, window 1, margins 0.1 m and 1 %, blend 0. */
void lv_default_paint_params(lv_paint_params* p);
/* n_views 1..32.  Outputs, each may be NULL, lv_map_size() entries in map order (the index space of lv_map_fetch / lv_map_knn):
 *   n_seen[i]        the number of views that see point i;
 *   rgb[3i .. 3i+2]  blend 0: the seeing views' samples summed in view order, then divided by n_seen[i];
 *                    blend 1: the sample of the seeing view with the smallest z (ties: the lower view index);
 *   depth[i]         the smallest z among the seeing views.
 * A point no view sees: rgb 0, depth +inf, n_seen 0.  Arguments outside the limits above (a non-finite pose or intrinsic, a NULL
 * image, a format outside LV_IMAGE_* included) give LV_EINVAL and write nothing; an empty or unbuilt map gives LV_OK.  Read-only:
 * ordered behind every earlier map mutation like lv_map_knn, reads the active store during a background rebuild (nothing is
 * journaled) and returns once the host outputs are written. */
int  lv_map_paint(lv_ctx* ctx, const lv_camera_view* views, size_t n_views, const lv_paint_params* p,
                  float* rgb, float* depth, uint8_t* n_seen);

/* ---- Surface normals and outlier removal ---------------------------------------------------------
 * The local surface of the device map: a normal and a curvature per living point, and the removal of points that have no
 * surface around them (the reference's open TODO "Erase unused (potentially dangerous) points in the map"; PCL's
 * NormalEstimation, StatisticalOutlierRemoval and RadiusOutlierRemoval).  Both are one computation over the map's own points.
 *
 * Neighbourhood of a living point p for k and max_dist: N(p) = what lv_map_knn returns for the query p with this k and
 * max_dist: the up to k living points with the smallest (calc_dist f32, id), admitted iff d2 <= max_dist * max_dist (f32).  p is
 * a map point, so it is in N(p) with d2 = 0 (PCL's convention for a cloud searched against itself).  n = |N(p)|.
 *
 * lv_map_normals, per living point (k 2..32, max_dist > 0 finite, min_neighbours 3..k, orient 0 or 1, viewpoint finite):
 *   offsets  o_j = (double)x_j - (double)p per axis (exact in f64), in neighbour order j = 0..n-1;
 *            mean = (sum o_j) / n;  C = (sum (o_j - mean)(o_j - mean)^T) / n; all f64, summed in neighbour order, unfused.
 *   normal   the unit eigenvector of the smallest eigenvalue l0 <= l1 <= l2 of C (f64), rounded to f32 once at the end.
 *            curvature = (float)(l0 / (l0 + l1 + l2)) (PCL's surface variation), 0 when the trace is 0.
 *   sign     orient 0: the component of largest magnitude is positive (ties: the lower axis); orient 1: towards viewpoint,
 *            normal . (viewpoint - p) >= 0 in f64, the orient-0 rule when that dot product is 0.
 *   n < min_neighbours: normal (0, 0, 0), curvature NaN.  n_used = n always.
 *   mean_dist = (float)((sum_j sqrt((double)d2_j)) / (n - 1)), +inf when n = 1 (the point's own 0 is in the sum).
 *
 * lv_map_remove_outliers:
 *   mode 0   statistical (k 1..31, max_dist > 0 finite, std_mul finite): d(p) = the f64 mean distance above over k + 1
 *            neighbours (p and k others).  A point with fewer than k others inside max_dist has d = +inf: it is an outlier and
 *            takes no part in the statistics.  Over the n_f points with finite d: mu = sum d / n_f,
 *            sigma = sqrt(sum (d - mu)^2 / (n_f - 1)) (two passes, f64; the order of the two sums is the implementation's),
 *            threshold = mu + std_mul * sigma.  Outlier iff d > threshold.  stats = {mu, sigma, threshold}.
 *   mode 1   radius (radius > 0 finite, min_neighbours >= 1): outlier iff the number of OTHER living points with
 *            d2 <= radius * radius (f32, as above) is below min_neighbours.  Exact; stats = {0, 0, 0}.
 * Outliers leave the map like the points of lv_map_remove_dynamic (survivors keep their order), unless dry_run != 0.  The call
 * is ordered behind every earlier map mutation and acts on the active store; a background rebuild in flight replays the
 * RESOLVED rule (mode 0: the threshold the active store computed) on its copy, so the same points go. */
typedef struct lv_surface_params {
    int    k;                   /* 2..32 neighbours, the point itself included */
    float  max_dist;            /* > 0, finite */
    int    min_neighbours;      /* 3..k */
    int    orient;              /* 0: largest component positive, 1: towards viewpoint */
    double viewpoint[3];        /* orient 1 only; finite */
} lv_surface_params;
typedef struct lv_outlier_params {
    int    mode;                /* 0 statistical, 1 radius */
    int    k;                   /* mode 0: 1..31 other neighbours */
    float  max_dist;            /* mode 0: > 0, finite */
    float  std_mul;             /* mode 0: finite */
    float  radius;              /* mode 1: > 0, finite */
    int    min_neighbours;      /* mode 1: >= 1 */
    int    dry_run;             /* != 0: classify only, the map is not touched */
} lv_outlier_params;
/* Defaults: k 10, max_dist 2 m, min_neighbours 5, orient 0, viewpoint 0. */
void lv_default_surface_params(lv_surface_params* p);
/* Defaults: mode 0, k 10, max_dist 2 m, std_mul 2, radius 0.5 m, min_neighbours 5, dry_run 0. */
void lv_default_outlier_params(lv_outlier_params* p);
/* Outputs, each may be NULL, `capacity` entries of room, lv_map_size() written in map order (the index space of lv_map_fetch /
 * lv_map_knn): normals[3i .. 3i+2], curvature[i], mean_dist[i], n_used[i].  Parameters outside the limits, a NULL params or
 * capacity < lv_map_size() give LV_EINVAL and write nothing; an empty or unbuilt map gives LV_OK.  Read-only, ordered like
 * lv_map_knn. */
int  lv_map_normals(lv_ctx* ctx, const lv_surface_params* p, float* normals, float* curvature, float* mean_dist, int32_t* n_used,
                    size_t capacity);
/* flags: NULL, or lv_map_size() entries in map order as the map stood BEFORE the removal, 1 = outlier.  *n_removed (may be NULL):
 * the points that left the map (0 with dry_run).  stats: NULL or 3 doubles.  Parameters outside the limits or a NULL params give
 * LV_EINVAL and change nothing; an empty or unbuilt map gives LV_OK, 0 removed. */
int  lv_map_remove_outliers(lv_ctx* ctx, const lv_outlier_params* p, uint8_t* flags, size_t* n_removed, double* stats);

/* ---- Map clustering ------------------------------------------------------------------------------
 * Which points of the device map belong together (PCL's EuclideanClusterExtraction), and the removal of whole clusters: the
 * complement of the two point-by-point removals above.  lv_map_remove_dynamic takes only the points of an object a later sweep
 * saw through (the reference's open TODO "Try to add a module for removing dynamic objects such as people or vehicles"): its
 * hits, grown to the connected object, take the shell along.  lv_map_remove_outliers keeps a small blob that supports itself:
 * components below a size are the rule that removes it.
 *
 * Definition.  Two living map points a, b are ADJACENT iff calc_dist(a, b) <= radius * radius: the f32, left-to-right, unfused
 * squared distance and the comparison of lv_map_radius_search (the product radius * radius in f32).  The rule is symmetric and
 * duplicates are adjacent.  A CLUSTER is a connected component of that graph over the INCLUDED points: every living point when
 * mask == NULL, otherwise the points whose mask byte is non-zero (mask: lv_map_size() bytes in map order, the order of
 * lv_map_fetch).  An excluded point links nothing and has label -1.
 * Components with fewer than min_size points, or with more than max_size points when max_size != 0, are not reported: their
 * points have label -1.  The reported clusters are numbered 0 .. C-1 by size descending (the order PCL returns them in), ties to
 * the cluster whose first member in map order comes first.  Partition and labels are exactly defined: a pure function of the
 * living points, the mask and the parameters, bitwise reproducible.
 *
 * lv_map_cluster is read-only and ordered like lv_map_knn: it sees every earlier insert, eviction and rebuild, and reads the
 * active store while a background rebuild runs.
 * lv_map_remove_clusters removes whole components (survivors keep their order, as with lv_map_remove_outliers):
 *   seeds == NULL  debris: every included point of a component with fewer than min_size points leaves the map; max_size is ignored.
 *   seeds != NULL  object growth (seeds: lv_map_size() bytes in map order): every component whose size is within
 *                  [min_size, max_size] (max_size 0: no upper limit) and that holds at least one seeded INCLUDED point leaves
 *                  the map whole.  max_size keeps a seed on a wall from removing the wall.
 * Excluded points are never removed.  With dry_run != 0 the map is not touched.
 * Background rebuild: mask and seeds are per-point arrays in the active store's order, so the removal is NOT journaled.  A
 * call that removes (dry_run == 0) instead WAITS until a background rebuild in flight (lv_map_relinearise_async) has landed and
 * been adopted, everything journaled before it included, and then acts on that store: no removal is lost, and the map order the
 * caller's arrays refer to is kept by the adoption.  The wait is the rest of that rebuild (lv_map_rebuild_status tells whether
 * one is running): a caller on the 100 Hz cycle should issue the removal when none is, or expect this call to take that long.
 * lv_map_cluster and a dry run never wait. */
typedef struct lv_cluster_params {
    float    radius;     /* > 0, finite */
    uint32_t min_size;   /* >= 1 */
    uint32_t max_size;   /* 0: no limit */
    int      dry_run;    /* lv_map_remove_clusters: != 0: classify only, the map is not touched */
} lv_cluster_params;
/* Defaults: radius 0.5 m, min_size 1, max_size 0, dry_run 0. */
void lv_default_cluster_params(lv_cluster_params* p);
/* labels: NULL (count only), or `capacity` entries of room, lv_map_size() written in map order (capacity < lv_map_size():
 * LV_EINVAL).  sizes: NULL, or the first min(C, sizes_capacity) cluster sizes in label order.  *n_clusters (may be NULL) = C.
 * Parameters outside the limits or a NULL params give LV_EINVAL and write nothing; an empty or unbuilt map gives LV_OK, C = 0,
 * nothing else written. */
int  lv_map_cluster(lv_ctx* ctx, const lv_cluster_params* p, const uint8_t* mask, int32_t* labels, size_t capacity, uint32_t* sizes,
                    size_t sizes_capacity, size_t* n_clusters);
/* flags: NULL, or lv_map_size() entries in map order as the map stood BEFORE the removal, 1 = the point left (with dry_run:
 * would leave).  *n_removed (may be NULL): the points that left the map (0 with dry_run).  Parameters outside the limits or a
 * NULL params give LV_EINVAL and change nothing; an empty or unbuilt map gives LV_OK, 0 removed. */
int  lv_map_remove_clusters(lv_ctx* ctx, const lv_cluster_params* p, const uint8_t* mask, const uint8_t* seeds, uint8_t* flags,
                            size_t* n_removed);

/* ---- Plane segmentation ---------------------------------------------------------------------------
 * The dominant planes of the device map and the points that lie on them (PCL's SACSegmentation with SACMODEL_PLANE, and its
 * axis-constrained forms SACMODEL_PERPENDICULAR_PLANE / SACMODEL_PARALLEL_PLANE): "the floor is this plane, these points belong
 * to it, those are the walls".  lv_map_planes extracts up to max_planes planes from the living points, one after the other;
 * each plane's members leave the candidates of the next.  The result is exactly defined: a pure function of the living points
 * in map order, the mask and the parameters, bitwise reproducible.  The map is read, never changed.
 *
 * 1. Candidates.  Round r = 0, 1, ...: the INCLUDED living points (mask == NULL: all; otherwise those whose mask byte is
 *    non-zero, as in lv_map_cluster) that no earlier plane has taken, in map order, c[0 .. n).  n < 3 or n < min_inliers: stop.
 * 2. Draws.  Hypothesis h (0 .. iterations-1) of round r draws i_j = umulhi64(u_j, n), j = 0, 1, 2, with
 *    u_j = mix(seed ^ mix((r << 40) | (h << 8) | j)) and mix(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) *
 *    0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31) (splitmix64), all in 64 bits.  Two equal draws
 *    make the hypothesis invalid.
 * 3. Plane of a hypothesis, p_j = c[i_j], in f64, unfused, in the order written: u = p1 - p0, v = p2 - p0, c = u x v
 *    (cx = uy vz - uz vy, cy = uz vx - ux vz, cz = ux vy - uy vx); cc = (cx^2 + cy^2) + cz^2, uu and vv likewise.  Invalid iff
 *    !(cc > 1e-12 * (uu * vv)) (a sliver).  n^ = c / sqrt(cc), per component.  Sign: constraint 1: n^ . a^ >= 0 for the
 *    normalised axis a^ (dot product (x + y) + z); otherwise, and when that dot product is 0, the component of largest
 *    magnitude is positive, ties to the lower axis (the orient-0 rule of lv_map_normals).  Constraint, on
 *    t = |(n^x a^x + n^y a^y) + n^z a^z|: constraint 1 needs t >= cos(max_angle), constraint 2 needs t <= sin(max_angle),
 *    otherwise the hypothesis is invalid; a^ = axis / |axis| and both thresholds are formed once, in f64.
 *    normal = n^ rounded to f32, anchor = p0.
 * 4. Inlier test, in f32, unfused: q = p - anchor per coordinate, s = (nx qx + ny qy) + nz qz; inlier iff fabsf(s) <= distance.
 * 5. Winner: the valid hypothesis with the most inliers among the candidates (its `support`), ties to the smaller h.  No valid
 *    hypothesis, or support < min_inliers: stop, this round reports no plane.
 * 6. Refit (refine != 0), over the winner's inliers: g = (int32) rintf((p - anchor) * 256) per coordinate (the f32
 *    subtraction, the exact scaling, round half to even); a point with any |g| > 2^22 stays an inlier but is left out of the
 *    sums.  Exact integer sums n_fit, S1[3], S2[6] (xx, xy, xz, yy, yz, zz); M = n_fit S2 - S1 S1^T exactly (128-bit), each entry
 *    converted to f64 once; the eigenvector of M's smallest eigenvalue l0 (the solver of lv_map_normals, f64) with the sign rule
 *    of step 3, rounded to f32, is the new normal; the new anchor is (float)((double)anchor + (double)S1 / (256.0 * n_fit)) per
 *    coordinate; rms = sqrt(max(l0, 0)) / (256 n_fit) metres.  n_fit < 3: the hypothesis' plane stands, bit 0 of flags clear.
 *    The constraint judges hypotheses only, not the refit.
 * 7. Labels: the members of plane r are the inliers of the FINAL plane among this round's candidates (step 4); they get label r.
 *
 * Read-only and ordered like lv_map_knn: it sees every earlier insert, eviction and rebuild, reads the active store while a
 * background rebuild runs and never waits for one. */
typedef struct lv_plane_params {
    float    distance;     /* > 0, finite: inlier iff |s| <= distance (step 4) */
    uint32_t iterations;   /* K, hypotheses per plane, 1..65536 */
    uint32_t max_planes;   /* 1..32 */
    uint32_t min_inliers;  /* >= 3: extraction stops when the best hypothesis has fewer */
    uint64_t seed;
    int      constraint;   /* 0 none; 1 normal within max_angle of axis (floors, ceilings);
                              2 normal within max_angle of the plane perpendicular to axis (walls) */
    float    axis[3];      /* constraint != 0: finite, non-zero; normalised in f64 */
    float    max_angle;    /* constraint != 0: radians, in (0, pi/2) */
    int      refine;       /* != 0: least-squares refit over the inliers, then reclassify once */
} lv_plane_params;
typedef struct lv_plane {
    float    normal[3], anchor[3];   /* the plane: (p - anchor) . normal = 0 */
    double   d;                      /* -(normal . anchor) in f64, (x + y) + z: normal . p + d = 0 */
    double   rms;                    /* refit only: sqrt(max(l0, 0)) / (256 n_fit), metres; else NaN */
    uint32_t inliers;                /* final label count */
    uint32_t support;                /* count of the winning hypothesis */
    uint32_t hypothesis;             /* index of the winning hypothesis */
    uint32_t candidates;             /* candidates of this round */
    uint32_t n_fit;                  /* points in the refit sums */
    uint32_t flags;                  /* bit 0: refit done */
} lv_plane;
/* Defaults: distance 0.1, iterations 512, max_planes 1, min_inliers 100, seed 0, constraint 0, axis (0, 0, 1),
 * max_angle 10 degrees, refine 1. */
void lv_default_plane_params(lv_plane_params* p);
/* mask: NULL, or lv_map_size() bytes in map order, 0 = excluded.  labels: NULL, or `capacity` entries of room, lv_map_size()
 * written in map order (capacity < lv_map_size(): LV_EINVAL): the plane's index in extraction order, -1 for a point on no plane.
 * planes: NULL, or the first min(P, planes_capacity) records in extraction order.  *n_planes (may be NULL) = P.  Parameters
 * outside the limits or a NULL params give LV_EINVAL with the reason in lv_last_error() and write nothing; an empty or unbuilt
 * map gives LV_OK, P = 0, nothing else written. */
int  lv_map_planes(lv_ctx* ctx, const lv_plane_params* p, const uint8_t* mask, int32_t* labels, size_t capacity,
                   lv_plane* planes, size_t planes_capacity, size_t* n_planes);

/* ---- Place recognition ---------------------------------------------------------------------------
 * Where in a saved map am I, with no pose prior (the front half of the reference's "Prelocalization with a previously saved HD
 * map")?  A place is a Scan Context descriptor (Kim & Kim, IROS 2018) with its centre, a LiDAR origin in the world.  The context
 * holds a database of places on the device, independent of the map (map build / insert / evict / rebuild never touch it).
 *   frame    world axes, origin at the place's centre.  A scan at state x: q = M p for every point p of the current scan (LiDAR
 *            frame), M = R_x R_off (rotations of x.rot and x.offset_R_L_I, quaternions taken as given, composed in f64 and
 *            rounded to f32 once; each coordinate M0*px + M1*py + M2*pz in f32, left to right, unfused); its centre is
 *            R_x t_off + x.pos (f64).  A map place of centre c: q = p - (float)c in f32 for every living map point p.
 *   binning  rho = sqrtf(qx*qx + qy*qy); a point counts iff rmin <= rho < rmax and v = qz + z_offset > 0.
 *            ring = floor((rho - rmin) / ((rmax - rmin) / n_rings)), sector = floor((atan2f(qy, qx) + pi) / (2 pi / n_sectors)),
 *            both in f32, clamped to the last ring / sector.  A bin holds the largest v of its points, 0 when empty.
 *            Layout ring-major: desc[ring * n_sectors + sector] (the layout of describe, fetch and load).
 *   distance for shift s: query column j against place column (j + s) mod n_sectors; a pair is valid when both columns have a
 *            non-zero norm; d(s) = 1 - mean over valid pairs of cos(query column, place column), 1 when no pair is valid
 *            (f32: each dot product and norm summed over the rings in order, the cosines over j in order; a result below 0
 *            from rounding is 0).  A place's distance is min_s d(s), its shift the smallest s reaching it.
 *   shift    the query's frame is rotated from the world by yaw = s * 2 pi / n_sectors (wrapped to (-pi, pi]): a candidate IMU
 *            pose for place i is rotation Rz(yaw) R_x, position centre_i - Rz(yaw) R_x t_off.  The query state only supplies
 *            roll, pitch and the extrinsics; its position is ignored and its yaw may be anything.
 *   retrieval  the k places of smallest distance, ordered by (distance, id); deterministic.
 * At most 2^20 places (LV_ERANGE beyond).  Outputs are synchronised on return. */
typedef struct lv_place_params {
    int   n_rings;      /* 1..32 */
    int   n_sectors;    /* 2..64 */
    float rmin, rmax;   /* 0 <= rmin < rmax <= 1000, metres */
    float z_offset;     /* finite: added to qz before the v > 0 test and the bin maximum */
} lv_place_params;
/* Defaults: 20 rings, 60 sectors, 0..80 m, z_offset 2.0. */
void lv_default_place_params(lv_place_params* p);
/* Sets the parameters and clears the database (LV_EINVAL outside the limits, nothing changed).  Until it is called the defaults
 * apply. */
int  lv_place_configure(lv_ctx* ctx, const lv_place_params* p);
/* desc: n_rings * n_sectors floats, the descriptor of the current scan (lv_scan_set) at state x; nothing is stored.
 * LV_ESTATE without a scan. */
int  lv_place_describe(lv_ctx* ctx, const lv_state* x, float* desc);
/* Appends the current scan at state x as a keyframe place; *id (may be NULL) receives its id.  LV_ESTATE without a scan. */
int  lv_place_add_scan(lv_ctx* ctx, const lv_state* x, uint32_t* id);
/* Appends n (1..65536) places built from the device map at centres[3i .. 3i+2]; *first_id (may be NULL) receives the first id,
 * the others follow.  An empty or unbuilt map gives all-zero descriptors.  Read-only on the map and ordered like lv_map_knn
 * (reads the active store during a background rebuild). */
int  lv_place_add_map(lv_ctx* ctx, const double* centres, size_t n, uint32_t* first_id);
/* The k (1..64, clamped to the count) places nearest to the current scan at state x: ids, shifts and distances in retrieval
 * order, *n_out = the clamped k.  LV_ESTATE on an empty database or without a scan. */
int  lv_place_query(lv_ctx* ctx, const lv_state* x, int k, uint32_t* ids, int32_t* shifts, float* dist, size_t* n_out);
size_t lv_place_count(lv_ctx* ctx);
int  lv_place_clear(lv_ctx* ctx);
/* All places in id order: desc (count * n_rings * n_sectors floats) and centres (3 * count doubles), each may be NULL;
 * LV_EINVAL when capacity < lv_place_count(). */
int  lv_place_fetch(lv_ctx* ctx, float* desc, double* centres, size_t capacity);
/* Appends n places (ids count .. count + n - 1) in the layout of lv_place_fetch.  Values must be finite and >= 0, centres finite
 * (LV_EINVAL otherwise, nothing stored). */
int  lv_place_load(lv_ctx* ctx, const float* desc, const double* centres, size_t n);

/* ---- Occupancy grid ------------------------------------------------------------------------------
 * Where space was observed empty, occupied, or never observed: what a planner needs next to the map (OctoMap's log-odds volume
 * and octomap_server's projected 2-D map; the reference has no counterpart).  The sweeps lv_map_remove_dynamic takes (lv_view:
 * pose sensor -> world, raw returns in the sensor frame) are ray-cast into a dense grid of f32 log-odds held by the context.  The
 * grid is independent of the map: it needs no built map and map build / insert / evict / rebuild never touch it.
 * The rule is integer arithmetic after one quantisation step, so it is exactly defined: a pure function of the inputs, bitwise
 * reproducible and independent of scheduling.
 *   grid     origin[3] is the world position of the low corner of voxel (0, 0, 0); resolution (finite, > 0) its edge; nx, ny, nz each
 *            1..1024 with nx * ny * nz <= 2^28.  Linear index (k * ny + j) * nx + i, x fastest.  One f32 log-odds value L per
 *            voxel; NaN = never observed.
 *   quantisation  Q = 256 sub-units per voxel.  Per axis q = (int32) floorf(((p - origin) / resolution) * 256.0f): f32 operations in
 *            exactly that order (unfused; IEEE division).  The voxel of q is q >> 8 (arithmetic shift).
 *            A view whose sensor origin t is non-finite or has any |(t - origin) / resolution| >= 8192 gives no evidence (nor does
 *            a view with n = 0): it adds nothing to the grid and nothing to the stats.  max_range / resolution <= 4096 (LV_EINVAL
 *            beyond): every walk then stays inside +-(8192 + 4096 + 1) voxels and every product below 2^41.
 *   returns  r2 = x*x + y*y + z*z, summed left to right.  A return is ignored if it is non-finite or r2 < min_range * min_range.  If
 *            r2 > max_range * max_range the return is CUT: c = max_range / sqrtf(r2), the point becomes (x*c, y*c, z*c) and it is
 *            not a hit.  World point per component ((R0*x + R1*y) + R2*z) + t, unfused, as in lv_map_remove_dynamic.  R must be
 *            finite (LV_EINVAL) and is meant to be a rotation; a return whose world point quantises to |q| >= 2^24 on any axis
 *            (65536 voxels from the origin: only an R that is no rotation does that) is ignored.
 *   walk     from qs (the quantised t) to qe (the quantised world point), in integers only.  Per axis a: d_a = qe_a - qs_a,
 *            ad_a = |d_a|, s_a = sign(d_a); cells vs = qs >> 8 and ve = qe >> 8; steps left r_a = |ve_a - vs_a|; the numerator to the
 *            first boundary n_a = ((vs_a + 1) << 8) - qs_a if s_a > 0, qs_a - (vs_a << 8) if s_a < 0.  While any r_a > 0: among the
 *            axes with r_a > 0 take the one with the smallest n_a / ad_a, compared by int64 cross-multiplication
 *            (n_a * ad_b <= n_b * ad_a), ties to x, then y, then z; step that axis by s_a, add 256 to n_a, decrement r_a.  The walk
 *            has exactly r_x + r_y + r_z steps and ends in ve.  Every cell it stands in before ve is CROSSED; ve is HIT if the
 *            return was not cut, otherwise crossed.  Cells outside the grid are skipped.
 *   update   OctoMap's insertPointCloud semantics, one update per voxel per view: Hit_v and Free_v are the in-grid sets over all
 *            rays of view v, Free_v -= Hit_v; views are applied in call order.  A voxel of Hit_v:
 *            L = fminf(fmaxf((isnan(L) ? 0 : L) + l_hit, l_min), l_max); a voxel of Free_v the same with l_miss.
 *   projection  octomap_server's rule: over the layers k_lo..k_hi (inclusive, clipped to the grid) a column (i, j) is 100 if any
 *            L >= l_occ, else 0 if any L <= l_free, else -1 (also when the clipped band is empty).  int8 at j * nx + i: the `data`
 *            layout of nav_msgs/OccupancyGrid.
 * Every call below except lv_default_occupancy_params and lv_occ_configure gives LV_ESTATE before lv_occ_configure.  Arguments
 * outside the limits give LV_EINVAL and change nothing.  The calls run on the context's stream and return when their host
 * outputs are written.  The grid and its buffers are owned by the context and freed by lv_destroy; nothing is allocated before
 * lv_occ_configure. */
typedef struct lv_occupancy_params {
    float origin[3]; float resolution; int nx, ny, nz;
    float min_range, max_range;              /* 0 < min_range < max_range */
    float l_hit, l_miss, l_min, l_max;       /* l_miss < 0 < l_hit, l_min < 0 < l_max, finite */
    float l_occ, l_free;                     /* l_free < l_occ */
} lv_occupancy_params;
/* Defaults: 0.2 m voxels, 512 x 512 x 64 centred on 0 in x, y with z from -3.2 (origin -51.2, -51.2, -3.2); ranges 1..80 m;
 * l_hit 0.85, l_miss -0.4, l_min -2.0, l_max 3.5 (OctoMap's probabilities 0.7 / 0.4 / 0.12 / 0.97); l_occ 0.4, l_free -0.4. */
void lv_default_occupancy_params(lv_occupancy_params* p);
/* Allocates the grid, every voxel unknown; reconfiguring discards the grid. */
int  lv_occ_configure(lv_ctx* ctx, const lv_occupancy_params* p);
/* n_views 1..32.  stats (may be NULL): rays used (returns not ignored, the cut ones included), rays cut, voxel updates free
 * (the sizes of Free_v), voxel updates hit (of Hit_v), each summed over the views. */
int  lv_occ_integrate(lv_ctx* ctx, const lv_view* views, size_t n_views, uint64_t stats[4]);
/* L of the voxel each world point falls in (quantised as above); NaN outside the grid and for non-finite points. */
int  lv_occ_query(lv_ctx* ctx, const void* pts, size_t stride, size_t n, float* logodds);
/* grid2d: nx * ny values; capacity < nx * ny or k_lo > k_hi: LV_EINVAL. */
int  lv_occ_project(lv_ctx* ctx, int k_lo, int k_hi, int8_t* grid2d, size_t capacity);
/* logodds: nx * ny * nz values (capacity below that: LV_EINVAL). */
int  lv_occ_fetch(lv_ctx* ctx, float* logodds, size_t capacity);
/* Replaces the grid.  n must equal nx * ny * nz; every value NaN or inside [l_min, l_max] (LV_EINVAL otherwise, grid unchanged). */
int  lv_occ_load(lv_ctx* ctx, const float* logodds, size_t n);
/* Every voxel back to unknown. */
int  lv_occ_clear(lv_ctx* ctx);
int  lv_occ_get_params(lv_ctx* ctx, lv_occupancy_params* out);

/* ---- Distance field ----------------------------------------------------------------------------------
 * How far every voxel of the occupancy grid is from the nearest obstacle, and through lv_occ_distance_query in which direction:
 * costmap_2d's inflation layer, the ESDF of Voxblox and FIESTA, the clearance term of CHOMP and TEB (the reference has no
 * counterpart).  An exact Euclidean distance transform of the grid, three separable passes on the device.  All distances are
 * squared integers in voxel units, so the field is exactly defined: a pure function of the grid and the parameters.
 *   obstacles, 3-D field (planar = 0)  voxel v is an obstacle iff L(v) >= l_occ (NaN compares false); with unknown_is_obstacle != 0
 *            a voxel whose L is NaN is an obstacle too.  A voxel with l_free < L < l_occ is not an obstacle.
 *   obstacles, 2-D field (planar != 0)  the cells are those of lv_occ_project(k_lo, k_hi), with the same clipping (k_lo > k_hi:
 *            LV_EINVAL).  A cell is an obstacle iff its projected value is 100; with unknown_is_obstacle a cell whose value is -1
 *            is one too.  The field has nx * ny cells, index j * nx + i, and behaves as a grid with nz = 1.
 *   outside distance  d2_out(v) = min over the obstacles o of dx^2 + dy^2 + dz^2 on integer voxel offsets; 0 on obstacles.  Only
 *            voxels inside the grid count as obstacles: the grid's border is not one.
 *   inside distance (signed_field != 0)  d2_in(v): the same minimum over the voxels that are not obstacles.
 *   stored value  one int32 s2 per voxel: s2 = d2_out(v) where v is not an obstacle; on obstacles s2 = 0 when unsigned and
 *            s2 = -d2_in(v) when signed.  LV_OCC_FAR where no obstacle exists, -LV_OCC_FAR where no voxel that is not an obstacle
 *            exists.  Every finite |s2| <= 3 * 1023^2 < 2^24.
 *   truncation  max_cells = 0: none, otherwise 1..1024.  A value with |s2| > max_cells * max_cells is stored as +-LV_OCC_FAR;
 *            nothing else changes.
 *   metres   m = resolution * sqrtf((float)|s2|) with the sign of s2: f32, unfused, sqrtf correctly rounded.  s2 = 0 gives
 *            +0.0f, +-LV_OCC_FAR gives +-inf.
 *   query    a point is quantised per axis as lv_occ_query does it (q, then q >> 8); in a planar field z is not used and may
 *            be anything, non-finite included.  dist is m of the voxel; NaN for a non-finite point and for one outside the grid.
 *            grad (may be NULL) holds 3 floats per point.  Per axis a let m-, m0, m+ be the metre values at v - e_a, v, v + e_a; a
 *            neighbour is usable iff it is in the grid and its value finite.  grad[a] = 0 if m0 is not finite (or NaN);
 *            (m+ - m-) / (resolution + resolution) with both neighbours usable; (m+ - m0) / resolution with only +;
 *            (m0 - m-) / resolution with only -; 0 with none.  In a planar field grad[2] = 0.
 * The field is a SNAPSHOT of the grid at build time: lv_occ_integrate, lv_occ_load and lv_occ_clear leave it in place and set
 * stale = 1 (a planner keeps reading the last field while sweeps arrive); lv_occ_configure frees it; a new build replaces it.
 * Building never changes a bit of the log-odds grid.  Every call gives LV_ESTATE before lv_occ_configure, fetch and query also
 * before a build (lv_occ_distance_info reports built = 0 instead).  Parameters outside the limits, a capacity below the field's
 * size or both outputs NULL give LV_EINVAL and change nothing; like lv_occ_configure's, the parameters are judged before the
 * context.  Nothing is allocated before the first build; lv_destroy frees everything.  The calls run on the context's stream and
 * return when their host outputs are written. */
#define LV_OCC_FAR 2147483647
typedef struct lv_distance_params { int planar, k_lo, k_hi, unknown_is_obstacle, signed_field, max_cells; } lv_distance_params;
typedef struct lv_distance_info   { int built, planar, nx, ny, nz, stale; lv_distance_params params; } lv_distance_info;
/* All zero: a 3-D field, unknown = free, unsigned, untruncated. */
void lv_default_distance_params(lv_distance_params* p);
/* stats (may be NULL): obstacles, voxels with a finite value, the largest finite d2_out, the largest finite d2_in (0 when the
 * field is unsigned). */
int  lv_occ_distance_build(lv_ctx* ctx, const lv_distance_params* p, uint64_t stats[4]);
/* s2 and / or metres: nx * ny * nz values (nx * ny of a planar field); either may be NULL, not both. */
int  lv_occ_distance_fetch(lv_ctx* ctx, int32_t* s2, float* metres, size_t capacity);
int  lv_occ_distance_query(lv_ctx* ctx, const void* pts, size_t stride, size_t n, float* dist, float* grad);
/* nx, ny, nz: the field's (nz = 1 when planar); all zero with built = 0. */
int  lv_occ_distance_info(lv_ctx* ctx, lv_distance_info* out);
/* Frees the field. */
int  lv_occ_distance_clear(lv_ctx* ctx);

/* ---- Planner -----------------------------------------------------------------------------------------
 * The cost-to-go from every traversable cell of the distance field to a set of goals, and routes from any number of starts by
 * descent: navfn's potential array, global_planner, the global plan of move_base (the reference has no counterpart).  Edge costs
 * are integers, so the potential is the unique fixpoint of relaxation: a pure function of the field, the table and the goals,
 * the same bits whatever order the device relaxes in.
 * The planner works on the cells of the distance field last built: nx * ny * nz of them, nz = 1 for a planar field, with the
 * field's linear index (k * ny + j) * nx + i.  No float enters the rule after the goal and start points are quantised.
 *   cell cost  let s = s2(v).  The cell is BLOCKED, c(v) = 0, iff s < min_clear_s2 (1..3 * 1023^2): obstacles, negative values and
 *            -LV_OCC_FAR are.  Otherwise t = n_cost - 1 if s == LV_OCC_FAR, else min(isqrt(s), n_cost - 1), and c(v) = cost[t];
 *            isqrt is the exact integer floor square root.  cost is the caller's table of n_cost (1..1025) bytes, every entry
 *            1..255: the cost of standing isqrt(s) whole cells from the nearest obstacle.
 *   moves    an offset (dx, dy, dz), components in {-1, 0, 1}, not all zero, m of them non-zero.  connectivity 4 or 6 allows
 *            m = 1, 8 or 18 m <= 2, 26 m <= 3; a planar field takes 4 or 8, a 3-D field 6, 18 or 26 (LV_EINVAL otherwise).  The
 *            move u -> v is allowed iff u and v are in the field and traversable and so is every cell u + (a proper non-empty
 *            subset of the move's non-zero components): 2 cells for a face diagonal, 6 for a space diagonal.  No corner is cut.
 *   edge     edge(u, v) = w(m) * (c(u) + c(v)), w = 10, 14, 17 for m = 1, 2, 3: symmetric, at most 8670.
 *   goals    1..65536 world points, quantised per axis as lv_occ_query does it (q, then q >> 8); in a planar field z is not
 *            used.  A goal that is non-finite, outside the field or in a blocked cell is ignored; `goals used` counts the points
 *            that are not (two in one cell count twice).  With no usable goal the build succeeds and every cell is unreached.
 *   potential  one uint32 P per cell.  D(v) = the least total edge cost over paths of allowed moves from any goal cell to v, 0
 *            on goal cells.  P(v) = D(v) if D(v) < 0xFFFFFFFF, else LV_PLAN_UNREACHED; blocked and disconnected cells are
 *            LV_PLAN_UNREACHED.  A relaxation whose 64-bit sum P(u) + edge(u, v) reaches 0xFFFFFFFF is dropped (prefixes of a
 *            shortest path are cheaper than the path, so P stays well defined).
 *   path     per start point.  status 2: the point is non-finite, outside the field or in a blocked cell; 1: P there is
 *            LV_PLAN_UNREACHED; 0 otherwise.  cost[i] = P of the start cell, LV_PLAN_UNREACHED for status 1 and 2.  With status 0
 *            the path is the sequence of cells (linear indices) from the start cell to a cell with P = 0, both included: from u
 *            the next cell is the first v with u -> v allowed and P(v) + edge(u, v) == P(u), "first" in lexicographic order of
 *            (dz, dy, dx), each running -1, 0, 1.  Such a v exists (the fixpoint), P strictly decreases, so the walk ends; a
 *            start on a goal gives a path of one cell.  The row is empty for status 1 and 2.
 * The plan is a SNAPSHOT: it keeps its own copy of the cell costs, origin and resolution, so lv_occ_plan_paths keeps answering
 * after the distance field is rebuilt.  lv_occ_distance_build and lv_occ_distance_clear leave it in place and set stale = 1;
 * lv_occ_configure frees it; a new build replaces it (a build that fails in the runtime, LV_EHIP, leaves no plan: built = 0;
 * a refused one leaves the old plan).  Building never changes a bit of the log-odds grid or of the distance field
 * (a stale field is planned on as it is).  lv_occ_plan_build judges parameters, table and counts before the context (LV_EINVAL;
 * "null context" comes last); every call gives LV_ESTATE before lv_occ_configure, lv_occ_plan_build also before a distance build,
 * fetch and paths also before a plan build (lv_occ_plan_info reports built = 0 instead).  A refused call writes nothing, except as
 * stated for lv_occ_plan_paths.  Nothing is allocated before the first build; lv_destroy frees everything.  The calls run on the
 * context's stream and return when their host outputs are written. */
#define LV_PLAN_UNREACHED 0xFFFFFFFFu
typedef struct lv_plan_params { int connectivity; int min_clear_s2; } lv_plan_params;
/* rounds: the relaxation rounds the build took (how the device got there, not part of the rule). */
typedef struct lv_plan_info   { int built, planar, nx, ny, nz, stale, rounds; lv_plan_params params; } lv_plan_info;
/* connectivity 8 (a planar field's; a 3-D field needs 6, 18 or 26), min_clear_s2 1. */
void lv_default_plan_params(lv_plan_params* p);
/* goals: n_goals points of 3 floats, `stride` bytes (>= 12) apart.  stats (may be NULL): goals used, traversable cells, reached
 * cells, the largest finite P. */
int  lv_occ_plan_build(lv_ctx* ctx, const lv_plan_params* p, const uint8_t* cost, size_t n_cost, const void* goals, size_t stride,
                       size_t n_goals, uint64_t stats[4]);
/* potential and / or cell_cost: one value per cell of the plan; either may be NULL, not both.  capacity below the number of
 * cells: LV_EINVAL. */
int  lv_occ_plan_fetch(lv_ctx* ctx, uint32_t* potential, uint8_t* cell_cost, size_t capacity);
/* CSR output as in lv_map_radius_search: start i's path is cells[offsets[i] .. offsets[i + 1]), offsets holds n + 1 entries,
 * *total = offsets[n].  cells == NULL: count only (status, cost, offsets and *total are written).  capacity < *total: LV_EINVAL,
 * with status, cost, offsets and *total still written, as lv_map_radius_search does it.  Offsets are 64-bit: the count-only call
 * reports any total; one fill returns at most 2^31 - 1 cells (a larger total is LV_EINVAL in the same way: split the starts).
 * n < 2^31 - 1. */
int  lv_occ_plan_paths(lv_ctx* ctx, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets,
                       int32_t* cells, size_t capacity, size_t* total);
/* nx, ny, nz: the plan's (nz = 1 when planar); all zero with built = 0. */
int  lv_occ_plan_info(lv_ctx* ctx, lv_plan_info* out);
/* Frees the plan. */
int  lv_occ_plan_clear(lv_ctx* ctx);

/* ---- Lattice planner ---------------------------------------------------------------------------------
 * The cost-to-go of a car-like robot: over states (cell, heading) of the planar plan last built, with the caller's table of motion
 * primitives as directed edges (SBPL's (x, y, theta) lattice, the State Lattice planner of nav2; the reference has no
 * counterpart).  Edge costs are integers, so V is again the unique fixpoint of relaxation: a pure function of the plan's cost
 * bytes, the table and the goals, the same bits whatever order the device relaxes in.  No float enters the rule after the cells
 * of goal and start points are quantised; headings are integers.
 *   source   the PLANAR plan last built: its cost bytes c(cell) (0 = blocked), nx, ny, origin and resolution.  The lattice keeps
 *            its own copy (a snapshot).  A 3-D plan is refused with LV_ESTATE.
 *   states   (i, j, h), h in 0..H-1, H in 1..16, linear index (h * ny + j) * nx + i.  nx * ny * H <= 2^28 (LV_EINVAL beyond).
 *   table    H * P records, P in 1..16; record h * P + p is primitive p of heading h.  length = 0: the slot is empty.  LV_EINVAL,
 *            with a message that names the record, for a field out of range, reserved != 0, unused sweep entries that are not 0,
 *            a non-empty record with di == dj == 0 and h_to == h (a self loop), and for a table with no non-empty record.  A turn
 *            on the spot (di == dj == 0, h_to != h) is allowed.
 *   move     primitive p from u = (i, j, h) leads to v = (i + di, j + dj, h_to).  It is allowed iff the start cell, the end
 *            cell and every sweep cell (offsets from the START cell) are inside the grid and have c != 0.
 *            edge = length * (c(u) + c(v)) + penalty: directed, at least 2.  Sweep cells add no cost.
 *   goals    1..65536 records of 3 floats and an int32 h, `stride` bytes (>= 16) apart.  The cell is quantised as
 *            lv_occ_plan_build quantises a goal (z is not used); h = -1: all H states of the cell.  A goal that is non-finite,
 *            outside the grid, in a blocked cell or has h outside -1..H-1 is ignored; `goals used` counts the records that are
 *            not.  With no usable goal the build succeeds and every state is unreached.
 *   V        one uint32 per state: the least total edge cost over sequences of allowed primitives from the state to any goal
 *            state, 0 on goal states; LV_LATTICE_UNREACHED if that cost is >= 0xFFFFFFFF, if the cell is blocked, or if no
 *            sequence exists.  A relaxation whose 64-bit sum reaches 0xFFFFFFFF is dropped, as the planner's is.
 *   path     per start record (3 floats, int32 h; h = -1: the heading with the least V at that cell, ties to the smaller h).
 *            status 2: non-finite, outside the grid, in a blocked cell, or h outside -1..H-1; 1: V there is unreached; 0
 *            otherwise.  cost[i] = V of the start state (LV_LATTICE_UNREACHED for status 1 and 2).  With status 0 the path is the
 *            sequence of state indices from the start state to a state with V = 0, both included: from s the next state is the
 *            successor of the FIRST p in 0..P-1 that is non-empty, allowed and has edge + V(succ) == V(s).
 * The lattice is a SNAPSHOT of the plan: lv_occ_plan_build (once its own checks have passed, whatever it then returns) and
 * lv_occ_plan_clear leave it in place and set stale = 1; a distance build or a grid edit does not touch it (the plan says of
 * itself that it is stale); after lv_volume_recentre it keeps answering for the same world points through its own origin;
 * lv_occ_configure frees it; a new build replaces it (one that fails in the runtime, LV_EHIP, leaves built = 0; a refused one
 * leaves the old lattice bit for bit).  lv_occ_lattice_build judges parameters, table and counts before the context (LV_EINVAL;
 * "null context" comes last), then asks for the grid, a plan and a planar plan (LV_ESTATE), then for the state count (LV_EINVAL).
 * fetch and paths give LV_ESTATE before lv_occ_configure and before a lattice build (lv_occ_lattice_info reports built = 0
 * instead).  A refused call writes nothing, except as stated for lv_occ_lattice_paths.  Nothing is allocated before the first
 * build; lv_destroy frees everything. */
#define LV_LATTICE_REACH 8
#define LV_LATTICE_MAX_SWEEP 10
#define LV_LATTICE_UNREACHED 0xFFFFFFFFu
typedef struct lv_lattice_prim {   /* 32 bytes */
    int8_t   di, dj;        /* end cell minus start cell, each |.| <= LV_LATTICE_REACH */
    uint8_t  h_to;          /* heading at the end, 0..H-1 */
    uint8_t  n_sweep;       /* 0..LV_LATTICE_MAX_SWEEP cells passed between the two ends */
    uint16_t length;        /* 0: the slot is empty.  Otherwise it multiplies c(u) + c(v); 10 = one cell, the planner's scale */
    uint16_t reserved;      /* 0 */
    uint32_t penalty;       /* added once per use (reversing, turning), <= 2^24 */
    int8_t   sweep[LV_LATTICE_MAX_SWEEP][2];   /* offsets from the START cell, each |.| <= LV_LATTICE_REACH; unused entries 0 */
} lv_lattice_prim;
typedef struct lv_lattice_params { int H, P; } lv_lattice_params;
/* rounds, tile (the edge of a workgroup's tile of cells, 16 or 8) and reach (the largest |offset| of the table) tell how the
 * device got there; they are not part of the rule. */
typedef struct lv_lattice_info { int built, nx, ny, H, P, stale, rounds, tile, reach; lv_lattice_params params; } lv_lattice_info;
/* H 16, P 3. */
void lv_default_lattice_params(lv_lattice_params* p);
/* prims: n_prims = H * P records.  stats (may be NULL): goals used, traversable states, reached states, the largest finite V. */
int  lv_occ_lattice_build(lv_ctx* ctx, const lv_lattice_params* p, const lv_lattice_prim* prims, size_t n_prims, const void* goals,
                          size_t stride, size_t n_goals, uint64_t stats[4]);
/* V: one value per state.  capacity below nx * ny * H: LV_EINVAL. */
int  lv_occ_lattice_fetch(lv_ctx* ctx, uint32_t* V, size_t capacity);
/* CSR output exactly as lv_occ_plan_paths does it, over states: start i's path is states[offsets[i] .. offsets[i + 1]).
 * states == NULL: count only.  prims (may be NULL; ignored in a count-only call) runs parallel to states: the primitive taken
 * out of each state, 255 at a path's last state.  capacity < *total, or a total above 2^31 - 1: LV_EINVAL with status, cost,
 * offsets and *total still written.  n < 2^31 - 1. */
int  lv_occ_lattice_paths(lv_ctx* ctx, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets,
                          int32_t* states, uint8_t* prims, size_t capacity, size_t* total);
/* All zero with built = 0. */
int  lv_occ_lattice_info(lv_ctx* ctx, lv_lattice_info* out);
/* Frees the lattice. */
int  lv_occ_lattice_clear(lv_ctx* ctx);

/* ---- Frontiers ---------------------------------------------------------------------------------------
 * Where to go next when the site is not mapped yet: the boundary between space observed free and space never observed, grouped
 * into clusters and ranked by what the planner says it costs to get there (Yamauchi's frontiers, explore_lite,
 * frontier_exploration, the frontier clusters of FUEL in 3-D; the reference has no counterpart).  Connected-component labelling
 * of the grid on the device.  The rule is integer arithmetic once the cell states are decided, so it is exactly defined: a pure
 * function of the grid and the parameters, the same bits whatever the schedule.
 *   cells, 3-D (planar = 0)  the voxels of the grid, linear index (k * ny + j) * nx + i.  A voxel is FREE iff L <= l_free,
 *            OCCUPIED iff L >= l_occ, UNKNOWN iff L is NaN; one with l_free < L < l_occ is none of the three.
 *   cells, planar (planar != 0)  those of lv_occ_project(k_lo, k_hi), with the same clipping (k_lo > k_hi: LV_EINVAL).  A cell is
 *            FREE iff its projected value is 0, OCCUPIED iff it is 100, UNKNOWN iff it is -1.  The result has nx * ny cells, index
 *            j * nx + i, and behaves as a grid with nz = 1.
 *   frontier cell  a FREE cell with at least one UNKNOWN face neighbour (4 of them when planar, 6 in 3-D) that lies inside the
 *            field.  The field's border is not unknown, as it is no obstacle to the distance field.
 *   clusters  the connected components of the frontier cells under `connectivity`: 4 or 8 for a planar result, 6, 18 or 26 for a
 *            3-D one (LV_EINVAL otherwise), plain adjacency by the moves of the planner's "moves" paragraph; there is no corner rule
 *            here.  A component with fewer than min_size (1..2^28) cells is dropped: its cells get no label.
 *   numbering  labels 0..C-1 by size descending, ties to the smaller `first`: the order of lv_map_cluster.
 *   labels   one int32 per cell: the cluster's number on its members, LV_FRONTIER_NONE everywhere else.
 *   per cluster  size; first, the smallest member index; sum[a], the sums of the members' i, j, k; lo and hi, the bounding box
 *            (inclusive); centre[a] = (2 * sum[a] + size) / (2 * size) in integer division, the centroid rounded half up; rep, the
 *            member that minimises dx^2 + dy^2 + dz^2 to centre, ties to the smaller index.  rep is always a frontier cell, centre
 *            need not be.  sum[a] < 2^38.
 *   stats    FREE cells, UNKNOWN cells, frontier cells (before min_size is applied), clusters reported (C).
 *   rank     needs a plan (lv_occ_plan_info.built) whose planar, nx, ny, nz equal the frontier's (LV_ESTATE otherwise); reach 0..8
 *            (LV_EINVAL otherwise).  For cluster c, best_p[c] is the least potential P over all plan cells v within Chebyshev
 *            distance `reach` of any member of c (in a planar result in (i, j) only), clipped to the field, and best_cell[c] the v
 *            that attains it, ties to the smaller index.  If every such P is LV_PLAN_UNREACHED: best_p[c] = LV_PLAN_UNREACHED and
 *            best_cell[c] = -1.  (When the distance field counts unknown as an obstacle every frontier cell has s2 = 1 and is
 *            blocked for a robot wider than a cell: the cell to drive to is a reachable one nearby.  The planner's edges are
 *            symmetric, so a plan whose only goal is the robot's position holds the cost from the robot to every cell.)  A stale
 *            plan, or a stale frontier, is ranked as it is.
 * The result is a SNAPSHOT of the grid at build time, as the distance field is: lv_occ_integrate, lv_occ_load and lv_occ_clear
 * leave it in place and set stale = 1; lv_occ_configure frees it; a new build replaces it (a build that fails in the runtime,
 * LV_EHIP, leaves none; a refused one leaves the old result).  Building never changes a bit of the grid, the distance field or
 * the plan.  Parameters are judged before the context (LV_EINVAL; "null context" comes last); every call gives LV_ESTATE before
 * lv_occ_configure, fetch, clusters and rank also before a build (lv_occ_frontier_info reports built = 0 instead).  A refused call
 * writes nothing, except as stated for lv_occ_frontier_clusters.  Nothing is allocated before the first build; lv_destroy frees
 * everything.  The calls run on the context's stream and return when their host outputs are written. */
#define LV_FRONTIER_NONE (-1)
typedef struct lv_frontier_params { int planar, k_lo, k_hi, connectivity, min_size; } lv_frontier_params;
typedef struct lv_frontier_info   { int built, planar, nx, ny, nz, stale, n_clusters; lv_frontier_params params; } lv_frontier_info;
typedef struct lv_frontier_cluster {          /* 72 bytes */
    int32_t size, first, rep;                 /* cells; smallest member index; representative member index */
    int32_t centre[3], lo[3], hi[3];          /* rounded centroid; bounding box, inclusive (i, j, k) */
    uint64_t sum[3];                          /* sums of the members' i, j, k */
} lv_frontier_cluster;
/* planar 0, k_lo 0, k_hi 0, connectivity 26, min_size 1. */
void lv_default_frontier_params(lv_frontier_params* p);
/* stats (may be NULL): as above. */
int  lv_occ_frontier_build(lv_ctx* ctx, const lv_frontier_params* p, uint64_t stats[4]);
/* labels: one value per cell of the result; capacity below the number of cells (or labels NULL): LV_EINVAL. */
int  lv_occ_frontier_fetch(lv_ctx* ctx, int32_t* labels, size_t capacity);
/* Count, then fill, as lv_map_radius_search: *n = C always; out == NULL writes only *n; capacity < C: LV_EINVAL with *n still
 * written. */
int  lv_occ_frontier_clusters(lv_ctx* ctx, lv_frontier_cluster* out, size_t capacity, size_t* n);
/* best_p and / or best_cell: C values each; either may be NULL, not both (LV_EINVAL, as is capacity < C). */
int  lv_occ_frontier_rank(lv_ctx* ctx, int reach, uint32_t* best_p, int32_t* best_cell, size_t capacity);
/* nx, ny, nz: the result's (nz = 1 when planar); all zero with built = 0. */
int  lv_occ_frontier_info(lv_ctx* ctx, lv_frontier_info* out);
/* Frees the result. */
int  lv_occ_frontier_clear(lv_ctx* ctx);

/* ---- Ray casting -------------------------------------------------------------------------------------
 * What a sensor would see from a given place, and how much unknown space a pose would uncover: line of sight, simulated range
 * scans, and the information gain of a candidate view that explore_lite, NBVP and FUEL weigh a frontier by (the reference has no
 * counterpart).  The walk of the "Occupancy grid" section, unchanged, but READING the log-odds instead of writing them.  The rule
 * is integer arithmetic once the ends are quantised and the cell states decided, so it is exactly defined: a pure function of
 * the grid and the arguments, the same bits whatever the schedule.  No float leaves the device.
 *   cell states  those of the 3-D cells of "Frontiers": FREE iff L <= l_free, OCCUPIED iff L >= l_occ, UNKNOWN iff L is NaN; a
 *            voxel with l_free < L < l_occ is OTHER.
 *   ends     lv_occ_raycast: `from` is quantised as a view's sensor origin is (per axis c = (p - origin) / resolution must have
 *            |c| < 8192, then qs = (int32) floorf(c * 256.0f)) and `to` as a return's world point is (qe = (int32)
 *            floorf(((p - origin) / resolution) * 256.0f), |qe| < 2^24), f32 operations in exactly that order.  A ray one of whose
 *            ends fails (non-finite included) is IGNORED.  lv_occ_view_gain: qs, qe and which returns are ignored or cut are
 *            exactly those of lv_occ_integrate for the same view ("quantisation", "returns"); R must be finite (LV_EINVAL).
 *            These are the bounds under which the walk's products fit in int64: for a view every product stays below 2^41, as
 *            argued there; for lv_occ_raycast |qs| < 2^21 and |qe| < 2^24 give ad_a < 2^25 and n_a < 2^26, every product below 2^51.
 *   cells of a ray  c_0 = vs, c_1, ..., c_S = ve: the cells the walk of "Occupancy grid" stands in, S = r_x + r_y + r_z.  Step
 *            s >= 1 enters c_s across axis a_s (0, 1, 2) at the fraction num_s / den_s of the segment qs -> qe, where num_s is n_a
 *            as it stood BEFORE the step added 256 to it and den_s = ad_a; 0 <= num_s <= den_s (0 only when qs lies on a cell
 *            face and the ray leaves through it at once).  Cells outside the grid belong to the sequence but have no state:
 *            they neither stop a ray nor count.
 *   stop     a cell inside the grid stops a ray iff it is OCCUPIED, or UNKNOWN while stop_unknown != 0.  c_0 is examined like
 *            every other cell.  s* is the least s whose c_s stops the ray.
 *   result, STOPPED  cell = the linear index of c_s*; steps = s*; axis = a_s*; num / den = num_s* / den_s* (s* = 0: axis -1, num 0,
 *            den 1); n_free and n_unknown count the in-grid FREE and UNKNOWN cells among c_0 .. c_(s* - 1).  The point where the
 *            ray enters the cell is qs + (qe - qs) * num / den sub-units: metres are the caller's business.
 *   result, CLEAR  (no cell stops the ray) cell = the linear index of ve, -1 if ve is outside the grid; steps = S; axis = -1;
 *            num = den = 1; the counts run over c_0 .. c_S.
 *   result, IGNORED  status 0, cell -1, every other field 0.
 *   view gain  per view v (an lv_view whose returns are the end points of a scan pattern in the sensor frame), with rays
 *            stopping at OCCUPIED cells only, cut and hit returns alike: gain[4v + 0] = rays used (returns not ignored),
 *            gain[4v + 1] = rays stopped, gain[4v + 2] = the DISTINCT in-grid UNKNOWN cells that lie before the stop on at least
 *            one used ray of v (c_0 .. c_(s* - 1); c_0 .. c_S, ve included, for a ray that does not stop), gain[4v + 3] the same for
 *            FREE cells.  Views are independent of each other and of their order.  A view that gives no evidence ("quantisation":
 *            its origin fails, or n = 0) yields four zeros.
 * Both calls read the LIVE grid, not a snapshot, and change no bit of the grid, the distance field, the plan or the frontier
 * result, nor any stale flag.  Parameters and NULL or short arguments are judged before the context (LV_EINVAL, nothing
 * written; "null context" comes last); both give LV_ESTATE before lv_occ_configure.  Nothing is allocated before the first call;
 * lv_occ_configure and lv_destroy free everything.  The calls run on the context's stream and return when their host outputs
 * are written. */
#define LV_RAY_IGNORED 0
#define LV_RAY_CLEAR   1
#define LV_RAY_STOPPED 2
typedef struct lv_ray_params { int stop_unknown; } lv_ray_params;
typedef struct lv_ray_result {                /* 32 bytes */
    int32_t status, cell, steps, axis, n_free, n_unknown, num, den;
} lv_ray_result;
/* stop_unknown 0. */
void lv_default_ray_params(lv_ray_params* p);
/* from, to: n world points each, the first three floats of every stride bytes (strides >= 12); out: n results.  n = 0 succeeds
 * and writes nothing; n < 2^31 - 1. */
int  lv_occ_raycast(lv_ctx* ctx, const lv_ray_params* p, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                    lv_ray_result* out);
/* n_views 1..32; gain: n_views x 4 counters as above. */
int  lv_occ_view_gain(lv_ctx* ctx, const lv_view* views, size_t n_views, uint64_t* gain);

/* ---- Elevation map -----------------------------------------------------------------------------------
 * A 2.5-D height map of the ground with a traversability class per cell, from the points of the device map or from the caller's:
 * ANYbotics' elevation_mapping and traversability_estimation, Autoware's points2costmap, the terrain layer of grid_map (the
 * reference has no counterpart).  Where the planar products of "Occupancy grid" call a cell an obstacle when any voxel of a fixed
 * band of layers is occupied, here every cell carries its own ground height, and what is lethal follows from the step to the
 * neighbouring cells, the slope and the height of what stands on the ground; what hangs above the robot is ignored.  Integer
 * arithmetic after one quantisation, integer min / max / add only: a pure function of the point SET and the parameters, the same
 * bits whatever the order of the points and the schedule.
 *   grid     origin[3], resolution (finite, > 0), nx, ny each 1..4096, nx * ny <= 2^24; cell index j * nx + i (the layout of
 *            nav_msgs/OccupancyGrid).  origin[2] is the zero of the height scale.
 *   point    per axis q_a = (int32) floorf(((p_a - origin_a) / resolution) * 256.0f), f32 operations in exactly that order (the
 *            quantisation of lv_occ_query: 256 sub-units per cell).  A point is IGNORED if an axis fails (non-finite, or
 *            |q_a| >= 2^24) or if its cell (q_x >> 8, q_y >> 8) lies outside the grid; otherwise it is USED in that cell c with
 *            the integer height z = q_z.
 *   layers   n(c) = the used points of c; lo(c) = min z.  The BODY BAND of c is its points with z - lo(c) <= head: nb(c) their
 *            number, top(c) their max z.  Points above the band are OVERHANG: they count in n and in nothing else.  A cell with
 *            n = 0 has lo = LV_ELEV_NONE, top = -LV_ELEV_NONE, nb = 0.  c is KNOWN iff nb(c) >= min_points.
 *   terrain  per KNOWN cell, its neighbours being the KNOWN cells of its 8-neighbourhood inside the grid: span = top - lo;
 *            step = max |lo(c') - lo(c)| over the neighbours, 0 with none; g_x from the cells at i - 1 and i + 1: lo(i+1) - lo(i-1)
 *            with both known, 2 * (lo(i+1) - lo(i)) with only i + 1, 2 * (lo(i) - lo(i-1)) with only i - 1, 0 with neither; g_y
 *            likewise along j; slope2 = min(g_x^2 + g_y^2, 2^31 - 1) computed in int64: tan^2 of the slope is slope2 / 512^2.
 *            Cells that are not known store span = step = slope2 = 0.
 *   class    int8: -1 if the cell is not known; 100 if span > max_span or step > max_step or slope2 > max_slope2; 0 otherwise.
 *   height   metres: origin[2] + resolution * ((float)lo / 256.0f), f32, unfused, in that order; NaN where the cell is not known.
 *   limits   min_points 1..2^20; head, max_span, max_step 0..2^25 (sub-units); max_slope2 0..2^31 - 1.
 *   source   pts == NULL (n is ignored): the living points of the device map, after the insert in flight has settled, as
 *            lv_map_paint reads them; a map that is not built or empty gives a built elevation map with every cell unknown and
 *            all-zero stats.  Otherwise n (< 2^31) caller points, the first three floats of every stride bytes (stride >= 12);
 *            n = 0 is allowed.
 *   query    the cell of a point is that of lv_occ_distance_query in a planar field: x and y quantised, z not used (it may be
 *            anything).  height and cls of that cell; NaN and -1 for a non-finite x or y and for a point outside the grid.
 * The result is a SNAPSHOT of its source: later inserts into and removals from the map do not change it; a new build replaces it,
 * a build refused with LV_EINVAL leaves it in place; lv_elev_clear and lv_destroy free it.  A build changes no bit of the map,
 * the occupancy grid or anything built from it.
 *   distance from cells  lv_occ_distance_build_cells builds the planar field of "Distance field" exactly as lv_occ_distance_build
 *            does with planar != 0, but over the caller's cells instead of the projected ones: cells[j * nx + i], n == nx * ny of
 *            the configured occupancy grid (else LV_EINVAL).  A cell is an obstacle iff its value is 100; with
 *            unknown_is_obstacle any negative value is one too; every other value is not an obstacle.  p->planar must be non-zero;
 *            k_lo / k_hi are not used and are reported back as given.  Truncation, signed fields, stats, fetch, query, info, the
 *            stale rule and what the planner and the frontier ranking do with the field are those of lv_occ_distance_build, so a
 *            class grid of this section (merged with lv_occ_project or not) becomes the planner's obstacles.  LV_ESTATE before
 *            lv_occ_configure; a refused call leaves the old field in place.
 * Parameters and NULL or short arguments are judged before the context (LV_EINVAL, nothing written;
 * "null context" comes last); lv_elev_fetch and lv_elev_query give LV_ESTATE before a build (lv_elev_info reports built = 0
 * instead).  Nothing is allocated before the first build.  The calls run on the context's stream and return when their host
 * outputs are written. */
#define LV_ELEV_NONE 2147483647
#define LV_ELEV_LO         0   /* int32 */
#define LV_ELEV_TOP        1   /* int32 */
#define LV_ELEV_SPAN       2   /* int32 */
#define LV_ELEV_STEP       3   /* int32 */
#define LV_ELEV_SLOPE2     4   /* int32 */
#define LV_ELEV_COUNT      5   /* uint32: n */
#define LV_ELEV_BAND_COUNT 6   /* uint32: nb */
#define LV_ELEV_CLASS      7   /* int8 */
#define LV_ELEV_HEIGHT     8   /* float */
typedef struct lv_elevation_params {
    float origin[3];
    float resolution;
    int nx, ny;
    int min_points;
    int head, max_span, max_step;   /* sub-units: 256 per cell */
    int max_slope2;
} lv_elevation_params;
typedef struct lv_elevation_info {
    int built, nx, ny, from_map;
    uint64_t n_points;              /* source points swept: the caller's n, or the map's living points */
    lv_elevation_params params;
} lv_elevation_info;
/* The footprint of lv_default_occupancy_params: origin (-51.2, -51.2, -3.2), resolution 0.2, 512 x 512; min_points 3; head 1920
 * (1.5 m), max_span 153 (0.12 m), max_step 128 (0.10 m), each floor(metres / resolution * 256); max_slope2 34727 =
 * floor((512 tan 20 deg)^2). */
void lv_default_elevation_params(lv_elevation_params* p);
/* stats (may be NULL): points used, overhang points, known cells, lethal cells. */
int  lv_elev_build(lv_ctx* ctx, const lv_elevation_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]);
/* out: nx * ny elements of the layer's type; capacity in elements. */
int  lv_elev_fetch(lv_ctx* ctx, int layer, void* out, size_t capacity);
/* height, cls: n values each; either may be NULL, not both. */
int  lv_elev_query(lv_ctx* ctx, const void* pts, size_t stride, size_t n, float* height, int8_t* cls);
/* All zero with built = 0. */
int  lv_elev_info(lv_ctx* ctx, lv_elevation_info* out);
/* Frees the elevation map. */
int  lv_elev_clear(lv_ctx* ctx);
/* cells: n = nx * ny values of the occupancy grid's plane; stats as lv_occ_distance_build's. */
int  lv_occ_distance_build_cells(lv_ctx* ctx, const lv_distance_params* p, const int8_t* cells, size_t n, uint64_t stats[4]);

/* ---- Rollouts ----------------------------------------------------------------------------------------
 * The local planner of move_base / nav2 on the device: K candidate control sequences are rolled forward through a unicycle model
 * from one start pose, the ones that collide are cut short, and the rest are scored against the plan (base_local_planner's
 * trajectory rollout, dwa_local_planner, the MPPI controller of nav2; the reference has no counterpart).  Every f32 operation and
 * its order are stated below and the sine and cosine are one fixed polynomial, so a rollout is exactly defined: a pure function
 * of the plan, the field and the arguments, the same bits whatever the schedule.
 *   reads    the plan last built: its cost bytes c and its potential P, with the plan's own origin and resolution.  It must be
 *            planar (LV_ESTATE otherwise).  With n_fp > 0 the distance field last built is read too; its planar, nx, ny must
 *            equal the plan's (LV_ESTATE otherwise).  A stale plan or field is used as it is.  Nothing is snapshotted, and no bit
 *            of the grid, the field, the plan or the frontier result changes, nor any stale flag.
 *   inputs   start = (x0, y0, th0), world metres and radians; K sequences of Tc pairs (v, w), m/s and rad/s, laid out
 *            [K][Tc][2]; T steps of dt seconds, step s = 1..T using pair min(s - 1, Tc - 1) (Tc = 1: one constant command, as
 *            DWA samples them; Tc = T: a full sequence, as MPPI does); n_fp footprint points (fx, fy) in the body frame, laid out
 *            [n_fp][2].  Nothing here needs to be finite: what a non-finite value leads to is stated under "pose test".
 *   motion   all in f32, no operation fused, in exactly this order.  A heading th is USABLE iff fabsf(th) < 1048576.0f (NaN is
 *            not).  (sn, cs) = the sine and cosine of th_(s-1) by the library's fixed polynomial (f32 -> f64, k = rint(x * 2 / pi),
 *            a three-term Cody-Waite reduction, two six-term polynomials in r^2, the quadrant from (int) k & 3, rounded to f32:
 *            the bound above is the one under which (int) k is defined); d = v * dt; x_s = x_(s-1) + d * cs;
 *            y_s = y_(s-1) + d * sn; th_s = th_(s-1) + w * dt.  A step may jump over a cell: keep |v| * dt at or below the
 *            resolution; there is no sub-stepping.
 *   pose test  for s = 1..T pose s is BAD for the first of these reasons that applies, and good otherwise.  1: th_(s-1) is not
 *            usable (before the step; it counts against pose s).  2: th_s is not usable.  3: (x_s, y_s) has no cell in the plan
 *            (quantised as lv_occ_plan_paths quantises a start; non-finite coordinates end here).  4: the cell's cost byte is 0.
 *            5: a footprint point has no cell in the field.  6: a footprint point's s2 < fp_clear_s2.  Footprint point g of
 *            pose s is (x_s + (cs' * fx - sn' * fy), y_s + (sn' * fx + cs' * fy)) with (sn', cs') the sine and cosine of th_s, the
 *            very values step s + 1 uses; every point is judged for reason 5 before any for reason 6.  Pose 0 is not examined:
 *            a robot standing in an inflated cell can still leave it.  n_ok = the number of good poses before the first bad one.
 *   result   per sequence.  status LV_ROLLOUT_CLEAR iff n_ok = T, else LV_ROLLOUT_STOPPED; steps = n_ok; why = 0 when clear,
 *            else the reason that made pose n_ok + 1 bad; cell_end = the plan's linear index of pose n_ok's cell, -1 if it has
 *            none (possible only for n_ok = 0); p_end = P there, LV_PLAN_UNREACHED without a cell; p_min = the least P over
 *            the poses 0..n_ok that have a cell and s_min the first step that attains it (LV_PLAN_UNREACHED and -1 if none has
 *            one); cost_sum = the sum of the cost bytes of poses 1..n_ok.
 *   poses    K x (T + 1) x 3 floats (x, y, th): rows 0..n_ok of a sequence are its poses, every float of a later row is the bit
 *            pattern 0x7FC00000.
 *   score    p_sel = p_end with goal_mode 0, p_min with goal_mode 1.  A sequence is ELIGIBLE iff steps >= min_steps and
 *            p_sel != LV_PLAN_UNREACHED; its score is w_cost * cost_sum + w_goal * p_sel + w_stop * (T - steps) in uint64 (below
 *            2^50: the weights are at most 65535); the score of any other is UINT64_MAX.
 *   best     best[0] = the eligible index with the least (score, index), best[1] = its score; both -1 if none is eligible.
 *   limits   T 1..1024; Tc 1..T; dt finite and > 0; n_fp 0..64, footprint non-NULL when n_fp > 0; fp_clear_s2 1..3 * 1023^2;
 *            min_steps 0..T; goal_mode 0 or 1; weights 0..65535; K 0..2^20, controls non-NULL when K > 0; start non-NULL;
 *            results, poses, score and best may each be NULL, but not all four.  K * Tc <= 2^24 pairs (128 MiB of controls,
 *            pinned on the host and again on the device), and with poses K * (T + 1) <= 2^24 rows (192 MiB).  K = 0 succeeds
 *            and writes best only; like every other call it is answered after the states below (LV_ESTATE comes first).
 * Parameters and NULL arguments are judged before the context (LV_EINVAL, nothing written; "null context" comes last);
 * LV_ESTATE before lv_occ_configure, before a plan build, and as stated under "reads".  A refused call writes nothing.  Nothing
 * is allocated before the first call; lv_occ_configure and lv_destroy free everything.  The call runs on the context's stream
 * and returns when its host outputs are written. */
#define LV_ROLLOUT_CLEAR   1
#define LV_ROLLOUT_STOPPED 2
typedef struct lv_rollout_params {
    int T, Tc;
    float dt;
    int fp_clear_s2;
    uint32_t w_cost, w_goal, w_stop;
    int min_steps, goal_mode;
} lv_rollout_params;
typedef struct lv_rollout_result {            /* 32 bytes */
    int32_t status, steps, why, cell_end;
    uint32_t p_end, p_min;
    int32_t s_min;
    uint32_t cost_sum;
} lv_rollout_result;
/* T 32, Tc 1, dt 0.1, fp_clear_s2 1, w_cost 1, w_goal 1, w_stop 0, min_steps 1, goal_mode 0. */
void lv_default_rollout_params(lv_rollout_params* p);
/* start: 3 floats; controls: K x Tc x 2 floats; footprint: n_fp x 2 floats; results: K records; poses: K x (T + 1) x 3 floats;
 * score: K values; best: 2 values. */
int  lv_occ_rollout(lv_ctx* ctx, const lv_rollout_params* p, const float* start, const float* controls, size_t K, const float* footprint,
                    size_t n_fp, lv_rollout_result* results, float* poses, uint64_t* score, int64_t* best);

/* ---- Localisation ------------------------------------------------------------------------------------
 * The measurement update of AMCL on the device: K candidate poses are weighed against one scan by the likelihood field, which is
 * a lookup of every scan end point in the distance field (Probabilistic Robotics, table 6.3; amcl's likelihood_field model; the
 * reference has no counterpart).  A particle filter around it finds and tracks the robot in a saved grid from a scan alone, with
 * no point map and no pose prior.  Every f32 operation and its order are stated below and the sine and cosine are the fixed
 * polynomial of "Rollouts", so a weight is exactly defined: a pure function of the field and the arguments, the same bits
 * whatever the schedule.
 *   reads    the distance field last built, planar or 3-D, with the field's own origin and resolution (the ones it was built
 *            at: it answers after lv_volume_recentre as it did before).  A stale field is used as it is.  Nothing is
 *            snapshotted, and no bit of the grid, the field, the plan or the frontier result changes, nor any stale flag.
 *   inputs   poses [K][4] = (x, y, z, th), world metres and radians; beams [B][3] = the scan's end points (ex, ey, ez) in a
 *            gravity-aligned body frame (x forward, z up); table = n_table costs, the caller's negative log-likelihood of an end
 *            point by the SQUARED voxel distance to the nearest obstacle, entry t for s2 = t (the caller supplies it as the
 *            planner's caller supplies the clearance-to-cost table).  Nothing here needs to be finite.
 *   rule     per particle, all in f32, no operation fused, in exactly this order.  th is USABLE iff fabsf(th) < 1048576.0f (NaN
 *            is not).  An unusable th gives n_in = 0 and the score UINT64_MAX.  Otherwise (sn, cs) = the sine and cosine of th
 *            by the polynomial of "Rollouts", and for beam b: px = x + (cs * ex - sn * ey); py = y + (sn * ex + cs * ey);
 *            pz = z + ez.  The cell of (px, py, pz) is the one lv_occ_distance_query finds: quantised per axis (q, then q >> 8)
 *            and tested against the field; in a planar field z is not used and may be anything.  A point without a cell
 *            (non-finite, too far to quantise, outside the field) costs out_cost.  Otherwise s2 is the field's value there,
 *            idx = 0 if s2 <= 0, else min(s2, n_table - 1) (so LV_OCC_FAR takes the last entry and the inside of a signed
 *            field entry 0), and the cost is table[idx].
 *   result   n_in = the number of beams that have a cell; score = the sum of the B costs in uint64; if n_in < min_inside the
 *            score is UINT64_MAX instead (n_in stays).
 *   best     best[0] = the index with the least (score, index) among the scores that are not UINT64_MAX, best[1] = its score;
 *            both -1 when there is none.
 *   limits   K 0..2^20, poses non-NULL when K > 0; B 1..65536; K * B <= 2^30; n_table 1..4096; every table entry and out_cost
 *            <= 2^24, so a score stays below 2^40; min_inside 0..B; beams and table non-NULL; score, n_in and best may each be
 *            NULL, but not all three.  K = 0 succeeds and writes best only; like every other call it is answered after the
 *            states below (LV_ESTATE comes first).
 * Parameters and NULL arguments are judged before the context (LV_EINVAL, nothing written; "null context" comes last);
 * LV_ESTATE before lv_occ_configure and before a field build.  A refused call writes nothing.  Nothing is allocated before the
 * first call; lv_occ_configure and lv_destroy free everything.  The call runs on the context's stream and returns when its host
 * outputs are written. */
typedef struct lv_mcl_params { uint32_t out_cost; int min_inside; } lv_mcl_params;
/* out_cost 0 (the table's last entry is NOT implied), min_inside 1. */
void lv_default_mcl_params(lv_mcl_params* p);
/* poses: K x 4 floats; beams: B x 3 floats; table: n_table values; score: K values; n_in: K values; best: 2 values. */
int  lv_occ_mcl_weigh(lv_ctx* ctx, const lv_mcl_params* p, const float* poses, size_t K, const float* beams, size_t B,
                      const uint32_t* table, size_t n_table, uint64_t* score, uint32_t* n_in, int64_t* best);

/* ---- Resident localisation filter ------------------------------------------------------------------
 * The whole cycle of AMCL on the device: K particles that stay there from one cycle to the next, with the motion update
 * (sample_motion_model_odometry, Probabilistic Robotics, table 5.6, with the filter's own reproducible noise), the measurement
 * update of "Localisation", the weights, the effective sample size, the estimate's sums and the systematic resampling.  f32
 * operations in a stated order up to a cell or a quantised coordinate, integers after it, no float atomics: every output is a
 * pure function of the arguments and the calls before, bitwise reproducible.
 *   draws    mix(x) is splitmix64's finaliser with its additive constant; word(i, j) = mix(mix(mix(seed) ^ epoch) ^ ((i << 8) | j))
 *            for particle i and j = 0..8, all 64-bit.  Standard normal n (0..2) of particle i: the sum of the twelve 16-bit fields
 *            of the words 3n, 3n + 1, 3n + 2; G = 2 * sum - 12 * 65535; z = (float)G * 2^-17.  The resampling draw of an epoch is
 *            mix(mix(mix(seed) ^ epoch) ^ UINT64_MAX).  epoch is a uint32 the store keeps: 0 after _set, incremented at the end of
 *            every _move and every _resample; both are refused (LV_ESTATE) once it is 2^32 - 1.
 *   move     delta = (rot1, trans, rot2), sigma = their standard deviations (from the alphas, by the caller), all finite,
 *            sigma >= 0.  In f32, nothing fused, in this order: r1 = rot1 - z0 * s_rot1; tr = trans - z1 * s_trans;
 *            r2 = rot2 - z2 * s_rot2; a = th + r1; (sn, cs) = the fixed polynomial of a; x += tr * cs; y += tr * sn; th = a + r2;
 *            if th >= 3.14159274f then th -= 6.28318548f; then if th < -3.14159274f then th += 6.28318548f.  z stays.  A particle
 *            whose heading is not USABLE ("Localisation") is left untouched; if a is not usable the heading becomes a and x, y stay.
 *   weigh    the rule, the inputs and the limits of lv_occ_mcl_weigh on the resident poses (K * B <= 2^30 is judged once there
 *            are particles); n_in is kept; acc_i becomes UINT64_MAX if it or the new score is UINT64_MAX, otherwise acc_i +=
 *            score_i.  best: the least (score, index) of THIS scan's scores, as lv_occ_mcl_weigh gives it; may be NULL, and then
 *            the call does not wait for the device.  The 2^20-th weigh since the last resampling is refused (LV_ESTATE): acc < 2^60.
 *   weights  s_min = the least acc that is not UINT64_MAX; w_i = wtable[min((acc_i - s_min) >> shift, n_w - 1)], 0 where acc_i is
 *            UINT64_MAX.  n_w 1..4096, every entry <= 2^20, shift 0..63.  W = sum w, sum_w2 = sum w^2, n_eligible = the particles
 *            whose acc is not UINT64_MAX; s_min is -1 when there is none.
 *   sums     over all particles, before any resampling.  Per axis a: q_a = floorf(((p_a - origin_a) / resolution) * 256) with
 *            the origin and resolution of the field last built (reported in the statistics), clamped to +-2^22, 0 where it is
 *            not finite; n_clamped = the particles clamped or zeroed in an axis.  qs = (int)rintf(sn * 1048576.0f), qc likewise,
 *            both 0 for a heading that is not usable.  S[0..2] = sum w * q_a, S[3] = sum w * qs, S[4] = sum w * qc, in int64
 *            (below 2^62).  The estimate is origin_a + resolution * (S[a] / W + 0.5) / 256 and atan2(S[3], S[4]).
 *   decision mode 0: never; mode 2: whenever W > 0; mode 1: iff W > 0 and W^2 * below_den < below_num * K * sum_w2, exactly
 *            (n_eff < below_num / below_den * K).  1 <= below_num <= below_den <= 65536.
 *   resample systematic with M = K: C = the inclusive prefix sums of w, r = draw mod W, t_j = (j * W + r) / K, ancestor_j = the
 *            smallest i with C_i > t_j; new pose j = old pose ancestor_j, bit for bit; every acc and the weigh counter become 0;
 *            n_in is not gathered.  With W = 0 nothing moves.
 * The particles are world poses: lv_occ_configure, a field build and lv_volume_recentre leave them alone, and a weigh reads the
 * field as it stands at the call (a stale one is used as it is).  Arguments and NULLs are judged before the context (LV_EINVAL,
 * nothing written, "null context" last); then LV_ESTATE: before lv_occ_configure (every call but _info and _clear), before a field
 * build (_weigh and _resample), before _set.  A refused call changes nothing, the epoch included.  Nothing is allocated before
 * _set; _clear and lv_destroy free everything.  _move does not wait for the device. */
typedef struct lv_mcl_resample_params { int shift; int mode; uint32_t below_num, below_den; } lv_mcl_resample_params;
typedef struct lv_mcl_filter_stats {
    uint64_t W, sum_w2;
    int64_t  s_min;             /* -1: no particle is eligible */
    int64_t  S[5];
    uint32_t n_eligible, n_clamped;
    int      resampled;
    uint32_t epoch;             /* after the call */
    uint32_t since_resample;    /* weigh calls since the last resampling, after the call */
    float    origin[3];         /* of the field the sums were quantised with */
    float    resolution;
} lv_mcl_filter_stats;
typedef struct lv_mcl_filter_info { uint64_t K, seed; int set; uint32_t epoch, since_resample; } lv_mcl_filter_info;
/* shift 0, mode 1, below_num 1, below_den 2. */
void lv_default_mcl_resample_params(lv_mcl_resample_params* p);
/* poses: K x 4 floats, K 1..2^20.  acc = 0, n_in = 0, epoch = 0. */
int  lv_occ_mcl_filter_set(lv_ctx* ctx, const float* poses, size_t K, uint64_t seed);
/* delta, sigma: 3 floats each. */
int  lv_occ_mcl_filter_move(lv_ctx* ctx, const float* delta, const float* sigma);
/* beams: B x 3 floats; table: n_table values; best: 2 values or NULL. */
int  lv_occ_mcl_filter_weigh(lv_ctx* ctx, const lv_mcl_params* p, const float* beams, size_t B, const uint32_t* table, size_t n_table,
                             int64_t* best);
/* wtable: n_w values; ancestors: K values or NULL, written only when the call resampled. */
int  lv_occ_mcl_filter_resample(lv_ctx* ctx, const lv_mcl_resample_params* p, const uint32_t* wtable, size_t n_w,
                                lv_mcl_filter_stats* stats, uint32_t* ancestors);
/* poses: K x 4 floats; acc, n_in: K values; each may be NULL, not all; capacity (in particles) >= K. */
int  lv_occ_mcl_filter_get(lv_ctx* ctx, float* poses, uint64_t* acc, uint32_t* n_in, size_t capacity);
/* zeros before _set; never LV_ESTATE. */
int  lv_occ_mcl_filter_info(lv_ctx* ctx, lv_mcl_filter_info* out);
int  lv_occ_mcl_filter_clear(lv_ctx* ctx);

/* ---- TSDF and mesh -------------------------------------------------------------------------------------
 * A truncated signed distance field fused from the sweeps, and a triangle mesh of its zero surface: the TSDF layer of Voxblox
 * and nvblox with its mesh integrator ("a mesh of what the robot saw"; the reference has no counterpart).  The sweeps are the
 * lv_view of "Occupancy grid".  The volume is a grid of its own, held by the context, independent of the occupancy grid and of
 * the map.  Like every map product here the rule is integer arithmetic after one quantisation step: a pure function of the
 * inputs, bitwise reproducible, independent of scheduling.
 *   grid     origin, resolution, nx, ny, nz, min_range, max_range with the limits, the indexing (x fastest) and the quantisation
 *            (Q = 256 sub-units per voxel) of "Occupancy grid".  trunc_cells 1..16, T = trunc_cells * 256 sub-units; max_weight
 *            1..2^18; carve 0 or 1.  Each voxel holds two int32: a sum S and a weight W; W = 0 means never observed; always
 *            |S| <= T * W.
 *   returns  exactly those of "Occupancy grid": the view's origin qs (a view that gives no evidence there gives none here), the
 *            ignored returns, the CUT returns, the unfused world transform and the quantised end point qe.
 *   one ray  all in int64.  d = qe - qs, l2 = d . d (< 2^52), len = floor(sqrt(l2)) exactly (the f64 root corrected by integer
 *            comparison).  len = 0: the ray gives nothing and is not counted.  Per axis ext_a = (d_a * T) / len by truncating
 *            division (|ext_a| <= T), qb = qe + ext, qa = qe - ext.  A HIT return walks start -> qb by the walk of "Occupancy
 *            grid", where start = qs if carve != 0 or len <= T, otherwise qa.  A CUT return gives nothing and is not counted
 *            when carve = 0; with carve != 0 it walks qs -> qe and every cell takes s = T.
 *            Every cell v the walk stands in, the first and the last included, has the centre c = 256 * v + 128 per axis and
 *            s = floor((qe - c) . d / len) (floor division; always against the original qe and d).  s < -T: no contribution;
 *            s > T: s = T.  Cells outside the grid are skipped.  The cell's contribution is (dS += s, dW += 1); the walk never
 *            stands in a cell twice, so a ray contributes to a cell at most once.
 *   one call  1..32 views carrying at most 2^24 returns together (LV_EINVAL beyond).  The contributions of all rays of all
 *            views are summed per voxel, (dS, dW); integer sums commute, so neither the order of the returns nor how they are
 *            split over the views of the call matters.  Then every voxel with dW > 0 folds: Wn = W + dW, Sn = S + dS; if
 *            Wn > max_weight then S = floor(Sn * max_weight / Wn) (floor division; the product stays below 2^55) and
 *            W = max_weight, otherwise S = Sn and W = Wn.
 *   stats    rays used (the returns that walked: CUT ones only with carve), rays cut (those of them that were CUT),
 *            contributions (the sum of dW), voxels touched (those with dW > 0).
 *   metres   m = resolution * (((float)S / (float)W) / 256.0f), f32 and unfused; NaN where W = 0.  Positive between the sensor
 *            and the surface, negative behind it.
 *   mesh     naive surface nets, every step an integer.  A voxel is KNOWN iff W >= min_weight (the build's argument, >= 1) and
 *            INSIDE iff S < 0.  Cell (i, j, k), 0 <= i <= nx - 2 and likewise in y and z, has the 8 voxel centres
 *            (i..i+1, j..j+1, k..k+1) as corners; it is ACTIVE iff all 8 are known and they are not all of one sign.  A crossing
 *            sits on a cell edge from voxel A to B = A + e_a whose ends differ in sign: num = S_A * W_B,
 *            den = S_A * W_B - S_B * W_A, both negated if den < 0, t = (256 * num) / den (0..256); the crossing is A's centre
 *            (256 * A + 128) plus t along axis a.  The vertex of an active cell is, per axis, the sum of its crossings'
 *            coordinates divided by their count (1..12; every term is non-negative): int32[3] sub-units.  In metres
 *            origin_a + resolution * ((float)v_a / 256.0f), f32 and unfused.  Vertices are numbered in the order of their cell's
 *            linear index.
 *            A face comes from a grid edge (p, a), from voxel p to p + e_a, whose ends are both known and differ in sign.  With
 *            b = (a + 1) % 3 and c = (a + 2) % 3 the four cells round the edge are p offset in (b, c) by (-1, -1), (0, -1), (0, 0),
 *            (-1, 0).  The edge gives a quad iff all four exist and are active (otherwise it is counted as refused); its
 *            vertices q0..q3 are those cells' in that order if p is inside, q0, q3, q2, q1 if p is outside, so that normals point
 *            from inside to outside, towards where the sensor was.  The quad is the triangles (q0, q1, q2) and (q0, q2, q3),
 *            uint32 indices.  Faces are ordered by 3 * linear(p) + a.
 * The mesh is a SNAPSHOT of the volume at build time, as the distance field is of its grid: lv_tsdf_integrate, lv_tsdf_load and
 * lv_tsdf_clear leave it in place and set stale = 1; lv_tsdf_configure and lv_tsdf_mesh_clear free it; a new build replaces it.
 * Every call below except lv_default_tsdf_params and lv_tsdf_configure gives LV_ESTATE before lv_tsdf_configure, and
 * lv_tsdf_mesh_fetch also before a build (lv_tsdf_mesh_info reports built = 0 instead).  Arguments outside the limits give
 * LV_EINVAL and change nothing; lv_tsdf_configure's parameters are judged before the context, as lv_occ_configure's are.  The
 * calls run on the context's stream and return when their host outputs are written.  Nothing is allocated before
 * lv_tsdf_configure; lv_destroy frees everything. */
typedef struct lv_tsdf_params {
    float origin[3]; float resolution; int nx, ny, nz;
    float min_range, max_range;              /* 0 < min_range < max_range */
    int trunc_cells;                         /* 1..16 */
    int max_weight;                          /* 1..2^18 */
    int carve;                               /* 0 or 1 */
} lv_tsdf_params;
/* reserved: 1 when the built mesh carries vertex colours ("Colour layer": the layer was present at the build), otherwise 0 */
typedef struct lv_mesh_info { int built, stale, min_weight, reserved; uint64_t vertices, triangles, active_cells, refused_edges; } lv_mesh_info;
/* Defaults: the occupancy grid's footprint (0.2 m voxels, 512 x 512 x 64, origin -51.2, -51.2, -3.2, ranges 1..80 m),
 * trunc_cells 3, max_weight 10000, carve 0. */
void lv_default_tsdf_params(lv_tsdf_params* p);
/* Allocates the volume, every voxel unobserved; reconfiguring discards the volume and its mesh. */
int  lv_tsdf_configure(lv_ctx* ctx, const lv_tsdf_params* p);
/* n_views 1..32, at most 2^24 returns in all.  stats (may be NULL) as above. */
int  lv_tsdf_integrate(lv_ctx* ctx, const lv_view* views, size_t n_views, uint64_t stats[4]);
/* metres and weight (either may be NULL, not both) of the voxel each world point falls in (quantised as lv_occ_query does);
 * NaN and 0 outside the grid and for non-finite points. */
int  lv_tsdf_query(lv_ctx* ctx, const void* pts, size_t stride, size_t n, float* metres, int32_t* weight);
/* S, W, metres: nx * ny * nz values each (capacity below that: LV_EINVAL); any may be NULL, not all. */
int  lv_tsdf_fetch(lv_ctx* ctx, int32_t* S, int32_t* W, float* metres, size_t capacity);
/* Replaces the volume.  n must equal nx * ny * nz; every voxel 0 <= W <= max_weight and |S| <= T * W (LV_EINVAL otherwise,
 * volume unchanged). */
int  lv_tsdf_load(lv_ctx* ctx, const int32_t* S, const int32_t* W, size_t n);
/* Every voxel back to unobserved. */
int  lv_tsdf_clear(lv_ctx* ctx);
int  lv_tsdf_get_params(lv_ctx* ctx, lv_tsdf_params* out);
/* min_weight >= 1 (LV_EINVAL otherwise).  counts (may be NULL): vertices, triangles, active cells, edges refused for a missing
 * cell.  A volume without a surface gives LV_OK and an empty mesh. */
int  lv_tsdf_mesh_build(lv_ctx* ctx, int min_weight, uint64_t counts[4]);
/* xyz: 3 floats per vertex (metres); sub: 3 int32 per vertex (sub-units); tri: 3 uint32 per triangle.  Any may be NULL, not all.
 * cap_vertices below the vertex count with xyz or sub given, or cap_triangles below the triangle count with tri given: LV_EINVAL,
 * nothing written. */
int  lv_tsdf_mesh_fetch(lv_ctx* ctx, float* xyz, int32_t* sub, uint32_t* tri, size_t cap_vertices, size_t cap_triangles);
int  lv_tsdf_mesh_info(lv_ctx* ctx, lv_mesh_info* out);
/* Frees the mesh. */
int  lv_tsdf_mesh_clear(lv_ctx* ctx);

/* ---- Depth fusion ------------------------------------------------------------------------------------------
 * Depth-camera images fused into the TSDF volume: the projective integrator of KinectFusion, Voxblox and nvblox
 * (ProjectiveTsdfIntegrator; the reference has no counterpart).  Where lv_tsdf_integrate walks every return's ray through the
 * volume, here every voxel projects itself into every image and reads one pixel: exactly one thread owns a voxel, so there are
 * no atomics on the volume and no scratch pass, and the result is the same bits whatever the schedule.  A view is one depth
 * image with its pinhole camera and its pose camera -> world; R, t, fx, fy, cx, cy and dist mean exactly what they mean in
 * lv_camera_view ("Map painting").  Depth is z along the optical axis (the ROS convention), not range.
 *   formats    LV_DEPTH_U16: ROS 16UC1, D = (float)raw * depth_scale metres, raw 0 is "no measurement"; depth_scale finite and
 *              > 0 (0.001 for millimetres).  LV_DEPTH_F32: ROS 32FC1, metres; depth_scale is ignored.
 *   limits     1..32 views; width and height 1..8192 each, width * height <= 2^24 per view and <= 2^26 pixels per call;
 *              row_stride >= width * bytes per pixel.  `depth` needs no alignment: the rows are staged by memcpy.
 * For every voxel and every view, in view order.  Every f32 operation is a single rounded operation in the order written;
 * nothing is fused (-ffp-contract=off) and division is correctly rounded.
 *   1. centre    p_a = origin_a + resolution * ((float)(256 * i_a + 128) / 256.0f) with the volume's present origin (after its
 *                shifts): the centre of "Colour layer".
 *   2. project   "Map painting" steps 1 to 3, unchanged, with this call's min_depth, max_depth and max_norm_radius: they yield
 *                z, u, v, or the view does not judge the voxel.
 *   3. pixel     px = (int)floorf(u + 0.5f), py = (int)floorf(v + 0.5f): the nearest pixel, never an interpolation (across a
 *                depth edge that would invent a surface).
 *   4. depth     U16: raw 0 is invalid, otherwise D = (float)raw * depth_scale.  F32: D is the value.  D is invalid unless it is
 *                finite and min_depth <= D <= max_depth (NaN, +-inf, 0 and negatives fall out by that comparison).
 *   5. distance  q = floorf(((D - z) / resolution) * 256.0f), compared in f32 against (float)T.  q < -T: no contribution.
 *                q > T: s = T if carve != 0, otherwise no contribution.  Otherwise s = (int32)q.
 *   6. add       (dS += s, dW += 1).
 * After the last view every voxel with dW > 0 folds as in "TSDF and mesh" (one call), with the volume's max_weight.  Integer
 * sums commute, so neither the order of the views nor, as long as W stays below max_weight, their split over calls matters
 * (at max_weight the fold rescales, and a rescale after every call is not the rescale after all of them).
 *   stats      (voxel, view) pairs that pass step 2; those of them with a valid D; the sum of dW; voxels with dW > 0.
 * Order of judgement as for lv_colour_integrate: the arguments before the context (LV_EINVAL, nothing written; the null context
 * last), then LV_ESTATE before lv_tsdf_configure.  Once its arguments hold, and whatever it then returns, the call sets a built
 * mesh's stale = 1 and makes the next lv_surf_raycast pack the states anew, as lv_tsdf_integrate does; it leaves the colour
 * layer alone.  It runs on the context's stream and returns when stats are written.
 * Known limits: the distance is the difference in z, not the distance to the surface: on a surface seen at an angle it
 * overestimates by 1 / cos, as Voxblox and nvblox accept.  One observation weighs 1 whatever its depth, as one LiDAR ray does. */
/* Names: lv_depth_*, as the layer's calls are lv_colour_*: the set of lv_tsdf_* FUNCTIONS is closed ("Surface ray casting"). */
enum { LV_DEPTH_U16 = 0, LV_DEPTH_F32 = 1 };   /* the ROS encodings 16UC1 / 32FC1 */
typedef struct lv_depth_view {
    float R[9]; float t[3];          /* as lv_camera_view */
    float fx, fy, cx, cy;
    float dist[5];
    int   width, height;
    int   format;                    /* LV_DEPTH_* */
    float depth_scale;               /* metres per unit, U16 only */
    const void* depth; size_t row_stride;   /* bytes between rows */
} lv_depth_view;
typedef struct lv_depth_params {
    float min_depth, max_depth;      /* 0 < min_depth < max_depth: of the voxel's z and of the measured D alike */
    float max_norm_radius;           /* > 0, as lv_paint_params */
    int   carve;                     /* 0 or 1: whether free space in front of the band takes s = T */
    int   reserved;
} lv_depth_params;
/* Defaults: depth 0.3..10 m, max_norm_radius 1.5, carve 0. */
void lv_default_depth_params(lv_depth_params* p);
/* n_views 1..32.  stats (may be NULL) as above. */
int  lv_depth_integrate(lv_ctx* ctx, const lv_depth_view* views, size_t n_views, const lv_depth_params* p, uint64_t stats[4]);

/* ---- Colour layer ------------------------------------------------------------------------------------------
 * A colour layer beside the TSDF, as Voxblox and nvblox carry one, and vertex colours for the mesh: the voxels near the surface
 * take the colour of the camera images that see them (the reference's TODO "Add vision buffer and ability to paint the map's
 * points", for the surface product).  The views and their parameters are lv_camera_view and lv_paint_params of "Map painting".
 * Integer arithmetic after one float step (the projection and the sample): bitwise reproducible, independent of scheduling.
 *   layer      per voxel four uint32: C[0..2], the sums of R, G, B, and the colour weight Wc.  Wc = 0: never coloured.  Always
 *              C[c] <= 255 * Wc and Wc <= 65535.  16 bytes per voxel, allocated by the first lv_colour_integrate or
 *              lv_colour_load, never before: a context that calls neither allocates nothing for it (lv_colour_info: present = 0).
 *   candidates a voxel is a candidate iff W >= min_weight and |S| <= (int64)band * W; band in sub-units, 1..T; min_weight >= 1.
 *              Judged once per call, against the volume as the call finds it.
 *   centre     per axis p_a = origin_a + resolution * ((float)(256 * i_a + 128) / 256.0f), f32 and unfused, origin the volume's
 *              present origin (after its shifts): the mesh's vertex in metres at v = 256 i + 128.
 *   views      the candidates' centres are the point set of "Map painting" steps 1 to 6, unchanged: the depth gate, the
 *              normalised radius, plumb_bob, the image bounds, the occlusion buffer filled by the candidates themselves with its
 *              window-min, SEEN iff z - zbuf <= fmaxf(margin_abs, margin_rel * z), the bilinear sample s in f32.  blend must be 0
 *              (LV_EINVAL otherwise); the limits on views and images are lv_map_paint's.
 *   quantise   per seeing view and channel q = (uint32_t)(s + 0.5f), in 0..255.
 *   accumulate per candidate n = the number of seeing views and dC[c] = the sum of their q: integer sums, so neither the order
 *              of the views nor their split inside one call matters.
 *   fold       every candidate with n > 0: Wn = Wc + n, Cn[c] = C[c] + dC[c]; if Wn > max_weight (1..65535) then
 *              C[c] = (uint32)(((uint64)Cn[c] * max_weight) / Wn) and Wc = max_weight, otherwise C = Cn and Wc = Wn.
 *   voxel      colour of a voxel: Wc > 0: c = (2 * C[c] + Wc) / (2 * Wc) by integer division, alpha 255; Wc = 0: 0, 0, 0, 0.
 *   vertex     colour of a mesh vertex: of the 8 corner voxels of its active cell those with Wc > 0, k their number and sum[c] the
 *              sum of their voxel colours; k > 0: (2 * sum[c] + k) / (2 * k), alpha 255; k = 0: 0, 0, 0, 0.  Computed inside
 *              lv_tsdf_mesh_build when the layer is present: a snapshot with the mesh, in vertex order.
 *   stats      candidates, (voxel, view) pairs that pass steps 1 to 3, pairs seen, voxels with n > 0.
 * Order of judgement as for the TSDF calls: the arguments before the context (LV_EINVAL, nothing written; the null context last),
 * then LV_ESTATE before lv_tsdf_configure, then what is the call's own (band > T: LV_EINVAL).  Without a layer lv_colour_fetch and
 * lv_colour_query give LV_ESTATE and lv_colour_clear is LV_OK and does nothing; lv_mesh_colours gives LV_ESTATE without a mesh
 * or with a mesh built while no layer was present.  lv_colour_integrate (whatever it returns once its arguments hold),
 * lv_colour_load and lv_colour_clear set a built mesh's stale = 1.  lv_tsdf_load and lv_tsdf_clear zero the layer (colours of
 * another volume mean nothing), lv_tsdf_integrate leaves it alone, lv_tsdf_configure and lv_destroy free it, and
 * lv_volume_recentre(LV_VOLUME_SURFACE) moves it with S and W: new voxel (i, j, k) holds what (i + d) held or four zeros, no
 * surviving bit changes, a zero shift touches nothing.
 * Known limits: a voxel behind a wall thinner than the band takes the colour of a camera that looks at the wall's back, and only
 * the candidates occlude: what the TSDF has not observed hides nothing. */
typedef struct lv_colour_params { lv_paint_params view; int band; int min_weight; int max_weight; int reserved; } lv_colour_params;
/* coloured: the voxels with Wc > 0, counted at the call.  (A struct tag without a typedef: the call below has the name.) */
struct lv_colour_info { int present, reserved; uint64_t voxels, coloured; };
/* Defaults: lv_default_paint_params but zbuf_scale 8, window 1, margin_abs 0.5; band 256, min_weight 1, max_weight 64. */
void lv_default_colour_params(lv_colour_params* p);
/* n_views 1..32.  stats (may be NULL) as above. */
int  lv_colour_integrate(lv_ctx* ctx, const lv_camera_view* views, size_t n_views, const lv_colour_params* p, uint64_t stats[4]);
/* sums: 4 uint32 per voxel (C[0], C[1], C[2], Wc); rgba: the voxel colours, 4 bytes per voxel.  Either may be NULL, not both;
 * capacity (voxels) below nx * ny * nz: LV_EINVAL. */
int  lv_colour_fetch(lv_ctx* ctx, uint32_t* sums, uint8_t* rgba, size_t capacity);
/* Replaces the layer.  n (voxels) must equal nx * ny * nz and every voxel keep the invariants above (LV_EINVAL otherwise, layer
 * unchanged). */
int  lv_colour_load(lv_ctx* ctx, const uint32_t* sums, size_t n);
/* The voxel colour of the voxel each world point falls in (quantised as lv_tsdf_query does); 0, 0, 0, 0 outside the grid. */
int  lv_colour_query(lv_ctx* ctx, const void* pts, size_t stride, size_t n, uint8_t* rgba);
/* Every voxel back to never coloured; keeps the allocation. */
int  lv_colour_clear(lv_ctx* ctx);
int  lv_colour_info(lv_ctx* ctx, struct lv_colour_info* out);
/* rgba: 4 bytes per vertex of the mesh last built, in vertex order; cap_vertices below the vertex count: LV_EINVAL. */
int  lv_mesh_colours(lv_ctx* ctx, uint8_t* rgba, size_t cap_vertices);

/* ---- Surface ray casting ---------------------------------------------------------------------------------
 * What a sensor would see of the TSDF surface from a pose: sub-voxel depth, the surface normal and the surface colour per ray,
 * as the ray casters of Voxblox and nvblox give them, for rendered depth and colour views of the reconstruction and for
 * synthetic scans in model-based localisation (the reference has no counterpart).  The walk of "Occupancy grid", unchanged, as
 * "Ray casting" runs it, READING S, W and the colour layer.  Every step after the quantisation of a ray's ends is integer
 * arithmetic (the normal: a fixed sequence of unfused f32 operations), so every output is a pure function of the volume and the
 * arguments, the same bits whatever the schedule.
 *   grid     the TSDF volume's, at its present origin (after its shifts).
 *   ends     lv_surf_raycast: exactly lv_occ_raycast's ("Ray casting", ends): `from` as a view's sensor origin, `to` as a return's
 *            world point; a ray one of whose ends fails (non-finite included) is IGNORED.  So |d_a| < 2^25 per axis for
 *            d = qe - qs, and l2 = d . d < 2^52: every product below fits in int64.
 *   cells    c_0 .. c_S, a_s and num_s / den_s as in "Ray casting".  A cell inside the grid is KNOWN iff W >= min_weight (the
 *            call's parameter, >= 1); a KNOWN cell is IN iff S < 0, otherwise OUT; an in-grid cell that is not KNOWN is UNKNOWN.
 *            Cells outside the grid have no state: they neither stop a ray nor count.
 *   stop     s* is the least s whose c_s is IN; c_0 is examined like every other cell.  The ray is a HIT iff s* >= 1 and
 *            c_(s* - 1) is inside the grid and OUT; then B = c_s* and A = c_(s* - 1).  Otherwise it is BLOCKED: it starts inside
 *            the surface, or enters it from unobserved space or from outside the grid.  A ray with no such s is CLEAR.  UNKNOWN
 *            cells are passed: a LiDAR volume fused without carve is unobserved in front of its truncation band, and a caster that
 *            stopped there would see nothing.
 *   depth    in sub-units along the ray, with len = floor(sqrt(l2)) exactly.  HIT: t = the mesh's crossing of the edge A -> B
 *            (num = S_A W_B, den = num - S_B W_A, t = (256 num) / den, in 0..256); u_A = (256 A + 128 - qs) . d;
 *            u = u_A + |d_a| t with a = a_s*, clamped to [0, l2]; depth = floor(u / len).  (B = A +- e_a, so the centres'
 *            projections on the ray are 256 |d_a| apart: u is the zero of the TSDF interpolated linearly between them; a step
 *            happened, so len >= 1.)  BLOCKED: depth = floor(num_s* len / den_s*), 0 for s* = 0; t = -1.  CLEAR: depth = len, t = -1.
 *            Metres: resolution * ((float)depth / 256.0f), f32 and unfused; the caller's business.
 *   record   HIT / BLOCKED: cell = the linear index of c_s*; steps = s*; axis = a_s* (-1 when s* = 0); n_known and n_unknown count
 *            the in-grid OUT and UNKNOWN cells among c_0 .. c_(s* - 1).  CLEAR: cell = the linear index of ve, -1 outside the
 *            grid; steps = S; axis = -1; the counts run over c_0 .. c_S.  IGNORED: status 0, cell -1, every other field 0.
 *   normal   (optional, 3 f32 per ray; zeros for everything but a HIT) with phi(v) = (float)S_v / (float)W_v the gradient at B:
 *            per axis a, both neighbours B +- e_a KNOWN: g_a = phi(+) - phi(-); only one KNOWN: g_a = 2.0f * (phi(+) - phi(B)) or
 *            2.0f * (phi(B) - phi(-)); a neighbour outside the grid is not KNOWN.  If on any axis neither neighbour is KNOWN the
 *            normal is zeros.  n = g / sqrtf((g_x g_x + g_y g_y) + g_z g_z), f32 and unfused in exactly that order, zeros when the
 *            norm is not > 0.  It points from inside to outside, towards where the sensor was, as the mesh's faces do.
 *   colour   (optional, 4 bytes per ray; 0, 0, 0, 0 for everything but a HIT) the voxel colour ("Colour layer", voxel) of B if its
 *            Wc > 0, otherwise of A if its Wc > 0, otherwise 0, 0, 0, 0.  Without a layer: 0, 0, 0, 0 everywhere, LV_OK, and
 *            nothing is allocated for the layer.
 *   views    lv_surf_raycast_views: 1..32 lv_view whose returns are the end points of a scan pattern in the sensor frame, at most
 *            2^24 returns together.  qs, qe and which returns are ignored or cut are exactly those of lv_tsdf_integrate /
 *            lv_occ_view_gain for the same view; cut and hit returns alike are rays qs -> qe.  Results are written for every
 *            return of every view, in order; ignored returns, and every return of a view that gives no evidence, are IGNORED.
 *            stats: rays used, HIT, BLOCKED, CLEAR.
 * Both calls read the LIVE volume and layer and change no bit of them, of the mesh or of any stale flag.  The walk reads a packed
 * copy of the states (2 bits per voxel), rebuilt by the first call after the volume changed or when min_weight differs from the
 * packed one; nothing is allocated before the first call, and lv_tsdf_configure and lv_destroy free everything.  Order of
 * judgement as for the colour calls: parameters and NULL or short arguments before the context (min_weight < 1, strides below 12,
 * NULL out, capacity below the returns: LV_EINVAL, nothing written; the null context last), then LV_ESTATE before
 * lv_tsdf_configure.  The calls run on the context's stream and return when their host outputs are written. */
/* Names: the calls and the states are lv_surf_* / LV_SURF_* ("surface"), the two structs lv_tsdf_ray_*: the set of lv_tsdf_*
 * FUNCTIONS is closed (the volume and its mesh, "TSDF and mesh"), as lv_mesh_colours stands outside lv_colour_*. */
#define LV_SURF_IGNORED 0
#define LV_SURF_CLEAR   1
#define LV_SURF_HIT     2
#define LV_SURF_BLOCKED 3
typedef struct lv_tsdf_ray_params { int min_weight; int reserved; } lv_tsdf_ray_params;
typedef struct lv_tsdf_ray_result {           /* 32 bytes */
    int32_t status, cell, steps, axis, depth, t, n_known, n_unknown;
} lv_tsdf_ray_result;
/* min_weight 1. */
void lv_default_surf_ray_params(lv_tsdf_ray_params* p);
/* from, to: n world points each, the first three floats of every stride bytes (strides >= 12); out: n results; normals (3 floats
 * per ray) and rgba (4 bytes per ray) may be NULL.  n = 0 succeeds and writes nothing; n < 2^31 - 1. */
int  lv_surf_raycast(lv_ctx* ctx, const lv_tsdf_ray_params* p, const void* from, size_t from_stride, const void* to, size_t to_stride,
                     size_t n, lv_tsdf_ray_result* out, float* normals, uint8_t* rgba);
/* n_views 1..32; out, normals, rgba: one entry per return of every view, in order; capacity (entries) below the returns:
 * LV_EINVAL.  normals, rgba and stats may be NULL. */
int  lv_surf_raycast_views(lv_ctx* ctx, const lv_tsdf_ray_params* p, const lv_view* views, size_t n_views, lv_tsdf_ray_result* out,
                           float* normals, uint8_t* rgba, size_t capacity, uint64_t stats[4]);

/* ---- Rolling volumes -------------------------------------------------------------------------------------
 * The occupancy grid and the TSDF volume follow the robot (costmap_2d's rolling_window, the local maps of Voxblox / nvblox, the
 * ring buffers of FIESTA / ego-planner; the reference has no counterpart).  lv_volume_recentre moves a volume by whole voxels:
 * the contents stay where they are in the world, the box moves, what leaves it is forgotten and what enters it is never
 * observed.  Nothing is interpolated: no bit of a surviving value changes.
 *   rule     a volume keeps the origin it was configured with, origin0, and an accumulated shift s[3] (int32 voxels, zero after
 *            configure).  A recentre by d[3]: s' = s + d; origin'[a] = origin0[a] + (float)s'[a] * resolution (f32, unfused, in
 *            that order: the origin depends on s' alone, so +d then -d gives back origin0 bit for bit); new voxel (i, j, k) holds
 *            what old voxel (i + d_x, j + d_y, k + d_z) held if that lies inside the grid, otherwise it is never observed (NaN,
 *            bits 0x7FC00000, in the occupancy grid; S = 0, W = 0 in the TSDF).  |d[a]| <= 2^20, |s'[a]| <= 2^20 and origin'
 *            finite (LV_EINVAL otherwise, nothing changes).  |d[a]| >= n_a is legal and leaves every voxel never observed.
 *            d = (0, 0, 0) does nothing at all: nothing goes stale, no buffer is touched, the stats are zero.
 *   after    a non-zero recentre of LV_VOLUME_OCC: lv_occ_get_params reports origin'; the distance field and the frontier are
 *            stale (as after lv_occ_integrate) and the next ray cast classifies the grid anew.  The field and the plan are
 *            snapshots with their own origin: lv_occ_distance_query, lv_occ_plan_paths and lv_occ_rollout go on answering for
 *            the same world points with the same bits.  The frontier's cells are indices: lv_occ_frontier_rank gives LV_ESTATE
 *            unless the frontier and the plan were both built at the grid's present accumulated shift (lv_volume_shift_info
 *            reports the three), that is until field, plan and frontier have been rebuilt.  Of LV_VOLUME_SURFACE:
 *            lv_tsdf_get_params reports origin'; a built mesh is stale (its vertices are metres and stay right).
 *   mark     lv_occ_mark fills voxels from points, the way back from the map to the grid: a strip the grid has just scrolled
 *            into is unknown to it although the point map may know it.  Source as lv_elev_build: pts = NULL reads the living
 *            points of the device map (after the insert in flight has settled), otherwise n < 2^31 caller points, stride >= 12.
 *            A point is used iff it quantises into the grid ("Occupancy grid") and its voxel lies in the inclusive box lo..hi
 *            clipped to the grid (a box that is empty after clipping marks nothing).  Per voxel the integer count c of the points
 *            used; a voxel with c >= min_points (1..2^20) is a candidate.  only_unknown != 0: a candidate whose L is NaN gets
 *            L = fminf(fmaxf(l_mark, l_min), l_max), any other is left alone (ray evidence is never overridden).
 *            only_unknown == 0: every candidate gets L = fminf(fmaxf((isnan(L) ? 0 : L) + l_mark, l_min), l_max), once per call.
 *            l_mark finite and non-zero; a negative value marks free space.  A pure function of the point set, in any order.
 *            The field and the frontier go stale iff a voxel was written.
 * The arguments are judged before the context (LV_EINVAL, the null context last), then LV_ESTATE if the volume is not configured,
 * then the accumulated shift.  The occupancy grid's second buffer (nx * ny * nz floats) is allocated by the first non-zero
 * recentre or the first lv_occ_mark and kept until lv_occ_configure; the TSDF moves through the scratch it already has. */
#define LV_VOLUME_OCC     0   /* the occupancy grid */
#define LV_VOLUME_SURFACE 1   /* the TSDF volume */
typedef struct lv_volume_shifts {
    int32_t grid[3], surface[3];             /* accumulated shift of each volume (0 if not configured) */
    int32_t field[3], plan[3], frontier[3];  /* the grid shift each snapshot was built at (0 if not built) */
} lv_volume_shifts;
/* stats (may be NULL): voxels kept, voxels exposed (now never observed), voxels that held evidence (L not NaN; W > 0) and left
 * the volume, 0. */
int  lv_volume_recentre(lv_ctx* ctx, int volume, const int32_t shift[3], uint64_t stats[4]);
int  lv_volume_shift_info(lv_ctx* ctx, lv_volume_shifts* out);
typedef struct lv_occ_mark_params { int lo[3], hi[3]; int min_points; int only_unknown; float l_mark; } lv_occ_mark_params;
/* Defaults: the whole grid (lo 0, hi 2^30), min_points 1, only_unknown 1, l_mark 0.85. */
void lv_default_occ_mark_params(lv_occ_mark_params* p);
/* stats (may be NULL): points used, voxels holding >= min_points, voxels marked, voxels left alone because they were observed. */
int  lv_occ_mark(lv_ctx* ctx, const lv_occ_mark_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]);

/* ---- Occupancy from the surface --------------------------------------------------------------------------
 * The way from the TSDF volume to the occupancy grid (the TSDF -> ESDF / costmap step of Voxblox and nvblox; the reference has no
 * counterpart).  lv_occ_from_surface classifies the volume's voxels into solid, open and unknown, optionally grows the solid ones
 * by whole voxels, and writes the result into the occupancy grid on the device, in the grid's own terms: everything built from
 * the grid (distance field, plans, frontiers, rays, localisation, lv_occ_project) then works for a robot that fuses depth images,
 * and the distance field of such a grid is the ESDF of the surface.  One f32 step, integers after it: a pure function of the
 * volume, the grid and the parameters, bitwise reproducible.
 *   voxels   with S, W as in "TSDF and mesh", a TSDF voxel is KNOWN iff W >= min_weight (1..2^18), SOLID iff KNOWN and
 *            (int64)S <= (int64)band * W (its fused distance is at most band / 256 voxel; band in -4096..4096: 0 gives the
 *            voxels on or behind the surface, a positive band thickens walls towards the sensor, a band beyond +-T makes
 *            everything known, or nothing, solid), OPEN iff KNOWN and not SOLID.
 *   class    of voxel v = (i, j, k) of the inclusive box lo..hi clipped to the grid as lv_occ_mark's.  Its centre is
 *            c_a = origin_g[a] + (((float)v_a + 0.5f) * resolution_g), f32, unfused, in that order; c is quantised in the volume
 *            as lv_tsdf_query quantises a point (occ_quant of "Occupancy grid" against the volume's origin and resolution, then
 *            q >> 8), which gives the TSDF voxel u.  An axis that does not quantise, or u outside the volume: v is OUTSIDE, its
 *            class NONE.  Otherwise OCCUPIED iff any TSDF voxel u + d, d in [-reach, reach]^3 (reach 0..4), inside the volume, is
 *            SOLID; else FREE iff u itself is OPEN; else NONE.  Free space is never grown: unknown space is never declared free
 *            by a neighbour.  Both volumes stand at their current origins, origin0 + (float)shift * resolution ("Rolling
 *            volumes"), and may differ in origin, resolution, shape and shift.
 *   write    with a = fminf(fmaxf(l_solid, l_min), l_max) and b = fminf(fmaxf(l_open, l_min), l_max) from the grid's clamps
 *            (l_solid, l_open finite, l_open < 0 < l_solid):
 *              LV_OCC_SURFACE_FILL        only where L is NaN: OCCUPIED -> a, FREE -> b.  Observed voxels and NONE are left alone:
 *                                         ray evidence is never overridden (lv_occ_mark's only_unknown).
 *              LV_OCC_SURFACE_OVERWRITE   the same whatever L held; NONE is left alone.
 *              LV_OCC_SURFACE_REPLACE     as OVERWRITE, and NONE -> never observed (bits 0x7FC00000): inside the box the grid
 *                                         becomes a pure function of the volume.
 *              LV_OCC_SURFACE_ACCUMULATE  OCCUPIED -> fminf(fmaxf((isnan(L) ? 0 : L) + l_solid, l_min), l_max), FREE the same with
 *                                         l_open, once per call; NONE is left alone.  Surface evidence adds to LiDAR evidence.
 *            Every value written is NaN or lies in [l_min, l_max].  The field and the frontier go stale iff a voxel's 32 bits
 *            changed; nothing of the volume, its colour layer, its mesh or its packed ray states is touched.
 * The parameters are judged before the context (LV_EINVAL, messages prefixed "lv_occ_from_surface: ", the null context last), then
 * LV_ESTATE without an occupancy grid, then LV_ESTATE without a TSDF volume; a box that is empty after clipping gives LV_OK and
 * zero stats before anything else is touched.  Three bitmaps of the volume (one bit per voxel each) are allocated by the first
 * call and kept until lv_occ_configure. */
#define LV_OCC_SURFACE_FILL        0
#define LV_OCC_SURFACE_OVERWRITE   1
#define LV_OCC_SURFACE_REPLACE     2
#define LV_OCC_SURFACE_ACCUMULATE  3
typedef struct lv_occ_surface_params {
    int lo[3], hi[3];        /* inclusive voxel box of the occupancy grid, clipped to it as lv_occ_mark's */
    int min_weight;          /* 1..2^18 */
    int band;                /* -4096..4096, in 1/256 voxel of the TSDF */
    int reach;               /* 0..4 TSDF voxels */
    int mode;                /* one of the four above */
    float l_solid, l_open;   /* finite, l_open < 0 < l_solid */
} lv_occ_surface_params;
/* Defaults: the whole grid (lo 0, hi 2^30), min_weight 1, band 0, reach 0, mode LV_OCC_SURFACE_FILL, l_solid 3.5, l_open -2.0. */
void lv_default_occ_surface_params(lv_occ_surface_params* p);
/* stats (may be NULL): voxels of the box classed OCCUPIED, classed FREE, voxels whose 32 bits changed, voxels of the box that are
 * OUTSIDE. */
int  lv_occ_from_surface(lv_ctx* ctx, const lv_occ_surface_params* p, uint64_t stats[4]);

/* ---- Localizator side ----------------------------------------------------------------------- */
/* `this->points2match = points`                   — src/Modules/Localizator.cpp:131.
 * Uploads the scan (LiDAR frame) once per correct(); it is invariant across IKFoM passes. */
int lv_scan_set(lv_ctx* ctx, const void* points, size_t stride, size_t n);

/* ---- row f-2: Compensator on the device ------------------------------------------------------------------
 * f32 members of the reference's `State` that State::propagate_f reads (include/Headers/Objects.hpp:97-137,
 * src/Objects/State.cpp:94-110); matrices row-major.  184 bytes. */
typedef struct lv_motion_state {
    float R[9], pos[3], vel[3], bw[3], ba[3], g[3], RLI[9], tLI[3], a[3], w[3];
    float pad_[2];
    double time;
} lv_motion_state;

/* Compensator::compensate(states, Xt2, points) + Compensator::downsample (src/Modules/Compensator.cpp:123-163):
 * de-skews a time-stamped raw scan (records: x,y,z floats at offset 0, a double time stamp at `time_offset`
 * bytes — 16 for the reference's Point) with the piecewise-constant-IMU motion model of State::propagate_f
 * over `states` (time-ordered, surrounding the points), moves every point into the LiDAR frame of Xt2 and,
 * if downsample_prec > 0, voxel-grid down-samples it (pcl::VoxelGrid semantics: centroid per leaf).  The
 * result becomes the current scan exactly as if lv_scan_set had been called with it. */
int lv_scan_deskew(lv_ctx* ctx, const void* points, size_t stride, size_t time_offset, size_t n,
                   const lv_motion_state* states, size_t n_states, const lv_motion_state* Xt2, float downsample_prec);
/* Compensator::downsample(points) on its own (src/Modules/Compensator.cpp:104-107,148-163): the same voxel grid for
 * points that are already compensated (downsample_prec <= 0: the points become the scan as they are, = lv_scan_set). */
int lv_scan_downsample(lv_ctx* ctx, const void* points, size_t stride, size_t n, float downsample_prec);
/* number of points of the current scan / copy them out (xyz packed, de-skew output order) */
/* ---- row f-4: LiDAR wire formats (sensor_msgs/PointCloud2 -> the reference's time-stamped Points) -------------
 * lv_cloud_ingest = Accumulator::process (src/Modules/Accumulator.cpp:143-153): PointCloudProcessor::msg2points
 * for the velodyne / hesai / ouster / custom point types (src/Utils/PointCloudProcessor.cpp:24-97 with the time
 * rules of src/Objects/Point.cpp:37-111), ::downsample (every downsample_rate-th point whose |p| > min_dist,
 * :99-110) and ::sort_points (by time, :112-121), followed by Accumulator::push of every point (:141) — into a
 * device-resident LiDAR buffer (BUFFER_L).  `data` = msg.data (n_points records of format->point_step bytes; the
 * field offsets come from msg.fields, lv_cloud_format_preset gives the PCL in-memory layouts of
 * include/Headers/Common.hpp:109-221).  lv_cloud_fetch = Accumulator::get_points(t1, t2) (t1 <= time <= t2, oldest
 * first; records are the reference's 32-byte Point: x,y,z floats, double time at 16, intensity, range);
 * lv_cloud_clear = Accumulator::clear_lidar(t) (drops time <= t from the old end; applied by the next window kernel, or by
 * whatever needs the buffer's true extent first);
 * lv_scan_deskew_window = the point half of Compensator::compensate(t1, t2) (src/Modules/Compensator.cpp:18-35):
 * the buffered points of [t1, t2] are de-skewed exactly as lv_scan_deskew does, without leaving the device. */
enum { LV_LIDAR_VELODYNE = 0, LV_LIDAR_HESAI = 1, LV_LIDAR_OUSTER = 2, LV_LIDAR_CUSTOM = 3 };
enum { LV_TIME_F32_SEC = 0, LV_TIME_F64_SEC = 1, LV_TIME_U32_NSEC = 2 };
enum { LV_ATTR_NONE = 0, LV_ATTR_F32 = 1, LV_ATTR_U8 = 2, LV_ATTR_U16 = 3, LV_ATTR_U32 = 4 };
typedef struct lv_cloud_format {
    uint32_t point_step;            /* msg.point_step */
    uint32_t off_x, off_y, off_z;   /* FLOAT32 fields */
    uint32_t off_time;              /* velodyne `time` (F32 s), hesai / custom `timestamp` (F64 s), ouster `t` (U32 ns) */
    int time_type;                  /* LV_TIME_* */
    uint32_t off_intensity;         /* `intensity` (F32; hesai U8) or ouster `reflectivity` (U16) */
    int intensity_type;             /* LV_ATTR_* */
    uint32_t off_range;             /* ouster `range` (U32); LV_ATTR_NONE: range = |p| */
    int range_type;
    int relative_time;              /* 1: stamps relative to the header stamp (velodyne, ouster); 0: absolute */
} lv_cloud_format;
typedef struct lv_ingest_params {   /* config/params.yaml:29-35 */
    uint64_t header_stamp_usec;     /* pcl header stamp (microseconds) */
    int stamp_beginning;
    int offset_beginning;
    double full_rotation_time;
    int downsample_rate;
    float min_dist;
} lv_ingest_params;
int    lv_cloud_format_preset(int lidar_type, lv_cloud_format* out);
int    lv_cloud_ingest(lv_ctx* ctx, const void* data, size_t n_points, const lv_cloud_format* format, const lv_ingest_params* params,
                       size_t* n_kept);
size_t lv_cloud_size(lv_ctx* ctx);
int    lv_cloud_fetch(lv_ctx* ctx, double t1, double t2, void* points_out, size_t capacity, size_t* n);
int    lv_cloud_clear(lv_ctx* ctx, double t);
/* Optional: allocate the ingest staging (two pinned buffers + the device work arrays) for messages of up to
 * max_points_per_message records of point_step bytes and a LiDAR buffer of buffer_points points now, instead of on the first
 * message (pinned allocations take milliseconds: the first sweep of a stream otherwise pays them). */
int    lv_cloud_reserve(lv_ctx* ctx, size_t max_points_per_message, size_t point_step, size_t buffer_points);
/* Optional: size the work buffers of the 100 Hz cycle now — the de-skew / voxel-grid buffers for windows of up to
 * max_window_points raw points, the scan / hand-over / insert buffers for scans of up to max_scan_points points — instead of
 * growing them (allocate, synchronise, free) during the first cycles of a stream. */
int    lv_reserve_stream(lv_ctx* ctx, size_t max_window_points, size_t max_scan_points);
int    lv_scan_deskew_window(lv_ctx* ctx, double t1, double t2, const lv_motion_state* states, size_t n_states,
                             const lv_motion_state* Xt2, float downsample_prec, size_t* n_window);

size_t lv_scan_size(lv_ctx* ctx);
/* Which chain produced the current scan in the last lv_scan_deskew / lv_scan_downsample / lv_scan_deskew_window call: the
 * one-launch chain for windows of up to 2048 points (SMALL), the two-launch chain for windows of up to 16 384 points from the
 * LiDAR buffer (LARGE), or the general chain (GENERAL: also when one of the others declined and the general chain ran
 * instead).  NONE: no such call yet, a call without points, or the scan was uploaded with lv_scan_set.  All three chains
 * produce the same bits; this is for tests and diagnostics.  Reads a host field: no device work, no wait. */
#define LV_SCAN_ROUTE_NONE    0
#define LV_SCAN_ROUTE_SMALL   1
#define LV_SCAN_ROUTE_LARGE   2
#define LV_SCAN_ROUTE_GENERAL 3
int    lv_scan_route(lv_ctx* ctx);
int    lv_scan_fetch(lv_ctx* ctx, float* xyz_out, size_t capacity);

/* One IKFoM::h_share_model evaluation (registered at src/Modules/Localizator.cpp:112) =
 * Mapper::match (Mapper.cpp:40-56) + Localizator::calculate_H (Localizator.cpp:29-57), reduced to
 * H^T H / H^T h on the GPU.  Synchronous. */
int lv_iterate(lv_ctx* ctx, const lv_state* x, lv_sums* out);

/* The Eigen-free half of IKFoM::h_share_model for an UNMODIFIED esekf loop (src/Modules/Localizator.cpp:105-117: the callback
 * update_iterated_dyn_share_modified calls; :132 the update): esekf depends on the N x 12 Jacobian and the residuals only
 * through H^T H and H^T h, so the callback hands it a pseudo measurement of *rows <= 12 rows with
 *     h_x^T h_x = sums->HTH      h_x^T h = sums->HTh
 * (h_x row-major, 12 columns = the first 12 tangent coordinates, rows >= *rows zero).  Without estimate_extrinsics: the upper
 * Cholesky factor of the leading 6 x 6 block padded with zero columns (6 rows; Localizator.cpp:52 zeroes columns 6..11);
 * with it, or if that block is not positive definite: the rank-revealing factor sqrt(lam) V^T of the symmetric eigen-
 * decomposition (12 / 6 rows, the rows of vanished eigenvalues zero).  sums->n_valid == 0 (dyn_share.valid = false) gives
 * *rows = 0.  Host arithmetic only: needs no context and no device.  The maintainer's h_share_model is then
 *     lv_iterate(ctx, &x, &sums); lv_pseudo_measurement(&sums, ext, hx, h, &rows); copy hx / h into dyn_share.h_x / .h
 * (both esekf gain branches checked in tests/test_hshare.py). */
int lv_pseudo_measurement(const lv_sums* sums, int estimate_extrinsics, double h_x[144], double h[12], int* rows);

/* esekf::update_iterated_dyn_share_modified(R, degeneracy_threshold, solve_time, print)
 *                                                 — call site src/Modules/Localizator.cpp:132.
 * Runs the whole iterated update on the device.  x and P (23x23 row-major) are updated in place.
 * passes (may be NULL) receives the number of measurement passes executed; per_pass (may be NULL)
 * receives the sums of each pass (capacity MAX_NUM_ITERS+1); trace (may be NULL) receives per pass
 * 23 doubles dx_ followed by the 26 state doubles after boxplus (49 x (MAX_NUM_ITERS+1)). */
int lv_update(lv_ctx* ctx, lv_state* x, double* P, int* passes, lv_sums* per_pass, double* trace);

/* ---- resident filter (row f-3): x and P stay on the device between prediction and correction -----------
 * lv_filter_set / lv_filter_get     = esekf::change_x + change_P / get_x + get_P (src/Modules/Localizator.cpp:136-152)
 * lv_predict(dt, Q, acc, gyro)      = esekf::predict(dt, Q, in) as called by Localizator::propagate
 *                                     (Localizator.cpp:159-173; Q row-major 12x12, acc = imu.a, gyro = imu.w)
 * lv_correct(passes)                = lv_update on the resident state; asynchronous when passes == NULL.
 * lv_filter_set itself neither uploads nor waits (round 4): the filter stays in pinned host memory until something needs it on the
 * device; an lv_correct that follows takes it along in its first launch's kernel arguments (as lv_update takes its x / P), so "set
 * the prior, correct" is two enqueue-only calls — bench.py's timed step.
 * Nothing here waits for the device except lv_filter_get and lv_correct with passes != NULL: lv_predict calls are queued (up to
 * eight steps with the same Q go out as one launch when something needs the filter: lv_correct, lv_filter_get, lv_map_add_scan,
 * lv_synchronize, an update by value); after lv_correct the posterior stays in the update's working copy until something needs
 * it elsewhere, and lv_filter_get reads it — and the pass count, lv_last_passes — from the host-mapped mailbox the update's
 * finishing pass writes (a poll, no copy).  The results are bit-identical to one launch per call with eager copies
 * (tests/test_gpu_filter.py). */
int lv_filter_set(lv_ctx* ctx, const lv_state* x, const double* P);
int lv_filter_get(lv_ctx* ctx, lv_state* x, double* P);
int lv_predict(lv_ctx* ctx, double dt, const double* Q, const double acc[3], const double gyro[3]);
int lv_correct(lv_ctx* ctx, int* passes);
/* Eigenvalues of the pose block (pos, rot) of H^T H of every pass of the last update run with degeneracy_mode >= 1:
 * eig receives n_passes x 6 doubles (capacity_passes rows available; Jacobi order, unsorted).  A REPORT, not a filter input:
 * updates that ran one launch per pass derive the values on the host from the logged sums, the three-kernel path derives them on
 * the device (FMA-contracted), both by the same fixed 8 cyclic Jacobi sweeps; the two agree to rounding, not bit for bit —
 * stated and tested tolerance 1e-9 relative to the largest eigenvalue (tests/test_gpu_configs.py, tests/test_gpu_parity.py). */
int lv_get_degeneracy_values(lv_ctx* ctx, double* eig, int capacity_passes, int* n_passes);

/* ---- Aiding observations -----------------------------------------------------------------------------
 * Measurements other than the scan — a GPS or barometer position, a wheel or Doppler velocity, a zero-velocity update, an AHRS
 * attitude — applied to the resident filter on the device as one more update of the same error-state filter, in order with the
 * queued lv_predict calls and without a host round trip:  lv_filter_set -> lv_predict ... -> lv_observe -> lv_correct -> lv_filter_get.
 *
 * dofs as lv_predict: pos 0, rot 3, offR 6, offT 9, vel 12, bg 15, ba 18, grav 21 (2); rot [+] d = R Exp(d).  R = the rotation
 * matrix of x.rot, p = x.pos, v = x.vel:
 *   kind            h(x)           innovation y            non-zero blocks of H (3 x 23): first, second
 *   POSITION        p + R lever    z - h                   pos: I              rot: -(R hat(lever))
 *   VELOCITY_WORLD  v              z - h  (ZUPT: z = 0)    vel: I              -
 *   VELOCITY_BODY   R^T v          z - h                   vel: R^T            rot: hat(R^T v)
 *   ATTITUDE        -              so3_log(q^-1 (x) z)     rot: I              -       (first order in y: the right Jacobian of
 *                                                                                       the logarithm is taken as I)
 * Rule per observation, all f64; the rows k = 0..m-1 are the components whose mask bit is set, ascending (m = popcount(mask));
 * H_k, y_k, R_kl below are the rows / entries of those components.  Every sum starts at 0.0 and adds its terms left to right in
 * the order written; "blocks" means the first block's three columns in ascending order, then the second block's:
 *   1. PHt[i][k] = sum over blocks of P[i][c] H_k[c]                          (23 x m)
 *      S[k][l]   = (sum over blocks of H_k[c] PHt[c][l]) + R_kl               (l <= k: the lower triangle is what is used)
 *   2. Cholesky S = L L^T by columns j = 0..m-1: d = S[j][j] - L[j][0]^2 - ... - L[j][j-1]^2 (subtracted one after the other);
 *      d <= 0 or non-finite: status 2; L[j][j] = sqrt(d); for i > j: L[i][j] = (S[i][j] - L[i][0] L[j][0] - ... ) / L[j][j]
 *   3. w = L^-1 y by forward substitution (w[i] = (y[i] - L[i][0] w[0] - ...) / L[i][i]); nis = w[0]^2 + ... ; gate > 0 and
 *      nis > gate: status 1
 *   4. row i of K: t = L^-1 PHt[i] forward, K[i] = L^-T t backward (K[i][k] = (t[k] - L[k+1][k] K[i][k+1] - ...) / L[k][k], terms in
 *      ascending row of L); dx[i] = K[i][0] y_0 + ...; x <- x [+] dx (the state's boxplus: so3 blocks R Exp(d), S2 gravity)
 *   5. A[i][c] = (i == c) - (K[i][0] H_0[c] + ...) on the columns of the blocks, (i == c) elsewhere;
 *      AP[i][j] = A[i][0] P[0][j] + ... + A[i][22] P[22][j];  KR[i][l] = K[i][0] R_0l + ...
 *      P[i][j] = (AP[i][0] A[j][0] + ... + AP[i][22] A[j][22]) + (KR[i][0] K[j][0] + ...)        (Joseph form)
 *   6. ... computed for i <= j and stored to [i][j] and [j][i]: the stored P is exactly symmetric.
 * The device contracts a * b + c into fused operations and takes sin / cos / atan from its own few-ulp versions, so it follows
 * this rule to rounding (1e-12 on a single observation, tests/test_gpu_observe.py), not bit for bit.  The reset Jacobian of the
 * SO(3) and S2 blocks after [+] is not applied to P (second order in dx; DESIGN.md "knowing differences").
 * Status 1 and 2 leave x and P exactly as they were; rows = m, y = the full 3-dim innovation, nis = 0 with status 2.
 *
 * lv_observe applies obs[0..n-1] (1 <= n <= LV_OBSERVE_BATCH) one after the other in ONE launch: the second sees the first's
 * posterior.  Queued predictions are launched first, so calls take effect in the order they were made.  out == NULL: enqueue
 * only (the 100 Hz form); out != NULL: waits for the context's stream and writes n results.  lv_observe_results waits and returns
 * the results of the last lv_observe (*n = their number, may be NULL; capacity below it: LV_EINVAL; LV_ESTATE before any).
 * An unknown kind, a mask outside 1..7, a non-finite z, R, lever or gate, gate < 0, a non-zero lever with a kind other than
 * POSITION, an ATTITUDE z with | |z| - 1 | > 1e-6, n outside 1..LV_OBSERVE_BATCH or a NULL obs give LV_EINVAL before anything
 * is enqueued: the filter and the queue are untouched.  LV_ESTATE before lv_filter_set.  Afterwards the filter is on the device
 * (a following lv_correct starts from it, lv_map_add_scan transforms with it, lv_filter_get copies it).
 * With a multi-GPU communicator the filter is replicated and the update deterministic: every rank calls lv_observe with the same
 * observations, as with lv_predict. */
enum { LV_OBS_POSITION = 1, LV_OBS_VELOCITY_WORLD = 2, LV_OBS_VELOCITY_BODY = 3, LV_OBS_ATTITUDE = 4 };
typedef struct lv_observation {
    int    kind;       /* LV_OBS_* */
    int    mask;       /* bits 0..2: which components of the 3-dim innovation are used; 1..7 */
    double z[4];       /* POSITION / VELOCITY_*: z[0..2]; ATTITUDE: unit quaternion x,y,z,w (the state's order) */
    double R[9];       /* 3x3 row-major covariance of the full 3-dim observation; the masked rows/cols are used */
    double lever[3];   /* POSITION only: antenna in the IMU frame; others: must be 0 */
    double gate;       /* > 0: reject when NIS > gate; 0: no gate */
} lv_observation;
typedef struct lv_observe_result { int status; int rows; double nis; double y[3]; } lv_observe_result;
/* status: 0 applied, 1 gated out, 2 S not positive definite (state untouched in 1 and 2) */
#define LV_OBSERVE_BATCH 8
/* kind as given, mask 7, z = 0 (ATTITUDE: the identity quaternion), R = I, lever = 0, gate = 0 */
void lv_default_observation(lv_observation* o, int kind);
int  lv_observe(lv_ctx* ctx, const lv_observation* obs, size_t n, lv_observe_result* out /* NULL: no wait */);
int  lv_observe_results(lv_ctx* ctx, lv_observe_result* out, size_t capacity, size_t* n);  /* of the last lv_observe; waits */

/* Split form of lv_update for multi-GPU runs (scan points sharded across ranks, map replicated):
 *   lv_update_begin(x, P)
 *   repeat MAX_NUM_ITERS+1 times:
 *       lv_pass_reduce()                      -> fills the device record lv_sums_device_ptr()
 *       <all-reduce(sum) LV_SUMS_LEN doubles at lv_sums_device_ptr() across ranks, same stream>
 *       lv_pass_solve()                       -> 23-dof solve, boxplus, convergence bookkeeping
 *   lv_update_end(x, P, passes)
 * All calls are asynchronous on the context stream except lv_update_end. */
int   lv_update_begin(lv_ctx* ctx, const lv_state* x, const double* P);
int   lv_pass_reduce(lv_ctx* ctx);
void* lv_sums_device_ptr(lv_ctx* ctx);
/* Use caller-owned device memory (>= LV_SUMS_LEN doubles, e.g. a torch tensor handed to RCCL) as
 * the sums record; NULL restores the context's own buffer. */
int   lv_set_sums_buffer(lv_ctx* ctx, void* device_ptr);
int   lv_pass_solve(lv_ctx* ctx);
int   lv_update_end(lv_ctx* ctx, lv_state* x, double* P, int* passes);

/* ---- multi-GPU, collective inside the library (SURVEY §8 row e) --------------------------------
 * One process per GPU; the scan is sharded (each rank calls lv_scan_set with its range), the map is
 * replicated.  After lv_comm_init every measurement pass of lv_update / lv_correct all-reduces the
 * 96-double record with RCCL (over xGMI) on the context stream: the whole iterated update is enqueued
 * without a host round trip per pass, and every rank ends with the bitwise identical state.  The reference
 * has no counterpart (single process); this replaces the same esekf call as lv_update.
 *   rccl_library: path of librccl to bind at run time (NULL: "librccl.so.1" from the loader path).  In a
 *                 process that also runs torch pass torch's bundled copy (<torch>/lib/librccl.so) so that
 *                 one RCCL serves both.
 *   lv_comm_unique_id: rank 0 creates the 128-byte id (ncclUniqueId) and hands it to the other ranks by any
 *                 means (torch.distributed broadcast, MPI, a file); lv_comm_init is collective.
 * lv_iterate stays per-rank (its sums describe this rank's points). */
#define LV_COMM_ID_BYTES 128
int lv_comm_unique_id(const char* rccl_library, void* id128);
int lv_comm_init(lv_ctx* ctx, const char* rccl_library, const void* id128, int rank, int world);
int lv_comm_destroy(lv_ctx* ctx);
int lv_comm_world(lv_ctx* ctx);
/* With a communicator lv_update / lv_correct run a pass as search / fit / reduce -> ncclAllReduce -> solve (three kernels
 * and a collective).  If the caller tells the LARGEST shard of the current scan over the ranks — n_max, the same value on
 * every rank, after every lv_scan_set* (which forgets it) — they take the one-launch-per-pass form instead: every rank
 * launches the same grid (sized for n_max), leaves its workgroup partials in its slot of a gather buffer, ncclAllGather
 * (in place, on the context stream) hands every rank all partials, and the next launch's prologue folds them in the same
 * fixed order on every rank: identical states without a broadcast, one launch + one collective per pass.
 * lv_set_comm_fused(ctx, 0) (or LV_COMM_FUSED=0) keeps the three-kernel form. */
int lv_comm_set_shard_max(lv_ctx* ctx, size_t n_max);
int lv_set_comm_fused(lv_ctx* ctx, int enabled);
/* The same one-launch-per-pass multi-rank form with the CALLER's transport instead of librccl (bring-up on fabrics RCCL
 * does not serve, and the two-ranks-on-one-GPU test of exactly the kernels, buffers and fold the RCCL route uses): after
 * every searching launch the library copies this rank's slot of the gather buffer to host memory and calls
 *   fn(user, slots, bytes_per_rank, rank, world)
 * with `slots` = world x bytes_per_rank bytes of host memory holding this rank's partials at slots + rank * bytes_per_rank;
 * fn fills in every other rank's slot (an all-gather by whatever means; it returns 0 when they are all there) and the
 * library copies the whole buffer back.  Tell the largest shard with lv_comm_set_shard_max as above; without it, or for
 * scans the one-launch form does not take, lv_update / lv_correct fail with LV_ESTATE (there is no all-reduce transport
 * here).  fn = NULL removes it.  Not combinable with lv_comm_init. */
typedef int (*lv_gather_fn)(void* user, void* slots, size_t bytes_per_rank, int rank, int world);
int lv_comm_set_host_gather(lv_ctx* ctx, int rank, int world, lv_gather_fn fn, void* user);

/* The same one-launch-per-pass multi-rank form over PEER-MAPPED memory (HIP IPC over xGMI), no collective library: every
 * rank exports the handles of its gather buffers and of its flag word (lv_comm_peer_export: LV_PEER_HANDLE_BYTES = 128 bytes,
 * two HIP IPC handles), the caller carries the blobs of all ranks to every rank by whatever means it has (they are plain
 * bytes), and lv_comm_peer_init maps them.  After each pass one small kernel publishes "my partials of this launch are in
 * memory" and pulls the other ranks' slots straight out of their buffers — a one-shot peer read instead of a ring collective
 * (SURVEY 8e).  Tell the largest shard with lv_comm_set_shard_max as above; ranks end bitwise equal.
 * Failure: a rank that does not publish within the give-up time (LV_PEER_TIMEOUT_MS in the environment, default 2000 ms —
 * far above ordinary host skew between processes) ends the others' wait; the rank that gave up poisons its own flag, so
 * every rank of the node fails the SAME update.  lv_update then returns LV_ESTATE with x and P untouched; the resident
 * filter (lv_correct) is declared unset and every later call fails with LV_ESTATE until lv_comm_destroy + lv_filter_set.
 * At most 8 ranks (one node); HSA_ENABLE_IPC_MODE_LEGACY=0 must be set in the environment of every rank.
 * EXPERIMENTAL and opt-in: verified with two processes on one GPU (shared L2), not yet across GPUs; a second
 * lv_comm_peer_init on the same context returns LV_ESTATE.  Not combinable with lv_comm_init / lv_comm_set_host_gather. */
#define LV_PEER_HANDLE_BYTES 128
int lv_comm_peer_export(lv_ctx* ctx, void* handles /* LV_PEER_HANDLE_BYTES */);
int lv_comm_peer_init(lv_ctx* ctx, int rank, int world, const void* handles /* world x LV_PEER_HANDLE_BYTES, in rank order */);

/* ---- API-parity / debug fetches (results of the most recent CAPTURED pass; original scan order) --
 * lv_iterate always captures; lv_update captures only after lv_set_capture(ctx, 1) (the last pass
 * executed wins).  Capturing writes ~200 B per scan point and is off on the fast path. */
int lv_set_capture(lv_ctx* ctx, int enabled);
/* Nearest_Search outputs: idx N x k (index into the map in insertion order, 0xFFFFFFFF = none),
 * d2 N x k squared distances ascending (+inf = none); k = NUM_MATCH_POINTS. */
int lv_fetch_knn(lv_ctx* ctx, uint32_t* idx, float* d2);
/* The same Nearest_Search outputs as the hand-over records of the most recent pass hold them, whatever build
 * ran it — in particular the NON-capturing kernels of lv_update / lv_correct / lv_pass_reduce (the timed path),
 * which carry no map indices: nbr_xyz N x k x 3 neighbour coordinates (zeros = none), d2 N x k (+inf = none; k = NUM_MATCH_POINTS),
 * p_world N x 3 (the transformed scan point, Mapper.cpp:51), found N.  Original scan order; any pointer may be
 * NULL.  Tests compare these with the oracle's neighbours to pin the fast build (the index-carrying lv_fetch_knn
 * needs a capturing launch). */
int lv_fetch_neighbors(lv_ctx* ctx, float* nbr_xyz, float* d2, float* p_world, int32_t* found);
/* The single-GPU lv_update / lv_correct run ONE launch per pass (pass_kernel: the solve of the previous pass in every
 * workgroup, the search, the plane fits; no capture, degeneracy_mode 0, lanes_per_query 8, up to 16 rounds per workgroup = 1 M scan points on a 256-CU part) and keep the
 * hand-over records in LDS (also with estimate_extrinsics since round 3).  lv_set_record_dump(ctx, 1) makes that same kernel also store them to memory so that
 * lv_fetch_neighbors can pin it (one uniform branch; off by default).  lv_last_update_fused: 1 if the most recent
 * lv_update / lv_correct took the one-launch-per-pass route, 0 if the three-kernel pass (search / fit / solve). */
int lv_set_record_dump(lv_ctx* ctx, int enabled);
int lv_last_update_fused(lv_ctx* ctx);
/* Measurement passes of the most recent lv_update / lv_correct.  lv_correct(ctx, NULL) does not wait for the device: the figure
 * is then valid after the next call that does (lv_filter_get, lv_synchronize) — one host/device round trip per cycle instead
 * of two when the caller fetches the state anyway (Localizator::latest_state after ::correct, src/main.cpp:88-89). */
int lv_last_passes(lv_ctx* ctx);
/* Geometry of the one-launch-per-pass kernel for an n_scan-point scan on a part with n_cus compute units (pure host
 * logic, no GPU needed): out = {searching workgroups, search steps per round (1 or 2), rounds per workgroup,
 * 1 if one more workgroup only keeps the books (a CU is left over) else 0}.  A workgroup searches 4 tiles of 32 points
 * per step; lv_update takes this route up to 16 rounds (1 M points on a 256-CU part), with and without estimate_extrinsics
 * (round 5: its multi-round form stages a fit wavefront's rows in two halves). */
int lv_pass_geometry(size_t n_scan, int n_cus, int out[4]);
/* A/B knob: 0 = always the three-kernel pass (environment LV_FUSED_PASS sets the default at lv_create). */
int lv_set_fused_pass(lv_ctx* ctx, int enabled);
/* Tuning / test knobs by name (the environment variables LV_<NAME> set the defaults at lv_create): "fused_pass",
 * "fused_ext" (one launch per pass also with estimate_extrinsics), "fused_multi_round" (1: ... whatever the rounds per workgroup, 0: up to three — the rule of
 * round 3; default: up to 16), "keeper_by_cost", "tile_lpt", "spin_wait", "comm_fused", "small_window" / "small_insert" (windows /
 * insert batches of up to 2048 points take their one-launch forms), "multi_overlap" (0: multi-round scans fit every round
 * between two barriers), "async_relinearise" / "async_relinearise_min" (the background map rebuild, lv_map_relinearise_async),
 * "async_relinearise_pause_us" (round 6, default 100: behind every slice the worker leaves the chip empty for that many microseconds, so
 * that what the calling cycle launches meanwhile starts at once; 0: slices back to back — the rebuild is ~8 x quicker, the cycles beside
 * it 15 % slower with a p99 of 0.65 instead of 0.55 ms),
 * "async_relinearise_slice_wgs" (the worker's large grids go out in slices of that many workgroups; default 256, 0: whole grids;
 * round 5's opt-in "async_relinearise_paced_*" form was removed in round 6: LV_EINVAL like any unknown name),
 * "async_relinearise_journal_max" (default 4096: the number of map operations that may wait for the worker; a rebuild that falls
 * further behind is cancelled, the map stays as it is, and this context re-linearises stop-the-world from then on).
 * None of those changes a result beyond the summation order of the workgroup partials.  ONE option does: "fast_fit" (default
 * 0) switches pass_kernel's plane fit to hardware reciprocal / square root + one Newton step — within a few f32 ulps of the
 * exact path, NOT bit-exact against the reference (tests/test_gpu_fast_fit.py states the flips and the state difference);
 * it exists for the default 6-column configuration only and is ignored elsewhere.  LV_EINVAL for an unknown name. */
int lv_set_option(lv_ctx* ctx, const char* name, int value);
/* instrumentation (contexts created with LV_PASS_CLK=1 in the environment): for every launch of the last update
 * (MAX_NUM_ITERS + 2 of them) and every workgroup slot (capacity_wg >= CUs + 1 of them per launch; slot *n_wg is the
 * launch's designated workgroup), 16 shader-clock stamps followed by 16 wall-clock stamps (100 MHz) at its phase
 * boundaries: out holds (MAX_NUM_ITERS + 2) x capacity_wg... see scripts/pass_clocks.py for the layout. */
int lv_get_pass_clocks(lv_ctx* ctx, long long* out, int capacity_wg, int* n_wg);   /* out = NULL: *n_wg = slots per launch */
/* Mapper::match outputs: valid N (Match::is_chosen), p_world N x 3, abcd N x 4 (Normal A,B,C,D),
 * dist N (Match::distance).  Any pointer may be NULL. */
int lv_fetch_matches(lv_ctx* ctx, uint8_t* valid, float* p_world, float* abcd, float* dist);
/* calculate_H outputs as N x 12 rows / N residuals with zero rows for rejected points. */
int lv_fetch_rows(lv_ctx* ctx, double* H, double* h);

/* Localizator::calculate_H(const state_ikfom&, const Matches&, MatrixXd& H, VectorXd& h)
 *                                                 — src/Modules/Localizator.cpp:29-57
 * for caller-supplied matches: p_world n x 3 (Match::point), abcd n x 4 (Match::plane.n), dist n
 * (Match::distance).  H receives n x 12 row-major rows, h receives n residuals.  Synchronous. */
int lv_calculate_H(lv_ctx* ctx, const lv_state* x, const float* p_world, const float* abcd, const float* dist, size_t n,
                   double* H, double* h);

/* ---- Pose graph --------------------------------------------------------------------------------------
 * A pose-graph optimiser on the device: it spreads loop closures and GPS fixes back over a trajectory.  Independent of the map
 * and of the volumes; everything in f64; bitwise reproducible from call to call (no float atomics, fixed summation orders).
 * The rule is the __host__ __device__ code of limo-velo_amd/csrc/lv_graph.hpp; tests/graph_ref.py restates it in numpy.
 *
 *   node      (t, q): position and unit quaternion x, y, z, w as in lv_state, R = R(q).  An increment d = (dt, dth) acts as
 *             t <- t + dt, R <- R Exp(dth) (q <- q * exp(dth / 2), then renormalised): position additive, rotation on the right,
 *             the filter's convention.  A fixed node takes no increment.
 *   edge      (i, j, tz, qz, info, huber): r = [ Ri^T (tj - ti) - tz ; Log(Rz^T Ri^T Rj) ].  With dv = Ri^T (tj - ti) and
 *             J = Jr^-1(r_th): dr_t/dt_i = -Ri^T, dr_t/dth_i = [dv]x, dr_t/dt_j = Ri^T, dr_th/dth_j = J, dr_th/dth_i = -J Rj^T Ri,
 *             every other block zero.  Jr^-1(p) = I + [p]x / 2 + c [p]x^2, c = 1 / th^2 - (1 + cos th) / (2 th sin th), and
 *             c = 1 / 12 + th^2 / 720 below th = 1e-4 (th = |p|).  Log takes the quaternion with w >= 0: |r_th| <= pi.
 *   prior     (i, tp, qp, lever, info, huber): r = [ ti + Ri lever - tp ; Log(Rp^T Ri) ]; dr_t/dt_i = I,
 *             dr_t/dth_i = -Ri [lever]x, dr_th/dth_i = Jr^-1(r_th).  A GPS fix is a prior whose rotation rows and columns of info
 *             are zero.
 *   info      a symmetric 6 x 6 matrix given as the 21 entries of its upper triangle, row by row (00 01 .. 05 11 12 .. 55), rows
 *             and columns ordered (t, th).  It may be positive semi-definite.
 *   cost      s = r^T info r per factor; cost = 1/2 sum rho(s), rho = s without Huber (huber = 0), else rho = s for
 *             sqrt(s) <= huber and 2 huber sqrt(s) - huber^2 beyond.  Weight w = 1 or huber / sqrt(s).  The Gauss-Newton blocks are
 *             J^T (w info) J, the gradient J^T (w info) r; there is no second-order term.
 *   loop      Levenberg-Marquardt on (H + lambda diag H) d = -g, lambda starting at lambda_init.  The system is solved by
 *             conjugate gradients from d = 0, preconditioned by the inverses of the 6 x 6 diagonal blocks of H + lambda diag H
 *             (a Cholesky in the order k = 0..5, column by column; a pivot that is not positive gives that component a zero row
 *             and column: it does not move).  The solve stops after the iteration at which r^T z <= pcg_tol^2 (r^T z)_0, at
 *             pcg_max_iterations, or when p^T A p is not positive.  The trial poses are x + d.  A step is ACCEPTED when
 *             cost_new <= cost_old + 64 eps |cost_old| (eps = 2^-52; the slack lets the loop pass the cost's rounding floor); then
 *             lambda <- max(lambda / 3, lambda_min), otherwise the poses stay and lambda <- min(4 lambda, lambda_max).  The
 *             status is LV_GRAPH_CONVERGED when an accepted step has max-norm (over all 6 n components) <= step_tol, the loop
 *             ends there; otherwise it ends after max_iterations iterations (accepted + rejected) with LV_GRAPH_MAX_ITERATIONS.
 *   sums      a node's diagonal block and gradient are summed over its incidence list (its edges by ascending edge id, then its
 *             priors by ascending id) in list order; a list longer than 64 entries is split over the 64 lanes of a wavefront
 *             (lane l takes entries l, l + 64, ... in order) and folded by a fixed tree.  The cost and the dot products are
 *             workgroup partials (fixed tree) summed in workgroup order by a fixed tree.  Nothing depends on arrival order.
 *   limits    n <= 2^20 nodes, n_edges <= 2^22, n_priors <= 2^20.  lv_graph_set gives LV_EINVAL, naming the record and the
 *             field, for: an index out of range; i == j; a non-finite number; a quaternion whose norm is off 1 by more than 1e-6;
 *             a negative diagonal entry of info; a negative huber; a graph with neither a fixed node nor a prior.  The records
 *             are judged before the context ("null context" comes last), and a rejected call writes nothing: the graph held before
 *             stays bit for bit.  lv_graph_optimise gives LV_EINVAL for parameters outside: max_iterations 1..10000,
 *             pcg_max_iterations 1..100000, 0 < pcg_tol < 1, step_tol >= 0, 0 < lambda_min <= lambda_init <= lambda_max, all finite.
 * Every call below except lv_default_graph_params gives LV_ESTATE before lv_graph_set (and after lv_graph_clear); lv_graph_get_info
 * reports set = 0 instead.  lv_graph_set keeps the given poses as x0 and as the current poses; lv_graph_optimise moves the current
 * poses and may be called again (it continues from them).  The calls run on the context's stream and return when their outputs
 * are written.  lv_destroy releases the store. */
#define LV_GRAPH_CONVERGED 0
#define LV_GRAPH_MAX_ITERATIONS 1
#define LV_GRAPH_MAX_NODES (1u << 20)
#define LV_GRAPH_MAX_EDGES (1u << 22)
#define LV_GRAPH_MAX_PRIORS (1u << 20)
typedef struct lv_graph_pose {   /* 56 bytes */
    double t[3];
    double q[4];                 /* x, y, z, w */
} lv_graph_pose;
typedef struct lv_graph_edge {   /* 240 bytes */
    uint32_t i, j;
    double   t[3];               /* tz */
    double   q[4];               /* qz */
    double   info[21];
    double   huber;              /* 0: no Huber */
} lv_graph_edge;
typedef struct lv_graph_prior {  /* 264 bytes */
    uint32_t i;
    uint32_t reserved;           /* must be 0 */
    double   t[3];               /* tp */
    double   q[4];               /* qp */
    double   lever[3];
    double   info[21];
    double   huber;
} lv_graph_prior;
typedef struct lv_graph_params {
    int32_t max_iterations;      /* 100 */
    int32_t pcg_max_iterations;  /* 1000 */
    double  pcg_tol;             /* 1e-2 */
    double  step_tol;            /* 1e-8 */
    double  lambda_init;         /* 1e-4 */
    double  lambda_min;          /* 1e-10 */
    double  lambda_max;          /* 1e8 */
} lv_graph_params;
typedef struct lv_graph_info {
    int32_t  set;                /* a graph is held */
    int32_t  status;             /* of the last lv_graph_optimise: LV_GRAPH_CONVERGED or LV_GRAPH_MAX_ITERATIONS; -1 before one */
    uint32_t n, n_edges, n_priors, n_fixed;
    uint32_t longest_list;       /* entries of the longest incidence list */
    uint32_t accepted, rejected; /* iterations of the last optimise */
    uint32_t pcg_iterations;     /* conjugate-gradient iterations of the last optimise, in total */
    double   initial_cost, final_cost;
    double   last_step;          /* max-norm of the last accepted step (0 when none was) */
    double   lambda;             /* after the last iteration */
} lv_graph_info;
void lv_default_graph_params(lv_graph_params* p);
/* Copies the graph to the device and builds its incidence lists.  fixed: n bytes, nonzero = fixed, or NULL (none fixed).  edges /
 * priors may be NULL when their count is 0.  Replaces the graph held before. */
int lv_graph_set(lv_ctx* ctx, const lv_graph_pose* poses, size_t n, const uint8_t* fixed, const lv_graph_edge* edges, size_t n_edges,
                 const lv_graph_prior* priors, size_t n_priors);
/* Runs the loop above from the current poses.  params NULL: the defaults.  info may be NULL. */
int lv_graph_optimise(lv_ctx* ctx, const lv_graph_params* params, lv_graph_info* info);
/* The current poses; capacity < n: LV_EINVAL. */
int lv_graph_fetch(lv_ctx* ctx, lv_graph_pose* poses, size_t capacity);
/* s = r^T info r of every edge (n_edges values) and prior (n_priors values) at the current poses, unweighted: a caller vets loop
 * closures with it.  Either pointer may be NULL. */
int lv_graph_chi2(lv_ctx* ctx, double* edge_s, double* prior_s);
/* out[k] = T_now[key] T_x0[key]^-1 p[k]: n points (x, y, z as f32 at the start of every `stride` bytes, stride >= 12) moved by the
 * correction of their key's node, computed in f64 and rounded once to f32; out: 3 n floats.  D = (R_now R_0^T, t_now - D_R t_0) is
 * formed once per key (a node whose pose equals its x0 bit for bit gives the identity exactly) and row sums run left to right:
 * out = ((D0 x + D1 y) + D2 z) + Dt per row.  A key >= the node count: LV_EINVAL, nothing written.  n <= 2^28. */
int lv_graph_warp_points(lv_ctx* ctx, const void* pts, size_t stride, const uint32_t* keys, size_t n, float* out);
int lv_graph_get_info(lv_ctx* ctx, lv_graph_info* info);
/* Forgets the graph (the buffers stay for the next one). */
int lv_graph_clear(lv_ctx* ctx);

/* ---- Trajectory --------------------------------------------------------------------------------------
 * A trajectory on the device for offline mapping: stamped poses (knots) that answer "where was the sensor at time t" for every
 * point of a recording, that can be smoothed, that take the pose graph's corrections spread over time, and against which a whole
 * recording's raw, time-stamped points are registered again in one pass.  Independent of the map, the volumes and the filter;
 * everything in f64; times are f64 seconds and nothing narrows them (only differences of times enter the arithmetic); bitwise
 * reproducible from call to call (no float atomics, fixed summation orders).  The rule is the __host__ __device__ code of
 * limo-velo_amd/csrc/lv_traj.hpp on the quaternion algebra of lv_graph.hpp; tests/traj_ref.py restates it in numpy.
 *
 *   knot      (time, t, q): position and unit quaternion x, y, z, w as in lv_graph_pose; times strictly ascending.
 *   sample    for time_a <= t < time_b of neighbouring knots: u = (t - time_a) / (time_b - time_a), p = p_a + u (p_b - p_a),
 *             q = q_a * Exp(u Log(q_a^-1 q_b)), renormalised (q / sqrt(((x^2 + y^2) + z^2) + w^2)).  Log takes the quaternion with
 *             w >= 0, the short way round, so a knot stored as -q gives the same rotation.  A time equal to a knot's time gives that
 *             knot's pose bit for bit, the last knot's included; one knot alone is a constant.  p_b - p_a and Log(q_a^-1 q_b) are
 *             formed once per knot.  Status: LV_TRAJ_INSIDE, LV_TRAJ_BEFORE (t below the first knot), LV_TRAJ_AFTER (above the
 *             last), LV_TRAJ_NONFINITE.  Outside, LV_TRAJ_CLAMP gives the first / last knot's pose and LV_TRAJ_REFUSE gives NaN;
 *             the status says which side under both.  A non-finite time gives NaN under both.
 *   smooth    a kernel smoother, Jacobi style (every knot reads the values of the iteration before).  The window of knot i is
 *             j in [max(0, i - half_window), min(n - 1, i + half_window)], w_j = exp(-0.5 ((time_j - time_i) / sigma)^2), the sums
 *             run in ascending j, W = sum w_j; p_i <- p_i + (sum w_j (p_j - p_i)) / W and q_i <- q_i * Exp((sum w_j Log(q_i^-1 q_j)) / W),
 *             renormalised: one step towards the weighted Karcher mean.  A knot with fixed[i] != 0 keeps its bits, and so do the
 *             two ends under pin_ends.  iterations = 0 changes nothing.  THIS IS A SIGNAL SMOOTHER, NOT A STATISTICAL ONE: the store
 *             holds no covariances, and weighing measurements against one another across loops remains lv_graph_*'s job.
 *   correct   corr is itself a small trajectory whose poses are corrections D_k = T_now T_0^-1 at keyframe times.  Every knot i
 *             becomes D(time_i) o knot_i with D(t) = corr sampled by the sample rule, clamped outside: t' = D_R t + D_t (row sums
 *             left to right, then + D_t), q' = D_q * q renormalised.  A sampled correction that is the identity bit for bit
 *             (q = (0, 0, 0, 1), t = 0) leaves the knot bit for bit (as lv_graph_warp_points promises).  Times are untouched.
 *   register  a point p (x, y, z f32, its own f64 time t): b = E_R p + E_t with the extrinsic E (LiDAR in body), w = R(q(t)) b + p(t)
 *             with the sampled pose, and with frame = LV_TRAJ_FRAME_AT: w = F_R w + F_t, F = (T(frame_time) E)^-1 formed once per
 *             call: the continuous-time de-skew into the LiDAR frame at frame_time.  All in f64, every row ((a x + b y) + c z) + d,
 *             rounded once to f32.  A point with a non-finite coordinate or time gives NaN and LV_TRAJ_NONFINITE; a point outside
 *             the trajectory follows `extrapolate`.
 *   routes    a workgroup takes 256 consecutive points, finds the knot range that brackets their finite times, and when the range
 *             holds at most 256 knots stages it in LDS (the tile route); otherwise every lane searches the whole time array (the
 *             search route).  Both run the same function on the same knots and give the same bits; stats[2] / stats[3] count the
 *             workgroups of either.  lv_set_option("traj_tile", 0) forces the search route (tests, timing); default 1.
 *   limits    1 <= n <= 2^20 knots; sample and register calls take up to 2^28 items.  lv_traj_set and lv_traj_correct give
 *             LV_EINVAL, naming the record and the field, for a non-finite number, a quaternion whose norm is off 1 by more than
 *             1e-6 and times that are not strictly ascending.  lv_traj_smooth: sigma > 0, half_window 1..64, iterations 0..100.
 *             lv_traj_register: time_offset >= 12, time_offset + 8 <= stride (offsets need not be aligned), the extrinsic finite
 *             and of unit norm, frame_time finite and on the trajectory.  Arguments are judged before the context ("null context"
 *             comes last; frame_time against the trajectory needs the store and comes after it), and a rejected call writes
 *             nothing: the trajectory held before stays bit for bit.
 * Before lv_traj_set and after lv_traj_clear every call below except the two defaults gives LV_ESTATE; lv_traj_get_info reports
 * set = 0 instead.  The calls run on the context's stream and return when their outputs are written.  With host arrays a register
 * call is bound by its transfers, not by the kernel (DESIGN.md "Trajectory"); lv_traj_register_cloud is the route without the
 * upload.  lv_destroy releases the store. */
#define LV_TRAJ_MAX_KNOTS (1u << 20)
#define LV_TRAJ_INSIDE 0
#define LV_TRAJ_BEFORE 1
#define LV_TRAJ_AFTER 2
#define LV_TRAJ_NONFINITE 3
#define LV_TRAJ_CLAMP 0
#define LV_TRAJ_REFUSE 1
#define LV_TRAJ_WORLD 0
#define LV_TRAJ_FRAME_AT 1
typedef struct lv_traj_knot {    /* 64 bytes */
    double time;                 /* seconds */
    double t[3];
    double q[4];                 /* x, y, z, w */
} lv_traj_knot;
typedef struct lv_traj_smooth_params {   /* 24 bytes */
    double  sigma;               /* seconds, > 0 (0.1) */
    int32_t half_window;         /* knots each side, 1..64 (8) */
    int32_t iterations;          /* 0..100 (1) */
    int32_t pin_ends;            /* the first and the last knot keep their bits (1) */
} lv_traj_smooth_params;
typedef struct lv_traj_register_params {   /* 72 bytes */
    int32_t extrapolate;         /* LV_TRAJ_CLAMP (default) or LV_TRAJ_REFUSE */
    int32_t frame;               /* LV_TRAJ_WORLD (default) or LV_TRAJ_FRAME_AT */
    double  ext_t[3];            /* E: LiDAR in body (offset_T_L_I); default 0 */
    double  ext_q[4];            /* (offset_R_L_I as a quaternion); default 0, 0, 0, 1 */
    double  frame_time;          /* with LV_TRAJ_FRAME_AT */
} lv_traj_register_params;
typedef struct lv_traj_info {    /* 64 bytes */
    int32_t  set;                /* a trajectory is held */
    uint32_t n;
    double   t_first, t_last;
    uint32_t smooth_iterations;  /* smoothing iterations applied since lv_traj_set */
    uint32_t corrections;        /* lv_traj_correct calls applied since lv_traj_set */
    uint64_t last_register[4];   /* the stats of the last register call */
} lv_traj_info;
void lv_default_traj_smooth_params(lv_traj_smooth_params* p);
void lv_default_traj_register_params(lv_traj_register_params* p);
/* Copies n knots to the device and forms their interval records.  Replaces the trajectory held before. */
int lv_traj_set(lv_ctx* ctx, const lv_traj_knot* knots, size_t n);
/* The current knots; capacity < n: LV_EINVAL. */
int lv_traj_fetch(lv_ctx* ctx, lv_traj_knot* knots, size_t capacity);
int lv_traj_get_info(lv_ctx* ctx, lv_traj_info* info);
/* Forgets the trajectory (the buffers stay for the next one). */
int lv_traj_clear(lv_ctx* ctx);
/* The sample rule for n times: out n poses, status n bytes; either may be NULL. */
int lv_traj_sample(lv_ctx* ctx, const double* times, size_t n, int extrapolate, lv_graph_pose* out, uint8_t* status);
/* The smoother above; fixed: one byte per knot or NULL. */
int lv_traj_smooth(lv_ctx* ctx, const lv_traj_smooth_params* params, const uint8_t* fixed);
/* Applies the corrections corr (m >= 1 records, judged as lv_traj_set judges its knots) to every knot. */
int lv_traj_correct(lv_ctx* ctx, const lv_traj_knot* corr, size_t m);
/* Registers n points: records of `stride` bytes with x, y, z f32 at 0 and an f64 time at time_offset (16 in the reference's 32-byte
 * Point).  params NULL: the defaults.  out: 3 n floats, status: n bytes; either may be NULL (to count only).  stats (may be NULL):
 * points inside, points outside (before + after + non-finite), workgroups of the tile route, workgroups of the search route.
 * n = 0: LV_OK, nothing written but stats. */
int lv_traj_register(lv_ctx* ctx, const lv_traj_register_params* params, const void* pts, size_t stride, size_t time_offset, size_t n,
                     float* out, uint8_t* status, uint64_t stats[4]);
/* The same kernel on the device LiDAR buffer: the points with t1 <= time <= t2, oldest first, exactly what lv_cloud_fetch(t1, t2)
 * returns and in its order.  The raw points do not leave the device and nothing in the buffer changes.  *n: the points of the
 * window.  out == NULL: only *n is set (to size out: 3 *n floats; status: *n bytes, may be NULL); capacity < *n points: LV_EINVAL. */
int lv_traj_register_cloud(lv_ctx* ctx, const lv_traj_register_params* params, double t1, double t2, float* out, uint8_t* status,
                           size_t capacity, size_t* n, uint64_t stats[4]);

/* ---- NDT registration --------------------------------------------------------------------------------
 * Cloud-to-cloud registration by the normal-distributions transform: a TARGET cloud becomes a voxel grid of Gaussians built
 * once, and a SOURCE cloud is aligned to it from K initial guesses at a time (what PCL's NormalDistributionsTransform::align,
 * ndt_omp and fast_gicp's NDTCuda do for one guess).  Independent of the filter, the scan and the volumes; the target may be
 * built from the living points of the device map.  The rule is the __host__ __device__ code of limo-velo_amd/csrc/lv_ndt.hpp;
 * tests/ndt_ref.py restates it in numpy.  The moments are integer sums, so the target is the same bit for bit whatever the order
 * of its points; the alignment is f64 with every sum in one order and repeats its own bits from call to call.
 *
 *   grid      origin[3], resolution (finite, > 0), nx, ny, nz each 1..1024 with nx * ny * nz <= 2^22; voxel (i, j, k) has index
 *             (k * ny + j) * nx + i.  min_points 2..2^20, reg finite in 0..1.
 *   point     per axis q_a = floorf(((p_a - origin_a) / resolution) * 256) in f32, the occupancy grid's quantisation.  A point
 *             with a non-finite or out-of-range q (|q| >= 2^24), or whose voxel c_a = q_a >> 8 lies outside the grid, is IGNORED.
 *             Otherwise it is USED in voxel c with the local coordinate r_a = q_a & 255.
 *   moments   per voxel n (uint32), S1[3] = sum r_a (int64), S2[6] = sum r_a r_b over the upper triangle in the order
 *             00 01 02 11 12 22 (int64).  Integer atomics: the sums commute.  The points given to a target (build plus adds, USED
 *             or not) number at most 2^31 - 1, so nothing overflows.
 *   Gaussian  of a voxel with n >= min_points (a USED voxel), in f64, u = (double)resolution / 256:
 *               m_a   = ((double)S1_a + 0.5 n) / n                                       (the centre of a sub-unit)
 *               mu_a  = ((double)origin_a + (double)resolution * c_a) + u * m_a
 *               C_ab  = (u^2 * ((double)S2_ab - ((double)S1_a * (double)S1_b) / n)) / (n - 1)
 *               Sigma = C + ((reg * ((C_00 + C_11) + C_22)) / 3 + u^2 / 12) I
 *             u^2 / 12 is the variance of the quantisation: Sigma is positive definite even for coincident points.  The term in
 *             reg bounds the condition number by 3 / reg + 1 without an eigenvector basis; this differs knowingly from PCL, which
 *             clamps the small eigenvalues to a fraction of the largest.  Omega = Sigma^-1 by a 3 x 3 Cholesky, column by
 *             column.  A voxel that is not USED stores zeros in MEAN, COV and ICOV.
 *   term      for source point p and pose (t, q), R = R(q): x = R p + t in f64, each row ((R_k0 p_0 + R_k1 p_1) + R_k2 p_2) + t_k.
 *             The voxel of x is that of x rounded once to f32, by the rule of `point`.  search = 1 takes that voxel; search = 7
 *             takes it and its six face neighbours in the order 0, +x, -x, +y, -y, +z, -z (ndt_omp's DIRECT1 / DIRECT7).  A voxel
 *             outside the grid or not USED contributes nothing.  For each remaining voxel, in that order:
 *               e = x - mu,  Oe = Omega e,  s = e^T Oe,  w = exp((-0.5 d2) s)
 *               M <- M + w Omega,  b <- b + w Oe,  sw <- sw + w          (M, b, sw start from 0 for every point)
 *             A point with at least one such voxel counts in n_in and adds, with A = -R [p]x and J = [ I , A ] (3 x 6):
 *               S <- S + sw,  g <- g + J^T b,  H <- H + J^T M J   (the 21 entries of the upper triangle)
 *   sums      S, g, H per hypothesis: a workgroup of 256 lanes takes LV_NDT_CHUNK consecutive source points, lane l the points
 *             l, l + 256, ... of the chunk in ascending order; the wavefronts fold by an xor-butterfly, the four of them add in
 *             order, and the workgroups' partials are added in chunk order.  No float atomics; nothing depends on arrival order.
 *   loop      each hypothesis on its own, Levenberg-Marquardt as lv_graph_optimise words it: (H + lambda diag H) d = -g by the
 *             6 x 6 Cholesky of the pose graph's block inverse (a pivot that is not positive freezes that component), trial pose
 *             t + dt, q * exp(dth / 2) renormalised.  A step is ACCEPTED when S_new >= S_old - 64 eps |S_old| (eps = 2^-52) and
 *             d is finite; then lambda <- max(lambda / 3, lambda_min) and the trial's S, g, H, n_in become the current ones (one
 *             evaluation per iteration); otherwise the pose stays and lambda <- min(4 lambda, lambda_max).
 *   status    LV_NDT_NO_OVERLAP when n_in = 0 at the guess: the guess is returned bit for bit, score 0.  LV_NDT_CONVERGED when
 *             an accepted step has max-norm <= step_tol; LV_NDT_MAX_ITERATIONS after max_iterations iterations (accepted +
 *             rejected; 0 only scores the guesses).
 *   best      best[0] is the hypothesis with the greatest score, the smaller index winning a tie, among those that are not
 *             NO_OVERLAP; best[1] its n_in.  -1, -1 with none.
 *   limits    n < 2^31 points per build or add; K <= 4096 guesses, n_src <= 2^20, K * n_src <= 2^30; d2 finite and > 0,
 *             search 1 or 7, max_iterations 0..1000, step_tol finite and >= 0, 0 < lambda_min <= lambda_init <= lambda_max < inf;
 *             a guess must be finite with a quaternion whose norm is within 1e-6 of 1.
 * Parameters and NULL or short arguments are judged before the context (LV_EINVAL, nothing written, "null context" last).
 * lv_ndt_add, lv_ndt_fetch and lv_ndt_align give LV_ESTATE before a build (and after lv_ndt_clear); lv_ndt_info reports built = 0
 * instead.  Nothing is allocated before the first build.  The target is a snapshot of its source; a refused call leaves it in
 * place bit for bit.  No call changes a bit of the map, the filter, the scan or any other store.  The calls run on the context's
 * stream and return when their outputs are written; lv_destroy releases the store. */
#define LV_NDT_CONVERGED 0
#define LV_NDT_MAX_ITERATIONS 1
#define LV_NDT_NO_OVERLAP 2
#define LV_NDT_CHUNK 512          /* source points per workgroup of the evaluation */
#define LV_NDT_MAX_DIM 1024
#define LV_NDT_MAX_VOXELS (1u << 22)
#define LV_NDT_MAX_GUESSES 4096
#define LV_NDT_MAX_SOURCE (1u << 20)
#define LV_NDT_COUNT 0   /* uint32 */
#define LV_NDT_S1    1   /* int64 x 3 */
#define LV_NDT_S2    2   /* int64 x 6 */
#define LV_NDT_MEAN  3   /* double x 3 */
#define LV_NDT_COV   4   /* double x 6: Sigma, upper triangle */
#define LV_NDT_ICOV  5   /* double x 6: Omega, upper triangle */
typedef struct lv_ndt_params {   /* 40 bytes */
    float   origin[3];
    float   resolution;          /* 1.0 */
    int32_t nx, ny, nz;          /* 128, 128, 16 over origin -64, -64, -8 */
    int32_t min_points;          /* 5 */
    double  reg;                 /* 0.01 */
} lv_ndt_params;
typedef struct lv_ndt_align_params {   /* 48 bytes */
    int32_t search;              /* 7 */
    int32_t max_iterations;      /* 100 */
    double  d2;                  /* 0.43312300470355464:Magnusson's value for 1 m voxels and an outlier ratio of 0.55 */
    double  step_tol;            /* 1e-6 */
    double  lambda_init;         /* 1e-4 */
    double  lambda_min;          /* 1e-10 */
    double  lambda_max;          /* 1e8 */
} lv_ndt_align_params;
typedef struct lv_ndt_result {   /* 264 bytes */
    lv_graph_pose pose;
    double   score;              /* S at the pose */
    double   info[21];           /* the upper triangle of H at the pose, laid out as lv_graph_edge.info */
    double   last_step;          /* max-norm of the last accepted step (0 when none was) */
    double   lambda;             /* after the last iteration */
    uint32_t n_in;               /* source points with at least one voxel at the pose */
    int32_t  status;             /* LV_NDT_CONVERGED, LV_NDT_MAX_ITERATIONS or LV_NDT_NO_OVERLAP */
    uint32_t accepted, rejected;
} lv_ndt_result;
typedef struct lv_ndt_target_info {   /* 80 bytes */
    int32_t  built;
    int32_t  from_map;           /* the last build or add read the device map */
    uint64_t n_used, n_ignored;  /* points of the build and of every add since */
    uint64_t used_voxels;        /* n >= min_points */
    uint64_t sparse_voxels;      /* 0 < n < min_points */
    lv_ndt_params params;
} lv_ndt_target_info;
void lv_default_ndt_params(lv_ndt_params* p);
void lv_default_ndt_align_params(lv_ndt_align_params* p);
/* Replaces the target by the Gaussians of n points (x, y, z as f32 at the start of every `stride` bytes, stride >= 12); pts = NULL
 * takes the living points of the device map, as lv_elev_build reads them (stride and n are then not used).  stats (may be NULL):
 * points used, points ignored, used voxels, occupied voxels below min_points. */
int lv_ndt_build(lv_ctx* ctx, const lv_ndt_params* p, const void* pts, size_t stride, size_t n, uint64_t stats[4]);
/* Accumulates further points into the moments of the target and recomputes its Gaussians: build(a) then add(b) is build(a u b)
 * bit for bit.  stats: the points of this call, the voxels of the whole target. */
int lv_ndt_add(lv_ctx* ctx, const void* pts, size_t stride, size_t n, uint64_t stats[4]);
/* A layer, by voxel: capacity counts voxels (nx * ny * nz needed). */
int lv_ndt_fetch(lv_ctx* ctx, int layer, void* out, size_t capacity);
/* Aligns n_src source points from K guesses.  params NULL: the defaults.  results: K records (may be NULL when K = 0); best: 2
 * values.  K = 0 succeeds and writes best only. */
int lv_ndt_align(lv_ctx* ctx, const lv_ndt_align_params* params, const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses,
                 size_t K, lv_ndt_result* results, int32_t best[2]);
int lv_ndt_info(lv_ctx* ctx, lv_ndt_target_info* out);
/* Forgets the target and frees its memory. */
int lv_ndt_clear(lv_ctx* ctx);

/* ---- Surface registration ------------------------------------------------------------------------------
 * The pose of a sensor against the TSDF surface: the other half of KinectFusion, of SDF-Tracker (Bylow et al. 2013), of voxblox's
 * ICP refinement and of voxgraph's submap registration (the reference has no counterpart).  A depth frame is tracked against the
 * volume it fills, a scan is re-localised in a saved volume, the synthetic scans of "Surface ray casting" find their consumer.
 * lv_surf_sample gives the interpolated distance and its gradient at world points; lv_surf_align minimises the distances of a
 * source cloud from K initial guesses at a time, shaped as lv_ndt_align is.  (The section stands here, not behind "Surface ray
 * casting", because its records hold an lv_graph_pose.)  The rule is the __host__ __device__ code of
 * limo-velo_amd/csrc/lv_surf_align.hpp; tests/surf_align_ref.py restates it in numpy.  f64 throughout, every sum in one order:
 * a call repeats its own bits, and a hypothesis gives the same bits alone as in a batch.
 *
 *   sample    of a world point x (f64), with o_a = (double)origin_a at the volume's present origin (after its shifts),
 *             r = (double)resolution and n_a the grid size: u_a = (x_a - o_a) / r - 0.5; a u_a that is not finite or has
 *             |u_a| >= 2^24 makes the point OUTSIDE.  i_a = floor(u_a), f_a = u_a - i_a; the point is OUTSIDE unless 0 <= i_a and
 *             i_a + 1 <= n_a - 1 on every axis.  The corners are the voxels (i_x + a, i_y + b, i_z + c), a, b, c in {0, 1}; the
 *             point is UNKNOWN unless every corner has W >= min_weight, otherwise KNOWN with phi_abc = (double)S / (double)W.
 *               along x:  c_bc = phi_0bc + f_x * (phi_1bc - phi_0bc),   e_bc = phi_1bc - phi_0bc
 *               along y:  c_c = c_0c + f_y * (c_1c - c_0c),   ex_c = e_0c + f_y * (e_1c - e_0c),   ey_c = c_1c - c_0c
 *               along z:  v = c_0 + f_z * (c_1 - c_0),   gx = ex_0 + f_z * (ex_1 - ex_0),   gy = ey_0 + f_z * (ey_1 - ey_0),
 *                         gz = c_1 - c_0
 *             d = (r / 256) * v in metres; n = (gx, gy, gz) / 256, dimensionless: the exact gradient of the interpolant, not
 *             normalised, zero where the field is clamped flat.  Only + - * / and floor occur.
 *   term      for source point p (f32) at the pose (t, q), R = R(q): x = R p + t in f64, the rows summed as in "NDT
 *             registration".  The point is IN iff sample(x) is KNOWN and |d| <= max_dist.  With a = |d| and the Huber width h:
 *             h = 0 or a <= h gives w = 1, rho = 0.5 * d * d; otherwise w = h / a, rho = h * (a - 0.5 * h).  A = -R [p]x,
 *             J = [ n^T , n^T A ] (1 x 6, (n^T A)_c = (n_0 A_0c + n_1 A_1c) + n_2 A_2c).  An IN point adds
 *               H_ab <- H_ab + (w J_a) J_b  (the 21 entries of the upper triangle, a <= b, in the order of lv_ndt_result.info),
 *               g_a <- g_a + (w d) J_a,   E <- E + rho,   and 1 to n_in.
 *   cost      E + (double)(n_src - n_in) * rho(max_dist): every source point that is not IN pays what a point at the gate pays, so
 *             the costs of different poses are comparable and a step cannot win by pushing points out of the band.
 *   sums      exactly those of "NDT registration": workgroups of 256 lanes take LV_SURF_ALIGN_CHUNK consecutive source points, lane l
 *             the points l and l + 256 of its chunk in ascending order; an xor-butterfly per wavefront, the four wavefronts added
 *             in order, the chunk partials added in chunk order; 28 accumulators and the count.  No float atomics.
 *   loop      each hypothesis on its own: (H + lambda diag H) delta = -g by the pose graph's 6 x 6 Cholesky (a pivot that is not
 *             positive freezes that component: a scan on one plane does not diverge), trial pose t + dt, q * exp(dth / 2)
 *             renormalised.  ACCEPTED iff delta is finite, the trial's n_in >= min_points and
 *             cost_new <= cost_old + 64 eps |cost_old| (eps = 2^-52); then lambda <- max(lambda / 3, lambda_min) and the trial's
 *             sums become the current ones (one evaluation per iteration); otherwise lambda <- min(4 lambda, lambda_max).
 *   status    LV_SURF_ALIGN_NO_OVERLAP when n_in < min_points at the guess: the guess is returned bit for bit, cost and info
 *             zero.  LV_SURF_ALIGN_CONVERGED when an accepted step has max-norm <= step_tol; LV_SURF_ALIGN_MAX_ITERATIONS after
 *             max_iterations turns (accepted + rejected; 0 only scores the guesses).
 *   best      best[0] is the hypothesis of least cost among those that are not NO_OVERLAP, the smaller index winning a tie;
 *             best[1] its n_in.  -1, -1 with none.
 *   limits    as lv_ndt_align's: K <= 4096, n_src <= 2^20, K * n_src <= 2^30; a guess finite with a quaternion whose norm is
 *             within 1e-6 of 1.  min_weight >= 1, max_iterations 0..1000, min_points >= 1, max_dist finite and > 0, huber and
 *             step_tol finite and >= 0, 0 < lambda_min <= lambda_init <= lambda_max < inf.  lv_surf_sample: n < 2^31 - 1.
 *             K = 0 writes best only; n_src = 0 gives NO_OVERLAP everywhere with the poses untouched.
 * Order of judgement as for the surface rays: parameters and NULL or short arguments before the context (LV_EINVAL, nothing
 * written, "null context" last), then LV_ESTATE before lv_tsdf_configure.  Both calls READ the live volume: they change no bit of
 * S, W, the colour layer, the mesh, the packed ray states or any stale flag.  They run on the context's stream and return when
 * their outputs are written.  Nothing is allocated before the first call; lv_tsdf_configure and lv_destroy free the scratch. */
/* Names: lv_surf_*, as the rays' calls are: the set of lv_tsdf_* FUNCTIONS is closed ("Surface ray casting"). */
#define LV_SURF_SAMPLE_OUTSIDE 0
#define LV_SURF_SAMPLE_UNKNOWN 1
#define LV_SURF_SAMPLE_KNOWN   2
#define LV_SURF_ALIGN_CONVERGED 0
#define LV_SURF_ALIGN_MAX_ITERATIONS 1
#define LV_SURF_ALIGN_NO_OVERLAP 2
#define LV_SURF_ALIGN_CHUNK 512   /* source points per workgroup of the evaluation */
typedef struct lv_surf_align_params {   /* 64 bytes */
    int32_t  min_weight;         /* 1 */
    int32_t  max_iterations;     /* 50; 0..1000 */
    uint32_t min_points;         /* 6; >= 1 */
    int32_t  reserved;
    double   max_dist;           /* 0.4 m; finite, > 0 */
    double   huber;              /* 0.1 m; finite, >= 0; 0: quadratic */
    double   step_tol;           /* 1e-6 */
    double   lambda_init;        /* 1e-4 */
    double   lambda_min;         /* 1e-10 */
    double   lambda_max;         /* 1e8 */
} lv_surf_align_params;
typedef struct lv_surf_align_result {   /* 264 bytes, laid out as lv_ndt_result with cost for score */
    lv_graph_pose pose;
    double   cost;               /* E plus the gate charge at the pose */
    double   info[21];           /* the upper triangle of H at the pose, laid out as lv_graph_edge.info */
    double   last_step;          /* max-norm of the last accepted step (0 when none was) */
    double   lambda;             /* after the last iteration */
    uint32_t n_in;               /* source points IN at the pose */
    int32_t  status;             /* LV_SURF_ALIGN_CONVERGED, LV_SURF_ALIGN_MAX_ITERATIONS or LV_SURF_ALIGN_NO_OVERLAP */
    uint32_t accepted, rejected;
} lv_surf_align_result;
void lv_default_surf_align_params(lv_surf_align_params* p);
/* pts: n world points (x, y, z as f32 at the start of every `stride` bytes, stride >= 12).  out: 4 doubles per point (d, n_x, n_y,
 * n_z), zeros unless KNOWN; status: one byte per point (LV_SURF_SAMPLE_*); either may be NULL, not both.  n = 0 succeeds. */
int lv_surf_sample(lv_ctx* ctx, int min_weight, const void* pts, size_t stride, size_t n, double* out, uint8_t* status);
/* src: n_src points in the sensor frame; guesses: K poses sensor -> world.  params NULL: the defaults.  results: K records (may be
 * NULL when K = 0); best: 2 values. */
int lv_surf_align(lv_ctx* ctx, const lv_surf_align_params* params, const void* src, size_t stride, size_t n_src,
                  const lv_graph_pose* guesses, size_t K, lv_surf_align_result* results, int32_t best[2]);

/* ---- Submap merging ------------------------------------------------------------------------------------
 * One TSDF volume resampled into the context's volume under a rigid pose and folded in as evidence: mergeLayerAintoLayerB of
 * Voxblox and voxgraph, the other half of the submap workflow whose registration is lv_surf_align (the reference has no
 * counterpart).  A long run is kept as small submaps (saved volumes, each with a pose-graph node) and the global surface is
 * rebuilt from them after every optimisation; two robots' volumes, or volumes of another resolution, are fused.  A submap is a
 * volume as lv_tsdf_fetch gives it, with the grid it was fetched from; `pose` carries the submap's frame into the world.  (The
 * section stands here because the call takes an lv_graph_pose.)  The rule is the __host__ __device__ code of
 * limo-velo_amd/csrc/lv_surf_merge.hpp; tests/surf_merge_ref.py restates it in numpy.  It is shaped like "Depth fusion": one
 * thread owns a destination voxel, there are no atomics on the volume, and after one f64 step everything is integers, so the
 * result is the same bits whatever the schedule.
 * For every destination voxel.  Every f64 operation is a single rounded operation in the order written; nothing is fused.
 * Everything after step 3 is integers.  FR = 32.
 *   1. centre    p_a: the f32 centre of "Depth fusion" step 1, with the volume's present origin (after its shifts), widened to
 *                f64.
 *   2. into the submap   d = p - t; x_b = (R_0b d_0 + R_1b d_1) + R_2b d_2, that is R^T d, with R = R(q) as "NDT registration"
 *                builds it.
 *   3. lattice   u_b = (x_b - (double)sub.origin_b) / (double)sub.resolution - 0.5.  A u_b that is not finite or has
 *                |u_b| >= 2^24 makes the voxel OUTSIDE.  LV_MERGE_TRILINEAR: e_b = (int64)floor(u_b * 32.0 + 0.5), the position
 *                rounded to 1/32 of a source voxel.  LV_MERGE_NEAREST: e_b = 32 * (int64)floor(u_b + 0.5).  i_b = e_b >> 5 (floor)
 *                and f_b = e_b & 31.
 *   4. corners   corner (a, b, c) in {0, 1}^3 is the source voxel (i_x + a, i_y + b, i_z + c) with the weight w = wx wy wz,
 *                w_axis = f for offset 1 and 32 - f for offset 0; the weights sum to 2^15.  Corners of weight 0 are not read and
 *                need not exist: a voxel on the submap's last layer with f = 0 is still inside.  The voxel is OUTSIDE if a corner of
 *                non-zero weight lies outside [0, n - 1] on an axis; otherwise UNKNOWN if such a corner has W_c < min_weight;
 *                otherwise KNOWN.
 *   5. distances a_c = floor(S_c * 256 / W_c) in int64 (|a_c| <= 2^20, since |S| <= Ts * W and Ts <= 2^12); m = sum w a_c
 *                (|m| <= 2^35); Wn = sum w W_c (<= 2^33).  The distances are interpolated unweighted by W: a W-weighted mean does
 *                not reproduce a linear field (0.6 voxel off where W varies 1..40: tests/test_surf_merge_ref.py shows it).
 *   6. units     kq = (int64)floorf((sub.resolution / resolution) * 4096.0f + 0.5f), once per call in f32; LV_EINVAL unless
 *                512 <= kq <= 32768, a resolution ratio of 1/8 to 8.  sbar = floor(m * kq / 2^27), the distance in 1/256
 *                destination sub-unit (|m * kq| <= 2^50).  With Td the volume's T: sbar < -256 Td gives no contribution, the voxel is
 *                DROPPED; sbar > 256 Td gives sbar = 256 Td.
 *   7. weight    dW = max(1, Wn >> 15), dS = floor(sbar * dW / 256) (|sbar * dW| <= 2^38, |dS| <= Td * dW <= 2^30).  Then the
 *                voxel folds exactly as "TSDF and mesh" (one call) folds (dS, dW) with the volume's max_weight: |S + dS| <= 2^31
 *                (|S| <= Td * max_weight <= 2^30; the sum is held in int64) and the product (S + dS) * max_weight stays below 2^55.
 * Integer sums commute: merging A then B equals B then A bit for bit while W stays below max_weight (at max_weight the fold
 * rescales, as in "Depth fusion").  At the identity, and at whole-voxel shifts on one lattice with equal resolution, dW = W and
 * |dS - S| <= 1 + W / 256 (the floor of step 5).
 *   stats      voxels not OUTSIDE; voxels that contribute (dW > 0: KNOWN and not DROPPED); the sum of dW; voxels DROPPED.
 *   limits     the submap's grid as lv_tsdf_configure's (origin finite, resolution finite and > 0, nx, ny, nz each 1..1024,
 *              nx * ny * nz <= 2^28), trunc_cells 1..16 (Ts = 256 * trunc_cells); every source voxel 0 <= W <= 2^18 and
 *              |S| <= Ts * W, judged as lv_tsdf_load judges a load; the pose finite with a quaternion whose norm is within 1e-6
 *              of 1; min_weight >= 1; interp LV_MERGE_TRILINEAR or LV_MERGE_NEAREST.
 * Order of judgement as for lv_depth_integrate: the arguments before the context (LV_EINVAL, nothing written; the null context
 * last), then LV_ESTATE before lv_tsdf_configure, then kq against the volume's resolution (LV_EINVAL).  Once its arguments hold,
 * and whatever it then returns, the call sets a built mesh's stale = 1 and makes the next lv_surf_raycast pack the states anew,
 * as lv_tsdf_integrate does; it leaves the colour layer alone and never touches the occupancy side.  A submap whose box cannot
 * meet the volume gives LV_OK, zero stats and no launch.  The submap is staged once per call; the call runs on the context's
 * stream and returns when stats are written.
 * Known limits: colours are not merged: the submap carries no colour layer and the volume's layer is left as it is.  The
 * distance is resampled, not re-measured: under a rotation the truncation band keeps its width along the old rays, as in Voxblox.
 * A voxel takes evidence only where all its corners of non-zero weight are known, so a merged surface ends half a source voxel
 * inside the submap's known region. */
/* Names: lv_surf_*, as the registration's calls are: the set of lv_tsdf_* FUNCTIONS is closed ("Surface ray casting"). */
enum { LV_MERGE_TRILINEAR = 0, LV_MERGE_NEAREST = 1 };
typedef struct lv_surf_submap {          /* 48 bytes: a volume as lv_tsdf_fetch gives it, with the grid it was fetched from */
    float origin[3]; float resolution; int nx, ny, nz; int trunc_cells;
    const int32_t* S; const int32_t* W;  /* nx * ny * nz each, x fastest */
} lv_surf_submap;
typedef struct lv_surf_merge_params { int32_t min_weight; int32_t interp; int32_t reserved[2]; } lv_surf_merge_params;   /* 16 bytes */
/* Defaults: min_weight 1, LV_MERGE_TRILINEAR. */
void lv_default_surf_merge_params(lv_surf_merge_params* p);
/* pose: submap -> world.  p NULL: the defaults.  stats (may be NULL) as above. */
int  lv_surf_merge(lv_ctx* ctx, const lv_surf_submap* sub, const lv_graph_pose* pose, const lv_surf_merge_params* p, uint64_t stats[4]);

/* ---- instrumentation ------------------------------------------------------------------------- */
typedef struct lv_timing {
    float last_update_ms;      /* device time of the last lv_update (HIP events on the ctx stream) */
    float last_reduce_ms;      /* average device time of the dominant kernel in the last lv_update: pass_kernel (one launch
                                  per pass) or search_kernel (three-kernel pass) */
    float last_solve_ms;       /* average device time of fit_reduce_kernel + solve_kernel in the last lv_update (three-kernel pass; else 0) */
    int   last_passes;
    int   fallback_queries;    /* scan points that left the bucketed voxel levels (generic search) in the last update */
    float pass_match_ms[8];    /* device time of search_kernel per pass of the last profiled lv_update */
    float pass_solve_ms[8];    /* device time of fit_reduce_kernel + solve_kernel per pass */
    int   mailbox_resyncs;     /* updates (since lv_create) whose result mailbox failed its checksum at first sight: the host
                                  then waited with hipStreamSynchronize instead (expected: 0; an update that ends on a pass
                                  without matches carries no checksum and is not counted) */
    float pass_collective_ms[8]; /* multi-GPU forms, profiled updates: device time of the pass' collective (ncclAllGather of the
                                  workgroup partials / ncclAllReduce of the record), HIP events around it on the ctx stream */
} lv_timing;
int lv_get_timing(lv_ctx* ctx, lv_timing* out);
/* 0 = off; 1 = per-kernel HIP-event timing inside lv_update (adds event records to the stream);
 * 2 = search_kernel / fit_reduce_kernel stamp 8 shader-clock values per workgroup (phase boundaries) */
int lv_set_profiling(lv_ctx* ctx, int enabled);
/* after a pass run with lv_set_profiling(ctx, 2): out receives n_blocks x 8 clock64() stamps */
int lv_get_phase_clocks(lv_ctx* ctx, long long* out, int capacity_blocks, int* n_blocks);
/* captured passes (lv_iterate / lv_set_capture): how many scan points were decided at voxel-bucket level
 * 0, 1, 2 ([0..2]), by the generic multi-level search ([3]) or by brute force ([4]) since the last begin */
int lv_get_level_histogram(lv_ctx* ctx, int out[8]);
/* shader-clock stamps of the solve kernel's phases of the last update: 16 passes x 16 stamps (capacity >= 256) */
int lv_get_solve_clocks(lv_ctx* ctx, long long* out, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* LIMOVELO_HIP_H */
