// lv_host.hpp — host-side state behind the C-ABI (include/limovelo_hip.h).
#pragma once
#include "lv_note.hpp"

#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/limovelo_hip.h"
#include "lv_device.hpp"
#include "lv_common.hpp"
#include "lv_buffers.hpp"
#include "lv_exchange.hpp"
#include "lv_update.hpp"
#include "lv_mapinc.hpp"

namespace lv {

struct MapStats {   // == lv_map_stats (include/limovelo_hip.h)
    uint64_t living, ids, capacity;
    uint64_t pool_used[4], pool_cap[4];
    uint64_t slots_used[4], slots_cap[4];
    uint64_t tombstones, dropped;
    uint64_t relinearisations, incremental_adds;
    uint64_t bytes;
};

constexpr int POOL_CELL = BUCKET_LEVELS;   // index of the voxel lists in MapStore::pool_cap / pool_base and the statistics

struct MapStore {
    // ---- points by id (insertion order; deleted ids keep their slot with x = +inf)
    float4* d_orig = nullptr;
    float4* d_orig2 = nullptr;     // compaction target (swapped with d_orig by relinearise)
    size_t capacity = 0;           // id slots allocated
    uint32_t n_ids = 0;            // ids handed out
    uint32_t m = 0;                // living points
    // ---- build scaffolding: Morton-sorted copy + per-level occupancy tables over it
    float4* d_sorted = nullptr;
    uint64_t* d_keys = nullptr;
    uint64_t* d_keys_sorted = nullptr;
    uint32_t* d_idx = nullptr;
    uint32_t* d_idx_sorted = nullptr;
    void* d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    uint32_t* d_counts = nullptr;
    uint4* d_tables[N_OCC] = {};           // occupied voxels -> run in d_sorted: [0], [1] levels 0, 1; [OCC_CELL] level 2 (lives on as the voxel-list table)
    uint32_t table_size[N_OCC] = {};
    uint32_t n_cells[N_OCC] = {};
    // ---- levels 0, 1: neighbourhood buckets with slack (built straight into their pools: no float4 staging copy since round 6)
    uint4* d_btable[BUCKET_LEVELS] = {};
    SlotAux* d_baux[BUCKET_LEVELS] = {};
    uint32_t btable_size[BUCKET_LEVELS] = {};
    float* d_bxyz[BUCKET_LEVELS] = {};    // 12-byte points: what the search kernel streams
    uint32_t* d_bidx[BUCKET_LEVELS] = {}; // ids (ascending inside a bucket)
    uint16_t* d_backpos[BUCKET_LEVELS] = {};   // [l][id * 27 + c]: position of a point inside the level-l bucket of its neighbour c
                                          // (BACKPOS_FAR: beyond 16 bits, found by binary search): a deletion is 27 probes + 27 direct writes per level
    uint32_t* d_cellpos = nullptr;        // [id]: position of a point in its voxel's list (allocated with d_backpos)
    size_t backptr_cap = 0;               // ids they are allocated for
    uint32_t* d_biglist = nullptr;        // build scratch: buckets of more than 64 points (a workgroup each)
    size_t biglist_cap = 0;
    // tile groups (level-0 storage only; read by the map queries and the surface pass): level-1 voxel -> {start, extent} of the region its eight level-0 runs were laid out in
    uint4* d_gtable = nullptr;
    uint32_t gtable_size = 0;
    uint32_t* d_gext = nullptr;           // build scratch: a group's extent while its runs take their places, then the groups' offsets
    uint32_t* d_goff = nullptr;
    size_t gscratch_cap = 0;
    uint32_t* d_broken = nullptr;         // groups an insert batch broke up (table slots) + their re-layout plans (lv_mapinc.hpp inc_regroup_*)
    RegroupPlan* d_regroup = nullptr;
    uint32_t broken_cap = 0;
    uint32_t n_groups = 0;
    uint4* d_comp[BUCKET_LEVELS] = {};     // (per instance of the insert machinery, like every work list and scratch table below) runs an insert batch compacts in place (lv_mapinc.hpp inc_compact_*), their staging area
    float4* d_cstage[BUCKET_LEVELS] = {};
    uint32_t* d_cnew[BUCKET_LEVELS] = {};
    uint32_t comp_cap = 0, cstage_cap = 0;
    size_t pool_cap[BUCKET_LEVELS + 1] = {};     // entries per pool: bucket levels 0, 1; [POOL_CELL]: d_cell4
    uint32_t pool_base[BUCKET_LEVELS + 1] = {};  // entries laid out by the last (re)build; the rest is split into arenas
    uint32_t n_bcells[BUCKET_LEVELS] = {};
    uint32_t* d_cell_slots = nullptr;  // scratch: table slots of the bucket voxels of the level being built
    uint32_t* d_bcount = nullptr;
    uint32_t* d_bcap = nullptr;
    uint32_t* d_boff = nullptr;
    size_t cells_cap = 0;
    uint32_t* d_flags = nullptr;       // [0] = append cursor, [1] = overflow flag
    void* d_scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    // ---- level 2: one list per voxel
    SlotAux* d_caux = nullptr;
    uint32_t caux_size = 0;
    float4* d_cell4 = nullptr;
    // ---- incremental maintenance (lv_mapinc.hpp)
    MapCounters* d_cnt = nullptr;      // [BUCKET_LEVELS]: one per instance of the incremental machinery; [0] also carries the batch's front half, the boxes and the lists
    MapCounters* h_cnt = nullptr;      // pinned mirror
    float4* d_new = nullptr;           // staged batch
    uint64_t* d_nkeys = nullptr;
    uint64_t* d_nkeys_sorted = nullptr;
    uint32_t* d_nidx = nullptr;
    uint32_t* d_nidx_sorted = nullptr;
    uint32_t* d_nalive = nullptr;
    uint32_t* d_napos = nullptr;
    uint32_t* d_nsurv = nullptr;       // the batch's survivors in sorted-batch (Morton box) order, + the flags / positions that build it
    uint32_t* d_nsflag = nullptr;
    uint32_t* d_nspos = nullptr;
    uint32_t* d_rank[BUCKET_LEVELS] = {};
    void* d_ntmp = nullptr;
    size_t ntmp_bytes = 0, batch_cap = 0;
    // voxel groups of a batch (lv_mapinc.hpp GroupRW)
    uint4* d_gtab[BUCKET_LEVELS] = {};    // [instance]
    uint32_t gtab_size = 0;
    uint32_t* d_prank[BUCKET_LEVELS] = {};
    uint32_t* d_pslot[BUCKET_LEVELS] = {};
    uint32_t* d_gbase[BUCKET_LEVELS] = {};
    uint32_t* d_gslot[BUCKET_LEVELS] = {};
    uint4* d_gdst[BUCKET_LEVELS] = {};
    uint32_t* d_gcnt = nullptr;        // [instance * 4 * LIST_SHARDS]: the sharded cursors of the batch's work lists
    uint4* d_reloc[BUCKET_LEVELS] = {};
    uint32_t reloc_cap = 0;
    float4* d_dead = nullptr;
    size_t dead_cap = 0;
    uint32_t* d_alive = nullptr;       // flags / ranks over all ids (eviction of the oldest, compaction)
    uint32_t* d_apos = nullptr;
    void* d_ascan_tmp = nullptr;
    size_t ascan_tmp_bytes = 0, alive_cap = 0;
    // 0.2 m boxes of ikd-Tree's down-sampling insert
    uint4* d_box = nullptr;
    uint32_t* d_box_next = nullptr;
    uint32_t box_size = 0;
    size_t box_next_cap = 0;
    bool have_boxes = false;

    // the tail of an incremental insert (new ids / living points / overflow, read from the device counters) is settled by the
    // next call that needs the map's bookkeeping, not by a wait at the end of the insert
    bool sweep_evict = true;     // lv_map_evict_box tests runs, not points (inc_evict_sweep_kernel; LV_SWEEP_EVICT=0 / lv_set_option: the per-point search)
    bool merged_back = true;     // independent stages of the insert's back half share launches (LV_MERGED_INSERT=0 / lv_set_option: off)
    bool surv_list = true;       // large down-sampling batches: the append passes walk a survivor list in Morton (box sort) order (LV_SURV_LIST=0 / "survivor_list": off)
    bool small_front = true;     // batches of up to 2048 points: the insert's front half in one workgroup launch (LV_SMALL_INSERT=0: off)
    NoteBoard notes;             // the insert's counters come back as a note (lv_note.hpp): n_new, n_dead, dropped, overflow
    uint32_t counters_seq = 0;
    hipStream_t counters_stream = nullptr;
    bool counters_pending = false;
    bool pending_counted_kill = false;
    uint32_t pending_n_dead = 0;
    int settle(hipStream_t stream);
    bool origin_set = false;
    float origin[3] = {0, 0, 0};
    float cell = 0.5f;
    float bbox_min[3], bbox_max[3];    // of everything ever inserted since the origin was chosen
    bool built = false;                // the search structure describes d_orig[0 .. n_ids)
    uint64_t relinearisations = 0, incremental_adds = 0, dropped_total = 0, tombstones = 0;
    MapView view{};

    int build_buckets(hipStream_t stream, int level, uint32_t n_occupied);
    int build_cells(hipStream_t stream, uint32_t n_occupied);
    int reserve(size_t cap);           // room for `cap` ids (keeps d_orig[0 .. n_ids))
    int rebuild(hipStream_t stream);   // search structure over d_orig[0 .. n_ids) (all of them living)
    // compaction of the living (ids become ranks) + rebuild
    int relinearise(hipStream_t stream);
    // k points staged in d_new[0 .. k): ikd-Tree Add_Points(points, downsample) without a rebuild; falls back to
    // relinearise when a pool or table runs full.  Synchronises the stream.
    // build_if_empty: Mapper::add's rule (an empty map is BUILT from the points, Mapper.cpp:22-27) instead of
    // Add_Points's (the box rule applies among the new points themselves)
    int add_staged(hipStream_t stream, uint32_t k, int downsample, float box_length, bool build_if_empty);
    int ensure_counters();
    int reset_batch_counters(hipStream_t stream);   // n_new, n_dead, overflow, dropped of every instance back to zero (after ensure_counters)
    int reserve_batch(size_t k);
    int evict_box(hipStream_t stream, const float lo[3], const float hi[3], int keep_inside, uint32_t* n_evicted);
    int evict_oldest(hipStream_t stream, uint32_t n_oldest, uint32_t* n_evicted);
    int kill_dead_list(hipStream_t stream, uint32_t n_dead);
    // A removed point turns DEAD_ENTRIES_PER_POINT entries into tombstones: kill_dead_list runs inc_kill_kernel once per bucket
    // level (27 neighbourhood buckets each) and instance 0 also kills the entry in the point's level-2 voxel list
    static constexpr uint64_t DEAD_ENTRIES_PER_POINT = 27 * BUCKET_LEVELS + 1;
    int retire_dead_list(hipStream_t stream, uint32_t* n_removed);                  // the filled dead list: kill, then finish_removal
    int finish_removal(hipStream_t stream, uint32_t n_dead, uint32_t* n_removed);   // m, tombstones, view; an emptied map is rebuilt
    int ensure_boxes(hipStream_t stream, float box_length);
    int ensure_alive_scratch();
    bool needs_relinearise(size_t incoming) const;
    // background re-linearisation (lv_rebuild.hpp, round 5): while a compacted copy of this map is being rebuilt on another stream /
    // thread, the stop-the-world relinearise is deferred (only id-space exhaustion still forces it)
    bool defer_relinearise = false;
    uint32_t last_new = 0;    // survivors of the previous insert batch: sizes the next batch's per-survivor launches (an estimate: add_staged)
    bool have_last_new = false;
    bool pool_low = false;    // the last insert left less than a quarter of the bucket pool's free part (settle): a re-linearisation is wanted
    uint32_t slice_wgs = 0;   // != 0: the large grids of a (re)build go out in slices of that many workgroups (a store rebuilt in the background)
    bool wants_relinearise(size_t incoming) const;   // the trigger, whatever defer_relinearise says
    // the living points of this map, compacted in id order, into dst.d_orig (dst: an idle store whose search structure is not
    // built yet): enqueued on `stream`, no host wait; m must be settled
    int snapshot_into(MapStore& dst, hipStream_t stream);
    MapRW rw(int inst = 0) const;   // instance 0: level-0 buckets, voxel lists, tile groups; instance 1: level-1 buckets
    void refresh_view();
    void stats(MapStats* out) const;
    void release();
    // stamp of the map as it stands: refresh_view (which every build, insert, eviction, re-linearisation and store swap ends with)
    // draws a new one from a process-wide counter, so two states of a map — or two stores — never share one (QueryStore::ensure_rank)
    uint64_t gen = 0;
};

// Map queries (lv_query.hip): batched k-NN / radius / box searches of arbitrary points against the active store.  Owns its staging
// and result buffers (grown on demand, freed by release); nothing here is shared with the update or the background rebuild.
struct QueryStore {
    PointStage pts;                // queries, packed xyz (doubling from QUERY_FLOOR floats)
    DevBuf<uint32_t> d_idx;        // k-NN: n x k results; radius: the ids found; box: the ranks found
    DevBuf<float> d_d2;            // k-NN / radius: their distances; box: their xyz
    DevBuf<int32_t> d_found;
    DevBuf<uint32_t> d_idx2;       // radius: the segmented sort's output
    DevBuf<float> d_d22;
    DevBuf<uint32_t> d_off;        // box: positions (n_ids + 1)
    DevBuf<uint32_t> d_cnt;        // box: flags by id
    DevBuf<uint64_t> d_roff;       // radius: per-query counts -> exclusive offsets of the queries' segments (n + 1), 64-bit
    DevBuf<uint64_t> d_rcnt;
    DevBuf<void> d_tmp;            // hipcub scratch
    DevBuf<uint32_t> d_rank;       // rank among the living by id, valid for the map whose stamp is rank_gen
    DevBuf<uint32_t> d_flag;
    uint64_t rank_gen = 0;
    PinBuf<uint32_t> h_word;       // a total read back by the host
    int stage_queries(hipStream_t stream, const void* q, size_t stride, size_t n);
    // nullptr when ranks equal ids (no dead id); else d_rank, rebuilt when the map's stamp moved
    int ensure_rank(const MapStore& map, hipStream_t stream, const uint32_t** rank);
    int knn(const MapStore& map, hipStream_t stream, const void* q, size_t stride, size_t n, int k, float max_dist, uint32_t* idx, float* d2,
            int32_t* found);
    int radius(const MapStore& map, hipStream_t stream, const void* q, size_t stride, size_t n, float radius, size_t* offsets, uint32_t* idx,
               float* d2, size_t capacity, size_t* total);
    int box(const MapStore& map, hipStream_t stream, const float lo[3], const float hi[3], uint32_t* idx, float* xyz, size_t capacity,
            size_t* n_out);
    void release();
};

// Multi-hypothesis passes and updates of the current scan (lv_batch.hip: lv_iterate_batch / lv_update_batch).  Its own
// buffers, grown on demand and kept: the hypothesis records (all M), the hand-over records and block partials of one chunk of
// hypotheses, and a KfDev that only knn_search's counters write (the context's kf is never touched by a batch).
struct BatchHyp;
// bytes of hand-over records (qrec_slots(K) x 16 B per point and hypothesis: 128 B for K = 5) one chunk may use; a batch with
// more is processed chunk after chunk (results do not depend on the chunking)
constexpr size_t BATCH_RECORD_BUDGET = (size_t)256 << 20;
struct BatchStore {
    DevBuf<BatchHyp> d_hyp;
    PinBuf<BatchHyp> h_hyp;
    DevBuf<float4> d_qrec;
    DevBuf<double> d_part;
    DevBuf<KfDev> d_sink;
    int chunk_hyp = 0;             // lv_set_option "batch_chunk_hypotheses": at most this many hypotheses per chunk (0: the budget alone)
    size_t chunk_size(uint32_t n, int num_match) const;
    // m hypotheses xs (prior covariance P) against the map and the scan (n sorted points): solve = false runs one pass without
    // a solve (lv_iterate_batch).  Outputs (each optional): final states, posterior covariances (m x 529), passes, the record
    // of each hypothesis' last pass (m x SUMS_LEN).  Returns once the host arrays are written.
    int run(const lv_params& prm, int max_blocks, const MapView& map, const float4* scan, uint32_t n, hipStream_t stream, const lv_state* xs,
            size_t m, const double* P, bool solve, lv_state* x_out, double* P_out, int* passes, double* recs);
    void release();
};

// (the launches of the update, their parameter structs and the driver that issues them: lv_update.hpp)
// lv_predict.hip
int launch_filter_to_kf(hipStream_t stream, const FilterDev* f, KfDev* kf);
// lv_scan.hip
struct CloudPoint;
struct ScanStore {
    float4* d_raw = nullptr;     // upload order; w = original index
    float4* d_sorted = nullptr;  // Morton order (LiDAR frame)
    uint32_t* d_keys = nullptr;
    uint32_t* d_keys_sorted = nullptr;
    uint32_t* d_idx = nullptr;
    uint32_t* d_idx_sorted = nullptr;
    void* d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    size_t capacity = 0;
    uint32_t n = 0;
    int route = 0;               // what produced the scan: LV_SCAN_ROUTE_* (lv_scan_route); a decline followed by the general chain: general
    uint32_t* d_tile_order = nullptr;  // search-kernel tiles, farthest-from-sensor first (order_tiles)
    uint32_t n_tiles = 0, tile_cap = 0;
    uint32_t tile_points = 0;          // scan points per search-kernel workgroup (256 / lanes_per_query); 0: no ordering
    // row f-2 (de-skew + voxel grid): raw time-stamped input and work buffers
    float4* d_in = nullptr;
    double* d_times = nullptr;
    float4* d_desk = nullptr;
    MotionState* d_states = nullptr;
    uint64_t* d_vkeys = nullptr;
    uint64_t* d_vkeys_sorted = nullptr;
    uint32_t* d_vidx = nullptr;
    uint32_t* d_vidx_sorted = nullptr;
    uint32_t* d_heads = nullptr;
    uint32_t* d_hpos = nullptr;
    unsigned* d_bounds = nullptr;
    void* d_vsort_tmp = nullptr;
    void* d_vscan_tmp = nullptr;
    size_t vsort_tmp_bytes = 0, vscan_tmp_bytes = 0, raw_cap = 0, states_cap = 0;
    int reserve(size_t cap);
    int reserve_raw(size_t cap, size_t n_states);
    int deskew_downsample(hipStream_t stream, uint32_t n_in, uint32_t n_states, const MotionState& xt2, float leaf, float sort_cell);
    bool small_enabled = true;   // windows of up to 2048 points take the one-launch chain (LV_SMALL_WINDOW=0 / lv_set_option: off)
    int voxel_and_sort(hipStream_t stream, uint32_t n_in, float leaf, float sort_cell, bool try_small = false);
    bool small_window_applies(uint32_t n_in) const;
    int window_small(hipStream_t stream, const float4* src, uint32_t n_in, uint32_t n_states, const MotionState* xt2, float leaf,
                     float sort_cell, bool* fell_back);
    bool large_enabled = true;   // larger windows: de-skew + bounds, keys, sort, one tail workgroup (LV_LARGE_WINDOW=0 / lv_set_option: off)
    bool large_window_applies(uint32_t n_in, uint32_t n_states, float leaf) const;
    int window_large(hipStream_t stream, const struct CloudPoint* cloud, uint32_t n_in, uint32_t n_states, const MotionState& xt2, float leaf,
                     float sort_cell, bool* fell_back);
    NoteBoard notes;             // (points out, status) of the window kernels: lv_note.hpp
    long long* d_tail_clk = nullptr;   // LV_TAIL_CLK=1: phase stamps of window_tail_kernel
    int sort(hipStream_t stream, const float bbox_min[3], float cell);
    int order_tiles(hipStream_t stream, uint32_t tile_points);
    int reserve_tiles(uint32_t nt);
    void release();
};

// ---- row f-4: LiDAR wire formats -> device-resident LiDAR buffer (lv_cloud.hip) ----------------------------
struct CloudFormat {   // == lv_cloud_format
    uint32_t point_step, off_x, off_y, off_z, off_time;
    int time_type;
    uint32_t off_intensity;
    int intensity_type;
    uint32_t off_range;
    int range_type;
    int relative_time;
};
struct IngestParams {  // == lv_ingest_params
    uint64_t header_stamp_usec;
    int stamp_beginning, offset_beginning;
    double full_rotation_time;
    int downsample_rate;
    float min_dist;
};
struct CloudPoint {    // the reference's Point (include/Headers/Objects.hpp:20-28), 32 bytes
    float x, y, z, pad_;
    double time;
    float intensity, range;
};
static_assert(sizeof(CloudPoint) == 32, "reference Point layout");

struct CloudStore {
    CloudPoint* d_buf = nullptr;   // BUFFER_L: time ordered, live range [head, size)
    uint32_t head = 0, size = 0;
    size_t buf_cap = 0;
    unsigned char* d_rawmsg = nullptr;
    unsigned char* h_rawmsg = nullptr;   // pinned staging, two buffers alternating between messages
    unsigned char* h_rawmsg2 = nullptr;
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    bool stage_busy[2] = {false, false};
    int stage_next = 0;
    size_t raw_cap = 0;
    CloudPoint* d_decoded = nullptr;
    CloudPoint* d_kept = nullptr;
    unsigned char* d_keep = nullptr;
    uint64_t* d_keys = nullptr;
    uint64_t* d_keys_sorted = nullptr;
    uint32_t* d_ids = nullptr;
    uint32_t* d_ids_sorted = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0, msg_cap = 0;
    uint32_t* d_count = nullptr;
    uint32_t* h_count = nullptr;   // pinned
    // clear_before does not wait for its result (the new head): the kernel posts it as a note (lv_note.hpp) that is picked up
    // by whoever touches the buffer next (settle), by which time it has long arrived — the wait was one of six host/device
    // round trips of a 100 Hz cycle; the window's index range comes back as a note too (words 0, 1; the clear's: word 3)
    NoteBoard notes;
    double clear_t = 0.0;        // the pending Buffer::clear(t)
    hipStream_t clear_stream = nullptr;
    bool clear_pending = false;
    int settle();
    int init();
    int reserve_msg(size_t n, size_t bytes);
    int reserve_buffer(hipStream_t stream, size_t total);
    int ingest(hipStream_t stream, const void* data, size_t n, const CloudFormat& fmt, const IngestParams& prm, double begin_time,
               size_t* n_kept);
    // reset8 != nullptr: the kernel also sets those eight words to the voxel grid's "no bounds seen" (ScanStore::d_bounds)
    int window(hipStream_t stream, double t1, double t2, uint32_t* lo, uint32_t* hi, unsigned* reset8 = nullptr);
    int clear_before(hipStream_t stream, double t);
    int unpack(hipStream_t stream, uint32_t lo, uint32_t n, float4* xyz, double* times);
    void release();
};

}  // namespace lv
