// lv_stores.hpp — the map, the scan and the LiDAR buffer of a context: what they hold and how their memory grows.
//
// Host code only.  Every device and pinned pointer is a DevBuf / PinBuf of lv_buffers.hpp, under the rules of DESIGN.md
// "Host-side buffers": growth is exact or doubling (rule 1), a failed allocation leaves {nullptr, 0} (rule 2), and what must
// survive a growth goes through grow_keep (rule 4).  A buffer converts to its pointer, so the code that launches kernels reads as it
// did with plain pointers.  The reserve paths and release() are defined here; tests/emu/stores_emu.cpp compiles them with g++ against
// tests/emu/hip/hip_runtime.h and tests/test_stores_host.py holds every one of them to its growth, to what it keeps, to a failure at
// each of its HIP calls and to a release without leaks.  Everything that launches a kernel is defined in lv_map.hip, lv_scan.hip and
// lv_cloud.hip.
//
// GROUP CAPACITIES (capacity, batch_cap, raw_cap, msg_cap and the sizes derived from them): a field that many readers use
// stands for a whole group of buffers.  It is 0 while any member of its group is missing and is written last, after every member is
// there: a call after a failed one allocates again and never reports room over a null buffer.  The doubling starts at the floor
// again then, which gives the size an unbroken history gives (every capacity is floor * 2^j).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>

#include "lv_buffers.hpp"
#include "lv_common.hpp"
#include "lv_device.hpp"
#include "lv_mapinc.hpp"
#include "lv_note.hpp"

namespace lv {

// Bytes of hipcub scratch for n items.  Defined beside the hipcub calls they size (lv_map.hip, lv_scan.hip, lv_cloud.hip); the host
// tests define them as fixed formulas.
int sort_pairs_scratch_u64(size_t n, int end_bit, size_t* bytes);              // DeviceRadixSort::SortPairs: 8-byte keys, bits [0, end_bit), uint32_t values
int sort_pairs_scratch_u32(size_t n, int end_bit, size_t* bytes);              // ... 4-byte keys
int exclusive_sum_scratch(size_t n, size_t* bytes);                            // DeviceScan::ExclusiveSum over uint32_t
int select_flagged_scratch(size_t n, size_t* bytes);                           // DeviceSelect::Flagged: CloudPoint items, byte flags

inline uint32_t next_pow2(uint64_t v) {   // (table sizes: at least 64 slots)
    uint32_t p = 64;
    while (p < v) p <<= 1;
    return p;
}
// the capacity a group grows to: doubling from `floor` (or from what it has) until it holds n
inline size_t grown(size_t have, size_t floor, size_t n) {
    size_t c = have ? have : floor;
    while (c < n) c *= 2;
    return c;
}

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
    DevBuf<float4> d_orig;
    DevBuf<float4> d_orig2;        // compaction target (swapped with d_orig by relinearise)
    size_t capacity = 0;           // id slots allocated: the group reserve() grows (d_orig .. d_dead, and the chains and positions by id once they exist)
    uint32_t n_ids = 0;            // ids handed out
    uint32_t m = 0;                // living points
    // ---- build scaffolding: Morton-sorted copy + per-level occupancy tables over it
    DevBuf<float4> d_sorted;
    DevBuf<uint64_t> d_keys;
    DevBuf<uint64_t> d_keys_sorted;
    DevBuf<uint32_t> d_idx;
    DevBuf<uint32_t> d_idx_sorted;
    DevBuf<void> d_sort_tmp;
    DevBuf<uint32_t> d_counts;
    DevBuf<uint4> d_tables[N_OCC];         // occupied voxels -> run in d_sorted: [0], [1] levels 0, 1; [OCC_CELL] level 2 (lives on as the voxel-list table)
    uint32_t table_size[N_OCC] = {};       // slots in use (a power of two: the hash mask), == the buffer's cap
    uint32_t n_cells[N_OCC] = {};
    // ---- levels 0, 1: neighbourhood buckets with slack (built straight into their pools: no float4 staging copy since round 6)
    DevBuf<uint4> d_btable[BUCKET_LEVELS];
    DevBuf<SlotAux> d_baux[BUCKET_LEVELS];
    uint32_t btable_size[BUCKET_LEVELS] = {};
    DevBuf<float> d_bxyz[BUCKET_LEVELS];     // 12-byte points: what the search kernel streams
    DevBuf<uint32_t> d_bidx[BUCKET_LEVELS];  // ids (ascending inside a bucket)
    DevBuf<uint16_t> d_backpos[BUCKET_LEVELS];   // [l][id * 27 + c]: position of a point inside the level-l bucket of its neighbour c
                                          // (BACKPOS_FAR: beyond 16 bits, found by binary search): a deletion is 27 probes + 27 direct writes per level
    DevBuf<uint32_t> d_cellpos;           // [id]: position of a point in its voxel's list (allocated with d_backpos, last: its cap is the ids they are allocated for)
    DevBuf<uint32_t> d_biglist;           // build scratch: buckets of more than 64 points (a workgroup each)
    // tile groups (level-0 storage only; read by the map queries and the surface pass): level-1 voxel -> {start, extent} of the region its eight level-0 runs were laid out in
    DevBuf<uint4> d_gtable;
    uint32_t gtable_size = 0;
    DevBuf<uint32_t> d_gext;              // build scratch: a group's extent while its runs take their places, then the groups' offsets
    DevBuf<uint32_t> d_goff;
    DevBuf<uint32_t> d_broken;            // groups an insert batch broke up (table slots) + their re-layout plans (lv_mapinc.hpp inc_regroup_*)
    DevBuf<RegroupPlan> d_regroup;
    uint32_t broken_cap = 0;
    uint32_t n_groups = 0;
    DevBuf<uint4> d_comp[BUCKET_LEVELS];     // (per instance of the insert machinery, like every work list and scratch table below) runs an insert batch compacts in place (lv_mapinc.hpp inc_compact_*), their staging area
    DevBuf<float4> d_cstage[BUCKET_LEVELS];
    DevBuf<uint32_t> d_cnew[BUCKET_LEVELS];
    uint32_t comp_cap = 0, cstage_cap = 0;
    size_t pool_cap[BUCKET_LEVELS + 1] = {};     // entries per pool: bucket levels 0, 1; [POOL_CELL]: d_cell4
    uint32_t pool_base[BUCKET_LEVELS + 1] = {};  // entries laid out by the last (re)build; the rest is split into arenas
    uint32_t n_bcells[BUCKET_LEVELS] = {};
    DevBuf<uint32_t> d_cell_slots;     // scratch: table slots of the bucket voxels of the level being built
    DevBuf<uint32_t> d_bcount;
    DevBuf<uint32_t> d_bcap;
    DevBuf<uint32_t> d_boff;           // (the last of the four: its cap is the voxels they are allocated for)
    DevBuf<uint32_t> d_flags;          // [0] = append cursor, [1] = overflow flag
    DevBuf<void> d_scan_tmp;
    // ---- level 2: one list per voxel
    DevBuf<SlotAux> d_caux;
    DevBuf<float4> d_cell4;
    // ---- incremental maintenance (lv_mapinc.hpp)
    DevBuf<MapCounters> d_cnt;         // [BUCKET_LEVELS]: one per instance of the incremental machinery; [0] also carries the batch's front half, the boxes and the lists
    PinBuf<MapCounters> h_cnt;         // pinned mirror
    DevBuf<float4> d_new;              // staged batch
    DevBuf<uint64_t> d_nkeys;
    DevBuf<uint64_t> d_nkeys_sorted;
    DevBuf<uint32_t> d_nidx;
    DevBuf<uint32_t> d_nidx_sorted;
    DevBuf<uint32_t> d_nalive;
    DevBuf<uint32_t> d_napos;
    DevBuf<uint32_t> d_nsurv;          // the batch's survivors in sorted-batch (Morton box) order, + the flags / positions that build it
    DevBuf<uint32_t> d_nsflag;
    DevBuf<uint32_t> d_nspos;
    DevBuf<uint32_t> d_rank[BUCKET_LEVELS];
    DevBuf<void> d_ntmp;
    size_t batch_cap = 0;              // points a batch may hold: the group reserve_batch() grows, with the sizes derived from it (gtab_size, reloc_cap, broken_cap, comp_cap, cstage_cap)
    // voxel groups of a batch (lv_mapinc.hpp GroupRW)
    DevBuf<uint4> d_gtab[BUCKET_LEVELS];    // [instance]
    uint32_t gtab_size = 0;
    DevBuf<uint32_t> d_prank[BUCKET_LEVELS];
    DevBuf<uint32_t> d_pslot[BUCKET_LEVELS];
    DevBuf<uint32_t> d_gbase[BUCKET_LEVELS];
    DevBuf<uint32_t> d_gslot[BUCKET_LEVELS];
    DevBuf<uint4> d_gdst[BUCKET_LEVELS];
    DevBuf<uint32_t> d_gcnt;           // [instance * 4 * LIST_SHARDS]: the sharded cursors of the batch's work lists
    DevBuf<uint4> d_reloc[BUCKET_LEVELS];
    uint32_t reloc_cap = 0;
    DevBuf<float4> d_dead;             // the dead list, one slot per id (its cap is the id capacity: the list cannot overflow)
    DevBuf<uint32_t> d_alive;          // flags / ranks over all ids (eviction of the oldest, compaction)
    DevBuf<uint32_t> d_apos;
    DevBuf<void> d_ascan_tmp;
    // 0.2 m boxes of ikd-Tree's down-sampling insert
    DevBuf<uint4> d_box;
    DevBuf<uint32_t> d_box_next;
    uint32_t box_size = 0;
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
    int reserve(size_t cap);           // room for `cap` ids (keeps d_orig[0 .. n_ids), the box chains and the positions by id)
    int reserve_ids(size_t ncap);      // (reserve's allocations)
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
    int reserve_cells(size_t n);       // the build's scratch per bucket voxel / list voxel, for n of them (lv_map.hip)
    int reserve_boxes();               // the box table and the chains for `capacity` ids (ensure_boxes' sizing)
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

struct CloudPoint;
struct ScanStore {
    DevBuf<float4> d_raw;        // upload order; w = original index
    DevBuf<float4> d_sorted;     // Morton order (LiDAR frame)
    DevBuf<uint32_t> d_keys;
    DevBuf<uint32_t> d_keys_sorted;
    DevBuf<uint32_t> d_idx;
    DevBuf<uint32_t> d_idx_sorted;
    DevBuf<void> d_sort_tmp;
    size_t capacity = 0;         // points the scan may hold: the group reserve() grows (d_raw .. d_sort_tmp)
    uint32_t n = 0;
    int route = 0;               // what produced the scan: LV_SCAN_ROUTE_* (lv_scan_route); a decline followed by the general chain: general
    DevBuf<uint32_t> d_tile_order;     // search-kernel tiles, farthest-from-sensor first (order_tiles)
    uint32_t n_tiles = 0;
    uint32_t tile_points = 0;          // scan points per search-kernel workgroup (256 / lanes_per_query); 0: no ordering
    // row f-2 (de-skew + voxel grid): raw time-stamped input and work buffers
    DevBuf<float4> d_in;
    DevBuf<double> d_times;
    DevBuf<float4> d_desk;
    DevBuf<MotionState> d_states;
    DevBuf<uint64_t> d_vkeys;
    DevBuf<uint64_t> d_vkeys_sorted;
    DevBuf<uint32_t> d_vidx;
    DevBuf<uint32_t> d_vidx_sorted;
    DevBuf<uint32_t> d_heads;
    DevBuf<uint32_t> d_hpos;
    DevBuf<unsigned> d_bounds;
    DevBuf<void> d_vsort_tmp;
    DevBuf<void> d_vscan_tmp;
    size_t raw_cap = 0;          // raw points of a de-skew: the group reserve_raw() grows (d_in .. d_hpos and the two scratches)
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
    DevBuf<long long> d_tail_clk;      // LV_TAIL_CLK=1: phase stamps of window_tail_kernel
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
    DevBuf<CloudPoint> d_buf;      // BUFFER_L: time ordered, live range [head, size)
    uint32_t head = 0, size = 0;
    DevBuf<unsigned char> d_rawmsg;
    PinBuf<unsigned char> h_rawmsg;      // pinned staging, two buffers alternating between messages
    PinBuf<unsigned char> h_rawmsg2;
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    bool stage_busy[2] = {false, false};
    int stage_next = 0;
    size_t raw_cap = 0;            // bytes of a message: the group of d_rawmsg and its two stagings
    DevBuf<CloudPoint> d_decoded;
    DevBuf<CloudPoint> d_kept;
    DevBuf<unsigned char> d_keep;
    DevBuf<uint64_t> d_keys;
    DevBuf<uint64_t> d_keys_sorted;
    DevBuf<uint32_t> d_ids;
    DevBuf<uint32_t> d_ids_sorted;
    DevBuf<void> d_tmp;
    size_t msg_cap = 0;            // points of a message: the group d_decoded .. d_tmp
    DevBuf<uint32_t> d_count;
    PinBuf<uint32_t> h_count;
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

// ---- MapStore -------------------------------------------------------------------------------------------------------------------
inline int MapStore::reserve(size_t cap) {
    if (cap <= capacity) return LV_OK;
    const size_t ncap = grown(capacity, 4096, cap);
    capacity = 0;
    const int rc = reserve_ids(ncap);
    if (!rc) capacity = ncap;
    refresh_view();   // (d_orig may have moved, whether the rest followed or not)
    return rc;
}
inline int MapStore::reserve_ids(size_t ncap) {
    // what is by id is kept: the points, and the box chains and the positions inside buckets and lists once they exist.  Another
    // stream may still be writing them (the insert's side stream): the whole device is waited for before each copy.
    if (d_orig.cap < ncap) LV_TRY(d_orig.grow_keep(ncap, n_ids, 0, nullptr, true));
    LV_TRY(need_all(ncap, d_orig2, d_sorted, d_keys, d_keys_sorted, d_idx, d_idx_sorted));
    size_t bytes = 0;
    LV_TRY(sort_pairs_scratch_u64(ncap, 63, &bytes));
    LV_TRY(d_sort_tmp.need(bytes));
    LV_TRY(d_dead.need(ncap));
    if (d_box_next.p && d_box_next.cap < ncap) LV_TRY(d_box_next.grow_keep(ncap, n_ids, 0, nullptr, true));
    if (d_cellpos.p) {
        for (int l = 0; l < BUCKET_LEVELS; ++l)
            if (d_backpos[l].cap < ncap * 27) LV_TRY(d_backpos[l].grow_keep(ncap * 27, (size_t)n_ids * 27, 0, nullptr, true));
        if (d_cellpos.cap < ncap) LV_TRY(d_cellpos.grow_keep(ncap, n_ids, 0, nullptr, true));
    }
    return LV_OK;
}

inline int MapStore::ensure_alive_scratch() {
    if (d_ascan_tmp.p && d_alive.cap >= capacity && d_apos.cap >= capacity) return LV_OK;   // (the scratch comes last: it is there only if the two are)
    LV_TRY(need_all(capacity, d_alive, d_apos));
    size_t bytes = 0;
    LV_TRY(exclusive_sum_scratch(capacity, &bytes));
    return d_ascan_tmp.resize(bytes);
}

inline int MapStore::ensure_counters() {
    if (d_cnt.p && h_cnt.p) return LV_OK;
    LV_TRY(d_cnt.need(BUCKET_LEVELS));
    LV_HIP(hipMemset(d_cnt.p, 0, BUCKET_LEVELS * sizeof(MapCounters)));
    LV_TRY(h_cnt.need(BUCKET_LEVELS));   // (last: the pair is there only once the device words are zero)
    std::memset(h_cnt.p, 0, BUCKET_LEVELS * sizeof(MapCounters));
    return LV_OK;
}

inline int MapStore::reserve_batch(size_t k) {
    if (k <= batch_cap) return LV_OK;
    const size_t ncap = grown(batch_cap, 4096, k);
    batch_cap = 0;
    gtab_size = reloc_cap = broken_cap = comp_cap = cstage_cap = 0;
    LV_TRY(need_all(ncap, d_new, d_nkeys, d_nkeys_sorted, d_nidx, d_nidx_sorted, d_nalive, d_napos, d_nsurv, d_nsflag, d_nspos));
    const uint32_t gtab = next_pow2((uint64_t)ncap * 4);
    for (int l = 0; l < BUCKET_LEVELS; ++l) {   // (per instance)
        LV_TRY(d_rank[l].need(ncap * 27 * SORTED_LEVELS));
        LV_TRY(need_all(ncap * REPL_LEVELS, d_prank[l], d_pslot[l]));
        LV_TRY(d_gtab[l].need(gtab));
        LV_TRY(need_all((size_t)gtab * GROUP_TARGETS, d_gbase[l], d_gslot[l], d_gdst[l]));
    }
    LV_TRY(d_gcnt.need(BUCKET_LEVELS * 4 * LIST_SHARDS));
    const uint32_t reloc = (uint32_t)(ncap * 27 > 0x0FFFFFF0ull ? 0x0FFFFFF0ull : ncap * 27);
    for (int l = 0; l < BUCKET_LEVELS; ++l) LV_TRY(d_reloc[l].need(reloc));
    // a batch of k points breaks up at most 27 k groups (one per target bucket), in practice a few per cent of k: more than this
    // raises `overflow` and the map is re-linearised
    const uint32_t broken = (uint32_t)(ncap * 2 < 16384 ? 16384 : ncap * 2);   // (sharded 64 ways by table slot: room for an uneven spread)
    LV_TRY(need_all(broken, d_broken, d_regroup));
    // runs compacted in place: the list (one entry per run) and the staging area (one entry per bucket entry of a listed run; a
    // run that finds it full moves instead)
    const uint32_t comp = reloc < (1u << 18) ? reloc : (1u << 18);
    const uint32_t cstage = (uint32_t)(ncap * 32 < (1u << 20) ? (1u << 20) : ncap * 32);
    for (int l = 0; l < BUCKET_LEVELS; ++l) {
        LV_TRY(d_comp[l].need(comp));
        LV_TRY(need_all(cstage, d_cstage[l], d_cnew[l]));
    }
    size_t a = 0, b = 0;
    LV_TRY(sort_pairs_scratch_u64(ncap, 63, &a));
    LV_TRY(exclusive_sum_scratch(ncap, &b));
    LV_TRY(d_ntmp.need(a > b ? a : b));
    gtab_size = gtab;
    reloc_cap = reloc;
    broken_cap = broken;
    comp_cap = comp;
    cstage_cap = cstage;
    batch_cap = ncap;
    return LV_OK;
}

inline int MapStore::reserve_boxes() {
    const uint32_t size = next_pow2((uint64_t)capacity * 4);
    if (size > box_size) {
        box_size = 0;
        LV_TRY(d_box.resize(size));
        box_size = size;
    }
    return d_box_next.need(capacity);
}

inline void MapStore::release() {
    release_all(d_orig, d_orig2, d_sorted, d_keys, d_keys_sorted, d_idx, d_idx_sorted, d_sort_tmp, d_counts, d_cellpos, d_biglist, d_gtable,
                d_gext, d_goff, d_broken, d_regroup, d_cell_slots, d_bcount, d_bcap, d_boff, d_flags, d_scan_tmp, d_caux, d_cell4, d_cnt,
                h_cnt, d_new, d_nkeys, d_nkeys_sorted, d_nidx, d_nidx_sorted, d_nalive, d_napos, d_nsurv, d_nsflag, d_nspos, d_ntmp, d_gcnt,
                d_dead, d_alive, d_apos, d_ascan_tmp, d_box, d_box_next);
    for (int l = 0; l < N_OCC; ++l) d_tables[l].release();
    for (int l = 0; l < BUCKET_LEVELS; ++l)
        release_all(d_btable[l], d_baux[l], d_bxyz[l], d_bidx[l], d_backpos[l], d_comp[l], d_cstage[l], d_cnew[l], d_rank[l], d_gtab[l],
                    d_prank[l], d_pslot[l], d_gbase[l], d_gslot[l], d_gdst[l], d_reloc[l]);
    note_free(notes);
    *this = MapStore();
}

// ---- ScanStore ------------------------------------------------------------------------------------------------------------------
inline int ScanStore::reserve(size_t cap) {
    if (cap <= capacity) return LV_OK;
    const size_t ncap = grown(capacity, 4096, cap);
    capacity = 0;
    LV_TRY(need_all(ncap, d_raw, d_sorted, d_keys, d_keys_sorted, d_idx, d_idx_sorted));
    size_t bytes = 0;
    LV_TRY(sort_pairs_scratch_u32(ncap, 30, &bytes));
    LV_TRY(d_sort_tmp.need(bytes));
    capacity = ncap;
    return LV_OK;
}

inline int ScanStore::reserve_raw(size_t cap, size_t n_states) {
    if (cap > raw_cap) {
        const size_t ncap = grown(raw_cap, 4096, cap);
        raw_cap = 0;
        LV_TRY(need_all(ncap, d_in, d_times, d_desk, d_vkeys, d_vkeys_sorted, d_vidx, d_vidx_sorted, d_heads, d_hpos));
        size_t bytes = 0;
        LV_TRY(sort_pairs_scratch_u64(ncap, 63, &bytes));
        LV_TRY(d_vsort_tmp.need(bytes));
        LV_TRY(exclusive_sum_scratch(ncap, &bytes));
        LV_TRY(d_vscan_tmp.need(bytes));
        raw_cap = ncap;
    }
    LV_TRY(d_states.need(n_states));
    return d_bounds.need(8);
}

inline int ScanStore::reserve_tiles(uint32_t nt) {
    return nt <= d_tile_order.cap ? LV_OK : d_tile_order.need_pow2(nt, 1024);
}

inline void ScanStore::release() {
    release_all(d_raw, d_sorted, d_keys, d_keys_sorted, d_idx, d_idx_sorted, d_sort_tmp, d_tile_order, d_in, d_times, d_desk, d_states, d_vkeys,
                d_vkeys_sorted, d_vidx, d_vidx_sorted, d_heads, d_hpos, d_bounds, d_vsort_tmp, d_vscan_tmp, d_tail_clk);
    note_free(notes);
    *this = ScanStore();
}

// ---- CloudStore -----------------------------------------------------------------------------------------------------------------
inline int CloudStore::init() {
    if (d_count.p && h_count.p && notes.d) return LV_OK;
    LV_TRY(need_all(4, d_count, h_count));
    const hipError_t e = note_alloc(notes);
    if (e != hipSuccess) note_free(notes);   // (a board without its device address is no board: the next call allocates again)
    LV_HIP(e);
    return LV_OK;
}

inline int CloudStore::reserve_msg(size_t n, size_t bytes) {
    if (bytes > raw_cap) {
        const size_t cap = grown(raw_cap, (size_t)1 << 20, bytes);
        raw_cap = 0;
        LV_HIP(hipDeviceSynchronize());   // (a staging buffer may still be in flight)
        LV_TRY(need_all(cap, d_rawmsg, h_rawmsg, h_rawmsg2));
        for (int b = 0; b < 2; ++b) {
            if (!ev_stage[b]) LV_HIP(hipEventCreateWithFlags(&ev_stage[b], hipEventDisableTiming));
            stage_busy[b] = false;
        }
        raw_cap = cap;
    }
    if (n > msg_cap) {
        const size_t cap = grown(msg_cap, 65536, n);
        msg_cap = 0;
        LV_TRY(need_all(cap, d_decoded, d_kept, d_keep, d_keys, d_keys_sorted, d_ids, d_ids_sorted));
        size_t a = 0, b = 0;
        LV_TRY(select_flagged_scratch(cap, &a));
        LV_TRY(sort_pairs_scratch_u64(cap, 64, &b));
        LV_TRY(d_tmp.need(a > b ? a : b));
        msg_cap = cap;
    }
    return LV_OK;
}

inline int CloudStore::reserve_buffer(hipStream_t stream, size_t total) {
    if (total <= d_buf.cap) return LV_OK;
    // Buffer::clear only advances `head`: before the buffer grows, the living range [head, size) moves to the front when it
    // fits there without overlapping itself (it does as soon as half of what was ever appended has been cleared) — the buffer of
    // a stream then stays at a few sweeps instead of doubling for ever (and reallocating, 0.3 ms, every time)
    const size_t live = size - head;
    if (head >= live && total - head <= d_buf.cap) {
        if (live) LV_HIP(hipMemcpyAsync(d_buf.p, d_buf.p + head, live * sizeof(CloudPoint), hipMemcpyDeviceToDevice, stream));
        size = (uint32_t)live;
        head = 0;
        return LV_OK;
    }
    LV_TRY(d_buf.grow_keep(grown(d_buf.cap, (size_t)1 << 18, total), size > head ? size - head : 0, head, stream, false));
    size -= head;
    head = 0;
    return LV_OK;
}

inline void CloudStore::release() {   // (no wait here: the callers have synchronised)
    release_all(d_buf, d_rawmsg, h_rawmsg, h_rawmsg2, d_decoded, d_kept, d_keep, d_keys, d_keys_sorted, d_ids, d_ids_sorted, d_tmp, d_count,
                h_count);
    for (int b = 0; b < 2; ++b)
        if (ev_stage[b]) hipEventDestroy(ev_stage[b]);
    note_free(notes);
    *this = CloudStore();
}

}  // namespace lv
