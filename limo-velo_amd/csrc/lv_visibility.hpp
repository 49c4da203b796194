// lv_visibility.hpp — free-space removal of dynamic points (lv_map_remove_dynamic, include/limovelo_hip.h "Dynamic-point
// removal"; kernels and host side in lv_visibility.hip).
#pragma once
#include "lv_host.hpp"
#include "lv_rules.hpp"   // VIS_MAX_*, VisRule

namespace lv {

// Bytes of the device blob a call classifies against: the views' poses (12 floats each: R row-major, t), padded to 256 B, then
// the n_views window-min images (height x width f32 each).  The background rebuild journals exactly this blob.
inline size_t vis_pose_bytes(int n_views) { return (((size_t)n_views * 12 * sizeof(float)) + 255) & ~(size_t)255; }
inline size_t vis_blob_bytes(const VisRule& q) { return vis_pose_bytes(q.n_views) + (size_t)q.n_views * q.width * q.height * sizeof(float); }

// Classification of every living point of `map` against the blob, on `stream`.  rank: NULL (ranks are ids) or the rank among
// the living by id (QueryStore::ensure_rank); hits: NULL or a device array of map.m counts, written at the ranks.  remove: the
// points seen through in >= min_hits views leave the map (its dead list, then MapStore::kill_dead_list, as evict_oldest).
// Synchronises the stream.  Shared by lv_map_remove_dynamic and the background rebuild's replay of it.
int vis_classify(MapStore& map, hipStream_t stream, const void* d_blob, const VisRule& q, const uint32_t* rank, uint8_t* hits,
                 bool remove, uint32_t* n_removed);

// The buffers of lv_map_remove_dynamic (grown on demand, kept): staged returns, the blob and the filter's intermediate image,
// the hit counts.
struct VisStore {
    PinBuf<float4> h_pts;        // the returns of every view, w = the view's index
    DevBuf<float4> d_pts;
    DevBuf<void> d_blob;
    DevBuf<float> d_tmp;
    DevBuf<uint8_t> d_hits;
    // the blob of the call (poses + window-min images) from the views, on `stream`
    int build(hipStream_t stream, const lv_view* views, size_t n_views, const VisRule& q);
    int ensure_hits(size_t n);
    void release();
};

}  // namespace lv
