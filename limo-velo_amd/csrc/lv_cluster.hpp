// lv_cluster.hpp — Euclidean clustering of the device map and removal by cluster (lv_map_cluster / lv_map_remove_clusters,
// include/limovelo_hip.h "Map clustering"; kernels and host side in lv_cluster.hip).
//
// The first part is plain inline code that also compiles for the host (any compiler but hipcc, through tests/emu/hip/hip_runtime.h
// whose atomics are sequential: tests/test_cluster_host.py holds it to scipy's connected components): the lock-free union-find
// by minimum id, the key that orders the clusters and the rules that decide what is reported and what is removed.
// LV_CLUSTER_HOST_ONLY leaves it at that first part (no ClusterStore, no lv_host.hpp).
//
// Union-find over parent[n_ids]: an included living id starts as its own parent, everything else holds CL_NONE and is never
// touched.  A link always hangs the HIGHER root under the LOWER one, so a parent is smaller than its child (no cycle can form)
// and the root of a finished component is its smallest id — its first member in map order, since ids are monotone in map order.
// Every value parent[x] ever held is a member of x's component no larger than x.  That makes a stale read harmless (it shows an
// ancestor of an earlier tree) and makes the one write that decides, the compare-and-swap on a root, self-checking: it succeeds
// only while the node still is a root, and on failure hands back the parent to go on from.  Nothing here waits for a value
// another lane has to write.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>
#if defined(__HIPCC__)
#define LV_CL_D __device__ __forceinline__
#define LV_CL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LV_CL_D inline
#define LV_CL_HD inline
#endif

namespace lv {

constexpr uint32_t CL_NONE = 0xFFFFFFFFu;   // parent of an id that takes no part (dead or excluded); the root of a lane without a hit

// parent[] is read and written by every wavefront of the link kernel: relaxed accesses at device scope, so a value is never
// served from a cache another compute die does not see
LV_CL_D uint32_t cl_load(const uint32_t* p) {
#if !defined(__HIPCC__)
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
LV_CL_D void cl_store(uint32_t* p, uint32_t v) {
#if !defined(__HIPCC__)
    *p = v;
#else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// the root of x's tree as far as this lane can see; halves the path on the way (parent[x] = parent[parent[x]]: an ancestor for an
// ancestor, whichever store of two racing lanes lands last)
LV_CL_D uint32_t cl_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cl_load(parent + x);
        if (p == x) return x;
        const uint32_t g = cl_load(parent + p);
        if (g == p) return p;
        cl_store(parent + x, g);
        x = g;
    }
}
// the same without a store (the flatten pass: every lane writes its own result elsewhere)
LV_CL_D uint32_t cl_root(const uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cl_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// joins the trees of a and b.  The compare-and-swap succeeds only on a node that is still a root; when it fails, the node has
// been linked by someone else meanwhile and the value returned is where to go on: every round either ends or moves to a
// strictly smaller id, so the loop is bounded without ever waiting.
LV_CL_D void cl_link(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// Clusters are numbered by ascending key: size descending, then the smaller root (= first member in map order) first
LV_CL_HD uint64_t cl_order_key(uint32_t size, uint32_t root) { return ((uint64_t)(~size) << 32) | (uint64_t)root; }
LV_CL_HD uint32_t cl_key_size(uint64_t key) { return ~(uint32_t)(key >> 32); }
LV_CL_HD uint32_t cl_key_root(uint64_t key) { return (uint32_t)key; }
// a component of `size` points is reported by lv_map_cluster (max_size 0: no upper limit)
LV_CL_HD bool cl_reported(uint32_t size, uint32_t min_size, uint32_t max_size) {
    return size >= min_size && (max_size == 0 || size <= max_size);
}
// a component leaves the map (lv_map_remove_clusters).  Debris (no seeds): fewer than min_size points, max_size ignored.
// Object growth (seeds): a reported size and at least one seeded member.
LV_CL_HD bool cl_removed(uint32_t size, uint32_t min_size, uint32_t max_size, bool seeded_mode, bool has_seed) {
    return seeded_mode ? (has_seed && cl_reported(size, min_size, max_size)) : size < min_size;
}

}  // namespace lv

#if !defined(LV_CLUSTER_HOST_ONLY)
#include "lv_host.hpp"
#include "lv_rules.hpp"   // ClusterRule

namespace lv {

// The buffers of lv_map_cluster / lv_map_remove_clusters (grown on demand, kept)
struct ClusterStore {
    DevBuf<uint32_t> d_parent;      // by id: the union-find, then (flattened) every included id's root
    DevBuf<uint32_t> d_size;        // by id: at a root, the size of its component
    DevBuf<int32_t> d_lab;          // by id: at a root, its cluster's label or -1; removal: 1 at a root whose component holds a seed
    DevBuf<uint32_t> d_flag;        // by id: 1 at a reported root; d_pos: its exclusive scan (n_ids + 1: the last entry is C)
    DevBuf<uint32_t> d_pos;
    DevBuf<uint64_t> d_key;         // the reported roots' order keys, and their sorted copy
    DevBuf<uint64_t> d_key2;
    DevBuf<int32_t> d_labels;       // outputs at living ranks
    DevBuf<uint32_t> d_sizes;       // sizes in cluster order
    DevBuf<uint8_t> d_mask;         // the caller's mask / seeds / the flags returned, at living ranks
    DevBuf<uint8_t> d_seeds;
    DevBuf<uint8_t> d_flags;
    DevBuf<void> d_tmp;             // hipcub scratch
    PinBuf<uint32_t> h_word;        // C read back by the host
    int ensure(size_t n_ids, size_t m);
    void release();
};

// The components of `map` under `q` (mask: device, m bytes at living ranks, or NULL): on return of the enqueued work d_parent
// holds every included id's root and d_size every root's size.  rank: QueryStore::ensure_rank's (NULL: ranks are ids).
int cluster_components(const MapStore& map, hipStream_t stream, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, const uint8_t* mask);
// after cluster_components: the canonical labels at living ranks in st.d_labels (want_labels), the sizes in cluster order in
// st.d_sizes, *n_clusters = C.  Synchronises.
int cluster_labels(const MapStore& map, hipStream_t stream, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, bool want_labels,
                   size_t* n_clusters);
// after cluster_components: the components the rule removes; flags (device, may be NULL) at the living ranks; remove: their points
// leave the map (its dead list, MapStore::kill_dead_list).  seeds: device, m bytes at living ranks (q.seeded).  Synchronises.
int cluster_remove(MapStore& map, hipStream_t stream, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, const uint8_t* seeds,
                   uint8_t* flags, bool remove, uint32_t* n_removed);

}  // namespace lv
#endif
