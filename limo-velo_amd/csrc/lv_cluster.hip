// lv_cluster.hip — lv_map_cluster / lv_map_remove_clusters: the connected components of the map's own fixed-radius graph, found
// where the points lie (include/limovelo_hip.h "Map clustering"; the union-find and the rules: lv_cluster.hpp).
//
//   cluster_init_kernel      one lane per id: parent = id for an included living id, CL_NONE otherwise; sizes 0, labels -1.
//   cluster_link_kernel      one wavefront per included id i walks the fixed-radius source of the query (p_i, radius)
//                            (radius_source / stream_radius, lv_query_dev.hpp): the level-0 run while the radius is inside the
//                            level-0 bound, else the level-2 lists covering [p - r, p + r], else every id.  A hit j counts only
//                            if j < i (every edge is taken once, from its higher end) and j is included.  Per chunk of 64
//                            candidates every hitting lane finds its root, the wavefront takes the minimum over those and i's
//                            own root, and the lanes whose root is another one link it to that minimum (cl_link: compare-and-swap
//                            on a root, retry from what it returns; two lanes with the same root cost one failed swap).  In a dense
//                            map most of the 10-30 hits of a point already share its root and nothing is written at all.
//                            No lane ever waits for a value another lane writes.
//   cluster_flatten_kernel   one lane per id: parent = the root, the root's size + 1 (one atomic per wavefront where all its lanes
//                            share a root, which is the common case in a large cluster).
//   labels                   flag the reported roots, scan, scatter their keys (~size << 32 | root), sort (hipcub radix sort), give
//                            every sorted root its position as label, scatter the labels to the living ranks.
//   removal                  cluster_seed_kernel marks the roots of seeded points; cluster_classify_kernel flags the members of the
//                            components the rule removes and appends them to the map's dead list (dead_list_append,
//                            lv_query_dev.hpp), retired by MapStore::retire_dead_list.
// The partition is a pure function of the living points, the mask and the radius: the order in which links land changes the
// trees on the way, never the components, and a finished root is always its component's smallest id.
#include "lv_cluster.hpp"

#include "lv_query_dev.hpp"

#include <hipcub/hipcub.hpp>

#include <cstring>

namespace lv {

namespace {

constexpr int CWAVES = 4;   // wavefronts (points) per workgroup
constexpr int CTHREADS = CWAVES * 64;

__global__ __launch_bounds__(256) void cluster_init_kernel(const float4* __restrict__ orig, uint32_t n_ids, const uint32_t* __restrict__ rank,
                                                           const uint8_t* __restrict__ mask, uint32_t* __restrict__ parent,
                                                           uint32_t* __restrict__ size, int32_t* __restrict__ lab) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const bool in = pt_alive(orig[id]) && (!mask || mask[rank_of(rank, id)] != 0);
    parent[id] = in ? id : CL_NONE;
    size[id] = 0u;
    lab[id] = -1;
}

__global__ __launch_bounds__(CTHREADS) void cluster_link_kernel(MapView map, float radius, uint32_t* parent) {
    __shared__ uint32_t s_pref[CWAVES][64], s_start[CWAVES][64];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const uint32_t id = blockIdx.x * (uint32_t)CWAVES + (uint32_t)w;
    if (id >= map.n_ids) return;                     // (wavefront-uniform, as the two below)
    if (id == 0u) return;                            // no smaller id to link to
    if (cl_load(parent + id) == CL_NONE) return;     // dead or excluded: links nothing
    const float4 P = map.orig[id];
    const float qx = P.x, qy = P.y, qz = P.z;
    const float max_d2 = radius * radius;
    uint32_t mine = id;   // a member of id's tree at or above id, the same in every lane
    auto visit = [&](float x, float y, float z, uint32_t cid, bool ok) {
        const float d = calc_dist(qx, qy, qz, Xyz{x, y, z});
        const bool hit = ok && admitted(d, max_d2) && cid < id;
        if (__ballot(hit) == 0ull) return;
        uint32_t r = CL_NONE;   // the root of this lane's hit, if it is an included point
        if (hit && cl_load(parent + cid) != CL_NONE) r = cl_find(parent, cid);
        const uint32_t own = lane == 0 ? cl_find(parent, mine) : CL_NONE;
        uint32_t m = min(r, own);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, off));
        if (r != CL_NONE && r != m) cl_link(parent, r, m);
        if (own != CL_NONE && own != m) cl_link(parent, own, m);
        mine = m;
    };
    const QGeom geo = make_geom(map, qx, qy, qz);
    stream_radius(map, radius_source(map, geo, qx, qy, qz, radius), geo, lane, s_pref[w], s_start[w], visit);
}

__global__ __launch_bounds__(256) void cluster_flatten_kernel(uint32_t n_ids, uint32_t* parent, uint32_t* __restrict__ size) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t root = CL_NONE;
    if (id < n_ids && cl_load(parent + id) != CL_NONE) {
        root = cl_root(parent, id);
        cl_store(parent + id, root);   // (an ancestor for an ancestor: lanes still walking through id lose nothing)
    }
    const unsigned long long in = __ballot(root != CL_NONE);
    if (in == 0ull) return;
    const int leader = __ffsll((long long)in) - 1;
    const uint32_t first = (uint32_t)__shfl((int)root, leader);
    if (__ballot(root != CL_NONE && root != first) == 0ull) {
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(size + first, (uint32_t)__popcll(in));
    } else if (root != CL_NONE) {
        atomicAdd(size + root, 1u);
    }
}

__global__ __launch_bounds__(256) void cluster_flag_kernel(uint32_t n_ids, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                           ClusterRule q, uint32_t* __restrict__ flag) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n_ids) flag[id] = (parent[id] == id && cl_reported(size[id], q.min_size, q.max_size)) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void cluster_key_kernel(uint32_t n_ids, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                          const uint32_t* __restrict__ size, uint64_t* __restrict__ key) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n_ids && flag[id]) key[pos[id]] = cl_order_key(size[id], id);
}
__global__ __launch_bounds__(256) void cluster_number_kernel(const uint64_t* __restrict__ sorted, uint32_t n, int32_t* __restrict__ lab,
                                                             uint32_t* __restrict__ sizes) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t k = sorted[j];
    lab[cl_key_root(k)] = (int32_t)j;
    sizes[j] = cl_key_size(k);
}
__global__ __launch_bounds__(256) void cluster_scatter_kernel(const float4* __restrict__ orig, uint32_t n_ids, const uint32_t* __restrict__ rank,
                                                              const uint32_t* __restrict__ parent, const int32_t* __restrict__ lab,
                                                              int32_t* __restrict__ labels) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids || !pt_alive(orig[id])) return;
    const uint32_t root = parent[id];
    labels[rank_of(rank, id)] = root == CL_NONE ? -1 : lab[root];
}

// lab[root] = 1 where the component holds a seeded included point (every writer stores the same value)
__global__ __launch_bounds__(256) void cluster_seed_kernel(uint32_t n_ids, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ parent,
                                                           const uint8_t* __restrict__ seeds, int32_t* __restrict__ lab) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const uint32_t root = parent[id];
    if (root != CL_NONE && seeds[rank_of(rank, id)] != 0) lab[root] = 1;
}

// One lane per id: flags (optional) at the point's rank; remove: the members of the removed components go to the dead list
// (x, y, z, id) and read x = +inf from here on.
__global__ __launch_bounds__(256) void cluster_classify_kernel(float4* __restrict__ orig, uint32_t n_ids, const uint32_t* __restrict__ rank,
                                                               const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size,
                                                               const int32_t* __restrict__ lab, ClusterRule q, uint8_t* __restrict__ flags,
                                                               int remove, float4* __restrict__ dead, uint32_t dead_cap, MapCounters* cnt) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool gone = false;
    if (id < n_ids) p = orig[id];
    if (id < n_ids && pt_alive(p)) {
        const uint32_t root = parent[id];
        const bool out = root != CL_NONE && cl_removed(size[root], q.min_size, q.max_size, q.seeded != 0, lab[root] == 1);
        if (flags) flags[rank_of(rank, id)] = out ? 1 : 0;
        gone = remove && out;
    }
    dead_list_append(gone, p, id, orig, dead, dead_cap, cnt);
}

}  // namespace

int ClusterStore::ensure(size_t n_ids, size_t m) {
    int rc = d_parent.need(n_ids);
    if (!rc) rc = d_size.need(n_ids);
    if (!rc) rc = d_lab.need(n_ids);
    if (!rc) rc = d_flag.need(n_ids);
    if (!rc) rc = d_pos.need(n_ids + 1);
    if (!rc) rc = d_labels.need(m);
    if (!rc) rc = d_mask.need(m);
    if (!rc) rc = d_seeds.need(m);
    if (!rc) rc = d_flags.need(m);
    if (!rc) rc = h_word.need(4);
    return rc;
}

void ClusterStore::release() {
    d_parent.release(); d_size.release(); d_lab.release(); d_flag.release(); d_pos.release(); d_key.release(); d_key2.release();
    d_labels.release(); d_sizes.release(); d_mask.release(); d_seeds.release(); d_flags.release(); d_tmp.release(); h_word.release();
}

int cluster_components(const MapStore& map, hipStream_t stream, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, const uint8_t* mask) {
    const MapView v = map.view;
    if (map.n_ids == 0) return LV_OK;
    // (one wavefront per id: a launch takes fewer than 2^32 threads)
    if (map.n_ids > 0x03FFFFF0u) { set_error("map of %u ids: clustering takes at most %u", map.n_ids, 0x03FFFFF0u); return LV_EINVAL; }
    const uint32_t ids = map.n_ids;
    hipLaunchKernelGGL(cluster_init_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, rank, mask, st.d_parent, st.d_size, st.d_lab);
    LV_HIP(hipGetLastError());
    hipLaunchKernelGGL(cluster_link_kernel, dim3(blocks_of(ids, CWAVES)), dim3(CTHREADS), 0, stream, v, q.radius, st.d_parent);
    LV_HIP(hipGetLastError());
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, ids, st.d_parent, st.d_size);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int cluster_labels(const MapStore& map, hipStream_t stream, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, bool want_labels,
                   size_t* n_clusters) {
    *n_clusters = 0;
    const uint32_t ids = map.n_ids;
    if (ids == 0) return LV_OK;
    hipLaunchKernelGGL(cluster_flag_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, ids, st.d_parent, st.d_size, q, st.d_flag);
    LV_HIP(hipGetLastError());
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, st.d_flag.p, st.d_pos.p, (int)ids, stream));
    int rc = st.d_tmp.need(bytes ? bytes : 1);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(st.d_tmp.p, bytes, st.d_flag.p, st.d_pos.p, (int)ids, stream));
    hipLaunchKernelGGL(scan_total_kernel<uint32_t>, dim3(1), dim3(64), 0, stream, st.d_pos, st.d_flag, ids, st.d_pos + ids);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(st.h_word, st.d_pos + ids, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    const uint32_t C = st.h_word[0];
    *n_clusters = C;
    if (C) {
        rc = st.d_key.need(C);
        if (!rc) rc = st.d_key2.need(C);
        if (!rc) rc = st.d_sizes.need(C);
        if (rc) return rc;
        hipLaunchKernelGGL(cluster_key_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, ids, st.d_flag, st.d_pos, st.d_size, st.d_key);
        LV_HIP(hipGetLastError());
        bytes = 0;
        LV_HIP((hipError_t)hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, st.d_key.p, st.d_key2.p, (int)C, 0, 64, stream));
        rc = st.d_tmp.need(bytes ? bytes : 1);
        if (rc) return rc;
        LV_HIP((hipError_t)hipcub::DeviceRadixSort::SortKeys(st.d_tmp.p, bytes, st.d_key.p, st.d_key2.p, (int)C, 0, 64, stream));
        hipLaunchKernelGGL(cluster_number_kernel, dim3(blocks_of(C, 256)), dim3(256), 0, stream, st.d_key2, C, st.d_lab, st.d_sizes);
        LV_HIP(hipGetLastError());
    }
    if (want_labels) {
        hipLaunchKernelGGL(cluster_scatter_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, rank, st.d_parent, st.d_lab, st.d_labels);
        LV_HIP(hipGetLastError());
    }
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int cluster_remove(MapStore& map, hipStream_t stream, ClusterStore& st, const ClusterRule& q, const uint32_t* rank, const uint8_t* seeds,
                   uint8_t* flags, bool remove, uint32_t* n_removed) {
    if (n_removed) *n_removed = 0;
    const uint32_t ids = map.n_ids;
    if (!map.built || map.m == 0 || ids == 0) return LV_OK;
    if (q.seeded) {
        hipLaunchKernelGGL(cluster_seed_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, ids, rank, st.d_parent, seeds, st.d_lab);
        LV_HIP(hipGetLastError());
    }
    int rc = map.ensure_counters();
    if (rc) return rc;
    rc = map.reset_batch_counters(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(cluster_classify_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, rank, st.d_parent, st.d_size, st.d_lab, q,
                       flags, remove ? 1 : 0, map.d_dead, (uint32_t)map.d_dead.cap, map.d_cnt);
    LV_HIP(hipGetLastError());
    if (!remove) {
        LV_HIP(hipStreamSynchronize(stream));
        return LV_OK;
    }
    return map.retire_dead_list(stream, n_removed);
}

}  // namespace lv
