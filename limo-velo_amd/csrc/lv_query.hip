// lv_query.hip — map queries: batched k-NN, radius and box searches of arbitrary map-frame points against the device map
// (ikd-Tree's Nearest_Search / Radius_Search / Box_Search, which the update's own search does not expose).
//
// k-NN (query_knn_kernel): ONE wavefront per query walks the ladder of the update's search (lv_match.hip), written
// once as knn_ladder (lv_query_dev.hpp) —
//   level 0  the query voxel's neighbourhood bucket (one contiguous id-sorted run of 12-byte points),
//   level 1  the region of its tile group while the group is in one piece (extent > 0),
//   level 2  the 27 level-2 voxel lists around it,
//   level 3  the 216 lists that tile the level-3 block,
//   finally  every id,
// with the acceptance rule generalised from 5 to k and to a caller's max_dist: level l is accepted iff
//   (k admitted candidates and d_k < r_l^2)  or  max_dist^2 < r_l^2  (every admissible point lies inside the block),
// otherwise the next level is searched from scratch.  Keys are (d2 bits << 32 | id) handled as f64 (lv_search_dev.hpp: one
// v_min_f64 / v_max_f64 pair is a compare-exchange), so key order is the oracle's (distance, index) order, ties included.  The
// running top-k is one key per lane, ascending over the lanes (k <= 32 < 64): a chunk of 64 candidates (one per lane) that holds
// no key below the k-th is skipped by one ballot; otherwise it is sorted by a 21-step bitonic network over __shfl_xor, merged
// by min(top[i], chunk[63 - i]) (the 64 smallest of the union, bitonic) and cleaned up by 6 bitonic steps.  No LDS except the
// 2 x 64 words of list offsets a wavefront needs on the list levels.
//
// Radius: a count kernel and a fill kernel walk the same source per query (radius_source / stream_radius, lv_query_dev.hpp) — the
// level-0 run if the radius is inside the level-0 radius bound, else the level-2 lists covering [q - r, q + r] (one list of margin
// per side), else (more lists than ids, or outside the voxel range) every id — with an exclusive scan of the counts in between; the
// segments are then sorted by id (hipcub segmented radix sort).
// Box: one pass over the ids with inc_evict_box_kernel's predicate, a scan, a scatter in id order.
// Results carry ids until the end; the rank among the living comes from a device scan of the alive flags (QueryStore::ensure_rank),
// rebuilt only when the map's stamp (MapStore::gen) moved and skipped when no id is dead.
#include "lv_query_dev.hpp"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

namespace lv {

namespace {

constexpr int QWAVES = 4;                          // wavefronts (queries) per workgroup
constexpr int QTHREADS = QWAVES * 64;
constexpr uint32_t NO_IDX = 0xFFFFFFFFu;
// hipcub counts the items of a scan / sort in an int: the largest query batch, id range or result set handed to one
constexpr int SCAN_MAX = 0x7FFFFFFF;

__global__ __launch_bounds__(QTHREADS) void query_knn_kernel(MapView map, const float* __restrict__ q, uint32_t n, int k, float max_d2,
                                                             const uint32_t* __restrict__ rank, uint32_t* __restrict__ idx,
                                                             float* __restrict__ d2, int32_t* __restrict__ found) {
    __shared__ uint32_t s_pref[QWAVES][64], s_start[QWAVES][64];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.x * (uint32_t)QWAVES + (uint32_t)w;
    if (qi >= n) return;   // (wavefront-uniform)
    const float qx = q[3 * (size_t)qi], qy = q[3 * (size_t)qi + 1], qz = q[3 * (size_t)qi + 2];
    TopK t;
    t.k = k;
    t.reset();
    const bool finite = __builtin_isfinite(qx) && __builtin_isfinite(qy) && __builtin_isfinite(qz);
    if (map.m != 0 && finite) {
        auto visit = [&](float x, float y, float z, uint32_t id, bool ok) {
            const float d = calc_dist(qx, qy, qz, Xyz{x, y, z});
            t.offer(ok && admitted(d, max_d2) ? make_key(d, id) : none_key(), lane);
        };
        const QGeom geo = make_geom(map, qx, qy, qz);
        knn_ladder(map, geo, t, max_d2, lane, s_pref[w], s_start[w], visit);
    }
    const bool real = !is_none(t.top) && lane < k;
    if (lane < k) {
        idx[(size_t)qi * k + lane] = real ? rank_of(rank, key_lo(t.top)) : NO_IDX;
        if (d2) d2[(size_t)qi * k + lane] = real ? __uint_as_float(key_hi(t.top)) : __uint_as_float(0x7F800000u);
    }
    const int nf = __popcll(__ballot(real));
    if (found && lane == 0) found[qi] = nf;
}

// radius search of one query (one wavefront); FILL = false: count, true: write the ids / distances from out_off on
template <bool FILL>
__global__ __launch_bounds__(QTHREADS) void query_radius_kernel(MapView map, const float* __restrict__ q, uint32_t n, float radius,
                                                                uint64_t* __restrict__ counts, const uint64_t* __restrict__ off,
                                                                uint32_t* __restrict__ out_id, float* __restrict__ out_d2) {
    __shared__ uint32_t s_pref[QWAVES][64], s_start[QWAVES][64];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.x * (uint32_t)QWAVES + (uint32_t)w;
    if (qi >= n) return;
    const float qx = q[3 * (size_t)qi], qy = q[3 * (size_t)qi + 1], qz = q[3 * (size_t)qi + 2];
    const float r2 = radius * radius;
    uint32_t got = 0;
    // (64-bit offsets: a call's total may pass 2^32 even though one query finds at most n_ids points)
    const uint64_t base = FILL ? off[qi] : 0ull, room = FILL ? off[qi + 1] - off[qi] : 0ull;
    const uint64_t below = (1ull << lane) - 1ull;
    auto visit = [&](float x, float y, float z, uint32_t id, bool ok) {
        const float d = calc_dist(qx, qy, qz, Xyz{x, y, z});
        const bool hit = ok && admitted(d, r2);
        const unsigned long long b = __ballot(hit);
        if (FILL && hit) {
            const uint32_t p = got + (uint32_t)__popcll(b & below);
            if (p < room) {
                out_id[base + p] = id;
                out_d2[base + p] = d;
            }
        }
        got += (uint32_t)__popcll(b);
    };
    const bool finite = __builtin_isfinite(qx) && __builtin_isfinite(qy) && __builtin_isfinite(qz);
    if (map.m != 0 && finite) {
        const QGeom geo = make_geom(map, qx, qy, qz);
        stream_radius(map, radius_source(map, geo, qx, qy, qz, radius), geo, lane, s_pref[w], s_start[w], visit);
    }
    if (!FILL && lane == 0) counts[qi] = got;
}

__global__ void query_alive_kernel(const float4* __restrict__ orig, uint32_t n_ids, uint32_t* __restrict__ flag) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n_ids) flag[id] = pt_alive(orig[id]) ? 1u : 0u;
}
// inc_evict_box_kernel's predicate (lv_mapinc.hpp): living and inside [lo, hi], both faces inclusive
__global__ void query_box_flag_kernel(const float4* __restrict__ orig, uint32_t n_ids, float lx, float ly, float lz, float hx, float hy, float hz,
                                      uint32_t* __restrict__ flag) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const float4 p = orig[id];
    const bool inside = p.x >= lx && p.x <= hx && p.y >= ly && p.y <= hy && p.z >= lz && p.z <= hz;
    flag[id] = (pt_alive(p) && inside) ? 1u : 0u;
}
__global__ void query_box_scatter_kernel(const float4* __restrict__ orig, uint32_t n_ids, const uint32_t* __restrict__ flag,
                                         const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rank, uint32_t* __restrict__ out_idx,
                                         float* __restrict__ out_xyz) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids || !flag[id]) return;
    const uint32_t p = pos[id];
    const float4 v = orig[id];
    out_idx[p] = rank_of(rank, id);
    out_xyz[3 * (size_t)p] = v.x;
    out_xyz[3 * (size_t)p + 1] = v.y;
    out_xyz[3 * (size_t)p + 2] = v.z;
}
__global__ void query_remap_kernel(uint32_t* __restrict__ v, uint32_t n, const uint32_t* __restrict__ rank) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = rank[v[i]];
}

// the query buffers follow the caller's batch from call to call: they double from these floors (DESIGN "Host-side buffers")
constexpr size_t QUERY_FLOOR = 1024, QUERY_TMP_FLOOR = 4096;

}  // namespace

int QueryStore::stage_queries(hipStream_t stream, const void* q, size_t stride, size_t n) {
    const int rc = pts.reserve(stream, n, QUERY_FLOOR);
    if (rc) return rc;
    pts.append(q, stride, n);
    return pts.upload(stream);
}

int QueryStore::ensure_rank(const MapStore& map, hipStream_t stream, const uint32_t** rank) {
    *rank = nullptr;
    if (map.n_ids == map.m) return LV_OK;   // no dead id: ranks are ids
    if (map.n_ids > (uint32_t)SCAN_MAX) { set_error("map of %u ids: the rank scan takes at most %d", map.n_ids, SCAN_MAX); return LV_EINVAL; }
    if (rank_gen == map.gen && d_rank) { *rank = d_rank; return LV_OK; }
    int rc = d_rank.need_pow2(map.n_ids, QUERY_FLOOR);
    if (rc) return rc;
    rc = d_flag.need_pow2(map.n_ids, QUERY_FLOOR);
    if (rc) return rc;
    hipLaunchKernelGGL(query_alive_kernel, dim3(blocks_of(map.n_ids, 256)), dim3(256), 0, stream, map.d_orig, map.n_ids, d_flag);
    LV_HIP(hipGetLastError());
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_flag.p, d_rank.p, (int)map.n_ids, stream));
    rc = d_tmp.need_pow2(bytes, QUERY_TMP_FLOOR);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(d_tmp.p, bytes, d_flag.p, d_rank.p, (int)map.n_ids, stream));
    rank_gen = map.gen;
    *rank = d_rank;
    return LV_OK;
}

int QueryStore::knn(const MapStore& map, hipStream_t stream, const void* q, size_t stride, size_t n, int k, float max_dist, uint32_t* idx,
                    float* d2, int32_t* found) {
    if (k < 1 || k > 32) { set_error("k = %d: must be in 1..32", k); return LV_EINVAL; }
    if (!(max_dist >= 0.f)) { set_error("max_dist must be >= 0 (a negative or NaN max_dist)"); return LV_EINVAL; }
    if (n && (!q || stride < 12 || !idx)) { set_error("bad query array (stride %zu) or null result", stride); return LV_EINVAL; }
    if (n > 0xFFFFFFF0ull / 32) { set_error("too many queries"); return LV_EINVAL; }
    if (n == 0) return LV_OK;
    int rc = stage_queries(stream, q, stride, n);
    if (!rc) rc = d_idx.need_pow2(n * (size_t)k, QUERY_FLOOR);
    if (!rc) rc = d_d2.need_pow2(n * (size_t)k, QUERY_FLOOR);
    if (!rc) rc = d_found.need_pow2(n, QUERY_FLOOR);
    const uint32_t* rank = nullptr;
    if (!rc) rc = ensure_rank(map, stream, &rank);
    if (rc) return rc;
    const float max_d2 = max_dist * max_dist;
    hipLaunchKernelGGL(query_knn_kernel, dim3(blocks_of(n, QWAVES)), dim3(QTHREADS), 0, stream, map.view, pts.d, (uint32_t)n, k, max_d2, rank, d_idx,
                       d_d2, d_found);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(idx, d_idx, n * k * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (d2) LV_HIP(hipMemcpyAsync(d2, d_d2, n * k * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (found) LV_HIP(hipMemcpyAsync(found, d_found, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int QueryStore::radius(const MapStore& map, hipStream_t stream, const void* q, size_t stride, size_t n, float radius, size_t* offsets,
                       uint32_t* idx, float* d2, size_t capacity, size_t* total) {
    if (!(radius >= 0.f)) { set_error("radius must be >= 0 (a negative or NaN radius)"); return LV_EINVAL; }
    if (!offsets || !total || (n && (!q || stride < 12))) { set_error("bad query array (stride %zu) or null offsets / total", stride); return LV_EINVAL; }
    if (n >= (size_t)SCAN_MAX) { set_error("%zu queries: a radius search takes fewer than %d", n, SCAN_MAX); return LV_EINVAL; }
    *total = 0;
    offsets[0] = 0;
    if (n == 0) return LV_OK;
    int rc = stage_queries(stream, q, stride, n);
    if (!rc) rc = d_roff.need_pow2(n + 1, QUERY_FLOOR);
    if (!rc) rc = d_rcnt.need_pow2(n, QUERY_FLOOR);
    if (rc) return rc;
    const MapView v = map.view;
    hipLaunchKernelGGL(query_radius_kernel<false>, dim3(blocks_of(n, QWAVES)), dim3(QTHREADS), 0, stream, v, pts.d, (uint32_t)n, radius, d_rcnt,
                       (const uint64_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
    LV_HIP(hipGetLastError());
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_rcnt.p, d_roff.p, (int)n, stream));
    rc = d_tmp.need_pow2(bytes, QUERY_TMP_FLOOR);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(d_tmp.p, bytes, d_rcnt.p, d_roff.p, (int)n, stream));
    hipLaunchKernelGGL(scan_total_kernel<uint64_t>, dim3(1), dim3(64), 0, stream, d_roff, d_rcnt, (uint32_t)n, d_roff + n);
    LV_HIP(hipGetLastError());
    static_assert(sizeof(size_t) == sizeof(uint64_t), "offsets are copied out as size_t");
    LV_HIP(hipMemcpyAsync(offsets, d_roff, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    const size_t tot = offsets[n];
    *total = tot;
    if (!idx) return LV_OK;   // count only: any total
    if (capacity < tot) { set_error("capacity %zu < %zu results", capacity, tot); return LV_EINVAL; }
    // the fill's segmented sort counts its items in an int: a larger result set is refused before anything is allocated or written
    if (tot > (size_t)SCAN_MAX) {
        set_error("%zu results: one radius search returns at most %d (split the queries; the count-only call has no limit)", tot, SCAN_MAX);
        return LV_EINVAL;
    }
    if (tot == 0) return LV_OK;
    rc = d_idx.need_pow2(tot, QUERY_FLOOR);
    if (!rc) rc = d_d2.need_pow2(tot, QUERY_FLOOR);
    if (!rc) rc = d_idx2.need_pow2(tot, QUERY_FLOOR);
    if (!rc) rc = d_d22.need_pow2(tot, QUERY_FLOOR);
    const uint32_t* rank = nullptr;
    if (!rc) rc = ensure_rank(map, stream, &rank);
    if (rc) return rc;
    hipLaunchKernelGGL(query_radius_kernel<true>, dim3(blocks_of(n, QWAVES)), dim3(QTHREADS), 0, stream, v, pts.d, (uint32_t)n, radius,
                       (uint64_t*)nullptr, (const uint64_t*)d_roff, d_idx, d_d2);
    LV_HIP(hipGetLastError());
    // the lists are unordered: every query's segment by id
    bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, d_idx.p, d_idx2.p, d_d2.p, d_d22.p, (int)tot, (int)n, d_roff.p, d_roff.p + 1, 0,
                                                                   32, stream));
    rc = d_tmp.need_pow2(bytes, QUERY_TMP_FLOOR);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceSegmentedRadixSort::SortPairs(d_tmp.p, bytes, d_idx.p, d_idx2.p, d_d2.p, d_d22.p, (int)tot, (int)n, d_roff.p, d_roff.p + 1, 0,
                                                                   32, stream));
    if (rank) {
        hipLaunchKernelGGL(query_remap_kernel, dim3(blocks_of(tot, 256)), dim3(256), 0, stream, d_idx2, (uint32_t)tot, rank);
        LV_HIP(hipGetLastError());
    }
    LV_HIP(hipMemcpyAsync(idx, d_idx2, tot * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (d2) LV_HIP(hipMemcpyAsync(d2, d_d22, tot * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int QueryStore::box(const MapStore& map, hipStream_t stream, const float lo[3], const float hi[3], uint32_t* idx, float* xyz, size_t capacity,
                    size_t* n_out) {
    if (!lo || !hi || !n_out) { set_error("null argument"); return LV_EINVAL; }
    *n_out = 0;
    if (map.view.m == 0 || map.n_ids == 0) return LV_OK;
    if (map.n_ids > (uint32_t)SCAN_MAX) { set_error("map of %u ids: a box search scans at most %d", map.n_ids, SCAN_MAX); return LV_EINVAL; }
    const uint32_t ids = map.n_ids;
    int rc = d_off.need_pow2((size_t)ids + 1, QUERY_FLOOR);
    if (!rc) rc = d_cnt.need_pow2(ids, QUERY_FLOOR);
    if (!rc) rc = h_word.need(4);
    if (rc) return rc;
    hipLaunchKernelGGL(query_box_flag_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2],
                       d_cnt);
    LV_HIP(hipGetLastError());
    size_t bytes = 0;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_cnt.p, d_off.p, (int)ids, stream));
    rc = d_tmp.need_pow2(bytes, QUERY_TMP_FLOOR);
    if (rc) return rc;
    LV_HIP((hipError_t)hipcub::DeviceScan::ExclusiveSum(d_tmp.p, bytes, d_cnt.p, d_off.p, (int)ids, stream));
    hipLaunchKernelGGL(scan_total_kernel<uint32_t>, dim3(1), dim3(64), 0, stream, d_off, d_cnt, ids, d_off + ids);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(h_word, d_off + ids, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    const size_t tot = h_word[0];
    *n_out = tot;
    if (!idx && !xyz) return LV_OK;   // count only
    if (capacity < tot) { set_error("capacity %zu < %zu results", capacity, tot); return LV_EINVAL; }
    if (tot == 0) return LV_OK;
    rc = d_idx.need_pow2(tot, QUERY_FLOOR);
    if (!rc) rc = d_d2.need_pow2(3 * tot, QUERY_FLOOR);
    const uint32_t* rank = nullptr;
    if (!rc) rc = ensure_rank(map, stream, &rank);
    if (rc) return rc;
    hipLaunchKernelGGL(query_box_scatter_kernel, dim3(blocks_of(ids, 256)), dim3(256), 0, stream, map.d_orig, ids, d_cnt, d_off, rank, d_idx, d_d2);
    LV_HIP(hipGetLastError());
    if (idx) LV_HIP(hipMemcpyAsync(idx, d_idx, tot * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (xyz) LV_HIP(hipMemcpyAsync(xyz, d_d2, 3 * tot * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

void QueryStore::release() {
    pts.release();
    d_idx.release(); d_d2.release(); d_found.release(); d_idx2.release(); d_d22.release(); d_off.release(); d_cnt.release();
    d_roff.release(); d_rcnt.release(); d_tmp.release(); d_rank.release(); d_flag.release(); h_word.release();
    *this = QueryStore();
}

}  // namespace lv
