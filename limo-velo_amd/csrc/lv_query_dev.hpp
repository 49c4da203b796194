// lv_query_dev.hpp — what the map tools share on the device (lv_query.hip, lv_surface.hip, lv_cluster.hip, lv_visibility.hip;
// DESIGN.md "Map-tool helpers"): the running top-k of one query (TopK over wave_sort64), the hash probe of a grid
// table, the three candidate streams (a level-0 run, the level-2 voxel lists of a box, every id) and the two walks made of them
// — the k-NN ladder (knn_ladder) and the fixed-radius walk (radius_source + stream_radius) — besides the rank of an id among
// the living (rank_of), the wave-aggregated append to the map's dead list (dead_list_append) and the total of an exclusive
// scan (scan_total_kernel).  The living-id test is pt_alive (lv_mapinc.hpp).
#pragma once

#include "lv_search_dev.hpp"

namespace lv {

__device__ __forceinline__ kkey shfl_key(kkey v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src);
    hi = __shfl(hi, src);
    return __hiloint2double(hi, lo);
}
// a candidate is admitted iff its distance is finite (tombstones and slack read x = +inf) and d2 <= max_d2
__device__ __forceinline__ bool admitted(float d, float max_d2) { return __float_as_uint(d) < 0x7F800000u && d <= max_d2; }

// ascending bitonic sort of one key per lane over the 64 lanes
__device__ __forceinline__ kkey wave_sort64(kkey v, int lane) {
#pragma unroll
    for (int s = 2; s <= 64; s <<= 1) {
#pragma unroll
        for (int j = s >> 1; j > 0; j >>= 1) {
            const kkey o = shfl_xor_key(v, j);
            const bool up = (lane & s) == 0, lower = (lane & j) == 0;
            v = (lower == up) ? kmin(v, o) : kmax(v, o);
        }
    }
    return v;
}

// the running top-k of one query: top ascending over the lanes; kth = the k-th smallest so far (NONE while fewer)
struct TopK {
    kkey top;
    kkey kth;
    int k;
    __device__ __forceinline__ void reset() {
        top = none_key();
        kth = none_key();
    }
    // one chunk: every lane offers one candidate key (NONE = nothing)
    __device__ __forceinline__ void offer(kkey c, int lane) {
        if (__ballot(c < kth) == 0ull) return;
        const kkey s = wave_sort64(c, lane);
        kkey v = kmin(top, shfl_key(s, 63 - lane));
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) {
            const kkey o = shfl_xor_key(v, j);
            v = (lane & j) == 0 ? kmin(v, o) : kmax(v, o);
        }
        top = v;
        kth = shfl_key(top, k - 1);
    }
    // the level's acceptance rule (file header)
    __device__ __forceinline__ bool accept(float r, float max_d2) const {
        if (!(r > 0.f)) return false;
        const float rr = r * r;
        return (!is_none(kth) && __uint_as_float(key_hi(kth)) < rr) || max_d2 < rr;
    }
};

// hash probe of one grid table: {start, count} of the entry whose key is `key`, count 0 if absent
__device__ __forceinline__ uint2 probe(const GridLevel& g, uint64_t key) {
    if (!g.table) return make_uint2(0u, 0u);
    uint32_t slot = hash_cell(key, g.shift) & g.mask;
    for (;;) {
        const uint4 e = g.table[slot];
        const uint64_t ek = (uint64_t)e.x | ((uint64_t)e.y << 32);
        if (ek == key) return make_uint2(e.z, e.w);
        if (ek == EMPTY_KEY) return make_uint2(0u, 0u);
        slot = (slot + 1) & g.mask;
    }
}

// a run of level-0 storage (bucket or tile-group region): visit(x, y, z, id, ok) for 64 entries at a time
template <class F>
__device__ __forceinline__ void stream_run(const MapView& map, uint32_t start, uint32_t count, int lane, F&& visit) {
    const Xyz* __restrict__ bp = reinterpret_cast<const Xyz*>(map.bxyz[0]) + start;
    const uint32_t* __restrict__ ip = map.bidx[0] + start;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t j = base + (uint32_t)lane;
        const bool ok = j < count;
        const Xyz p = bp[ok ? j : 0];
        const uint32_t id = ip[ok ? j : 0];
        visit(p.x, p.y, p.z, id, ok);
    }
}

// every id
template <class F>
__device__ __forceinline__ void stream_all(const MapView& map, int lane, F&& visit) {
    for (uint32_t base = 0; base < map.n_ids; base += 64) {
        const uint32_t j = base + (uint32_t)lane;
        const bool ok = j < map.n_ids;
        const float4 p = map.orig[ok ? j : 0];
        visit(p.x, p.y, p.z, j, ok);
    }
}

// the level-2 voxel lists of the box [b, b + s) (level-2 voxel coordinates), 64 lists per round: every lane probes one, a wave
// scan turns the lengths into one virtual candidate array, each lane finds its list by binary search over the prefix sums
// (s_pref / s_start: 64 words each, private to this wavefront)
template <class F>
__device__ __forceinline__ void stream_lists(const MapView& map, int bx, int by, int bz, int sx, int sy, int sz, int lane, uint32_t* s_pref,
                                             uint32_t* s_start, F&& visit) {
    const uint32_t nc = (uint32_t)sx * (uint32_t)sy * (uint32_t)sz;
    for (uint32_t r0 = 0; r0 < nc; r0 += 64) {
        const uint32_t ci = r0 + (uint32_t)lane;
        uint32_t start = 0, cnt = 0;
        if (ci < nc) {
            const uint32_t dx = ci % (uint32_t)sx, dy = (ci / (uint32_t)sx) % (uint32_t)sy, dz = ci / ((uint32_t)sx * (uint32_t)sy);
            const uint32_t nx = (uint32_t)bx + dx, ny = (uint32_t)by + dy, nz = (uint32_t)bz + dz;
            if (nx < (1u << 19) && ny < (1u << 19) && nz < (1u << 19)) {
                const uint2 e = probe(map.ct, pack_cell(nx, ny, nz));
                start = e.x;
                cnt = e.y;
            }
        }
        uint32_t incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        const uint32_t total = __shfl(incl, 63);
        if (total == 0) continue;
        wave_lds_fence();   // the previous round's readers are done
        s_pref[lane] = incl - cnt;
        s_start[lane] = start;
        wave_lds_fence();
        for (uint32_t base = 0; base < total; base += 64) {
            const uint32_t v = base + (uint32_t)lane;
            const bool ok = v < total;
            const uint32_t vv = ok ? v : 0u;
            int L = 0;   // the last list whose first virtual index is <= vv (empty lists share their successor's)
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) L += s_pref[L + step] <= vv ? step : 0;
            const float4 p = map.cell4[s_start[L] + (vv - s_pref[L])];
            visit(p.x, p.y, p.z, __float_as_uint(p.w), ok);
        }
    }
}

// The k-NN ladder of one query (one wavefront; lv_query.hip header): the level-0 run, the tile group's region while the group is
// in one piece, the 27 level-2 lists, the 216 lists of the level-3 block, every id — each rung searched from scratch (t.reset())
// until one is accepted (TopK::accept).  t arrives reset; visit offers the candidates to it.
template <class F>
__device__ __forceinline__ void knn_ladder(const MapView& map, const QGeom& geo, TopK& t, float max_d2, int lane, uint32_t* s_pref,
                                           uint32_t* s_start, F&& visit) {
    bool done = false;
    if (geo.amax < CELL_FAR) {
        const uint2 b0 = probe(map.bt[0], pack_cell((uint32_t)geo.c0x, (uint32_t)geo.c0y, (uint32_t)geo.c0z));
        stream_run(map, b0.x, b0.y, lane, visit);
        done = t.accept(search_radius(map, geo, 0), max_d2);
        if (!done) {
            const uint2 g1 = probe(map.gt, pack_cell((uint32_t)(geo.c0x >> 1), (uint32_t)(geo.c0y >> 1), (uint32_t)(geo.c0z >> 1)));
            if (g1.y > 0) {   // (extent 0: the group is not in one piece)
                t.reset();
                stream_run(map, g1.x, g1.y, lane, visit);
                done = t.accept(search_radius(map, geo, 1), max_d2);
            }
        }
        if (!done) {
            t.reset();
            stream_lists(map, (geo.c0x >> 2) - 1, (geo.c0y >> 2) - 1, (geo.c0z >> 2) - 1, 3, 3, 3, lane, s_pref, s_start, visit);
            done = t.accept(search_radius(map, geo, 2), max_d2);
        }
        if (!done) {
            t.reset();
            stream_lists(map, ((geo.c0x >> 3) - 1) * 2, ((geo.c0y >> 3) - 1) * 2, ((geo.c0z >> 3) - 1) * 2, 6, 6, 6, lane, s_pref, s_start, visit);
            done = t.accept(search_radius(map, geo, 3), max_d2);
        }
    }
    if (!done) {
        t.reset();
        stream_all(map, lane, visit);
    }
}

// The candidates of a fixed-radius walk around (qx, qy, qz): the level-0 run while the radius is inside the level-0 bound (every
// point within it lies in the level-0 block), else the level-2 lists covering [q - r, q + r] with one list of margin per side for
// the rounding of the voxel coordinates, else (more lists than ids, or outside the voxel range) every id.
struct RadiusSource {
    bool run, lists;     // neither: every id
    int lo[3], ext[3];   // lists: the box of lists (level-2 voxel coordinates)
};
__device__ __forceinline__ RadiusSource radius_source(const MapView& map, const QGeom& geo, float qx, float qy, float qz, float radius) {
    RadiusSource s = {false, false, {0, 0, 0}, {0, 0, 0}};
    if (geo.amax < CELL_FAR) {
        if (radius < search_radius(map, geo, 0)) {
            s.run = true;
        } else {
            const float qq[3] = {qx, qy, qz};
            uint64_t nl = 1;
            bool fits = true;
            for (int a = 0; a < 3; ++a) {
                const int l = (cell_coord(qq[a] - radius, map.origin[a], map.inv_cell) >> 2) - 1;
                const int h = (cell_coord(qq[a] + radius, map.origin[a], map.inv_cell) >> 2) + 1;
                fits = fits && l >= 0 && h < (1 << 19) && h >= l;
                s.lo[a] = l;
                s.ext[a] = h - l + 1;
                nl *= (uint64_t)(fits ? s.ext[a] : 1);
            }
            s.lists = fits && nl <= (uint64_t)map.n_ids;
        }
    }
    return s;
}
template <class F>
__device__ __forceinline__ void stream_radius(const MapView& map, const RadiusSource& src, const QGeom& geo, int lane, uint32_t* s_pref,
                                              uint32_t* s_start, F&& visit) {
    if (src.run) {
        const uint2 b0 = probe(map.bt[0], pack_cell((uint32_t)geo.c0x, (uint32_t)geo.c0y, (uint32_t)geo.c0z));
        stream_run(map, b0.x, b0.y, lane, visit);
    } else if (src.lists) {
        stream_lists(map, src.lo[0], src.lo[1], src.lo[2], src.ext[0], src.ext[1], src.ext[2], lane, s_pref, s_start, visit);
    } else {
        stream_all(map, lane, visit);
    }
}

// the rank of a living id among the living (rank NULL: no id is dead, ranks are ids)
__device__ __forceinline__ uint32_t rank_of(const uint32_t* __restrict__ rank, uint32_t id) { return rank ? rank[id] : id; }

// Wave-aggregated append to the map's dead list, called by every lane of the wavefront: the lanes with `gone` store (x, y, z, id)
// of their point p behind one atomicAdd per wavefront on n_dead and make the id read x = +inf from here on.  An entry beyond
// dead_cap raises `overflow` instead of being stored.
__device__ __forceinline__ void dead_list_append(bool gone, const float4& p, uint32_t id, float4* __restrict__ orig, float4* __restrict__ dead,
                                                 uint32_t dead_cap, MapCounters* cnt) {
    const unsigned long long mask = __ballot(gone);
    if (mask == 0ull) return;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&cnt->n_dead, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    if (!gone) return;
    const uint32_t di = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (di < dead_cap) dead[di] = make_float4(p.x, p.y, p.z, __uint_as_float(id));
    else atomicExch(&cnt->overflow, 1u);
    orig[id].x = pos_inf();
}

// the total of an exclusive scan: last offset + last count
template <class T>
__global__ void scan_total_kernel(const T* __restrict__ excl, const T* __restrict__ cnt, uint32_t n, T* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = n ? excl[n - 1] + cnt[n - 1] : T(0);
}

}  // namespace lv
