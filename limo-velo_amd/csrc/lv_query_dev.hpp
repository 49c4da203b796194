// lv_query_dev.hpp — wavefront primitives of the map queries (lv_query.hip) shared with the surface kernels (lv_surface.hip):
// the running top-k of one query (TopK over wave_sort64), the hash probe of a grid table and the three candidate streams of the
// ladder (a level-0 run, the level-2 voxel lists of a box, every id).  Moved here unchanged from lv_query.hip, whose kernels
// compile to the same instructions with it.
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

}  // namespace lv
