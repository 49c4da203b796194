// lv_occupancy.hip — the ray-cast occupancy grid (include/limovelo_hip.h "Occupancy grid"; the rule's code is lv_occupancy.hpp).
//
// Per view two kernels, on the context's stream:
//   occ_march_kernel  one lane per return: range rules, world transform, quantisation, then the integer walk.  The cells go into
//                     two bitmaps, crossed and hit (one bit per voxel, 32 consecutive x per word).  A lane keeps the word it
//                     stands in and the bits it has gathered there in registers and issues ONE no-return atomicOr when the walk
//                     leaves the word, after a plain load that skips it when the bits are already set (the words round the
//                     sensor are shared by every ray: most of those atomics are skipped).  OR is idempotent and commutative, so
//                     the bitmaps do not depend on the schedule; the load can only see too few bits, never too many.
//   occ_fold_kernel   one lane per four words of both bitmaps (uint4 loads): hit wins over crossed, the set voxels take their one
//                     update, non-zero words are cleared for the next view, the update counts go to the stats.
// lv_occ_project / lv_occ_query are one-lane-per-item streaming kernels; fetch / load / clear are copies and a fill.
#include "lv_occupancy.hpp"

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

constexpr uint32_t OCC_NAN_BITS = 0x7FC00000u;
constexpr uint32_t OCC_NO_WORD = 0xFFFFFFFFu;

struct OccPose {
    float R[9];
    float t[3];
};

// OR `bits` into *word unless they are all there already
__device__ __forceinline__ void occ_or(uint32_t* word, uint32_t bits) {
    if ((*word & bits) != bits) atomicOr(word, bits);
}

// pts: n returns (packed x, y, z) of one view; qs: its quantised sensor origin.  crossed / hit: the bitmaps.
__global__ __launch_bounds__(256) void occ_march_kernel(const float* __restrict__ pts, uint32_t n, OccGrid g, OccPose pose, int32_t qsx,
                                                        int32_t qsy, int32_t qsz, uint32_t* crossed, uint32_t* hit,
                                                        unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int kind = OCC_RAY_IGNORED;
    int32_t qe[3] = {0, 0, 0};
    if (i < n) kind = occ_return(g, pose.R, pose.t, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], qe);
    if (kind != OCC_RAY_IGNORED) {
        const int32_t qs[3] = {qsx, qsy, qsz};
        OccWalk w;
        occ_walk_init(w, qs, qe);
        uint32_t cur = OCC_NO_WORD, bits = 0;
        bool left = false;
        while (!occ_walk_done(w)) {
            if (occ_in_grid(g, w.vx, w.vy, w.vz)) {
                const uint32_t word = ((uint32_t)w.vz * (uint32_t)g.ny + (uint32_t)w.vy) * (uint32_t)g.wx + ((uint32_t)w.vx >> 5);
                if (word != cur) {
                    if (cur != OCC_NO_WORD) occ_or(crossed + cur, bits);
                    cur = word;
                    bits = 0;
                }
                bits |= 1u << (w.vx & 31);
            } else if (occ_walk_left(g, w)) {
                left = true;
                break;
            }
            occ_walk_step(w);
        }
        // ve: hit, or crossed when the return was cut
        if (!left && occ_in_grid(g, w.vx, w.vy, w.vz)) {
            const uint32_t word = ((uint32_t)w.vz * (uint32_t)g.ny + (uint32_t)w.vy) * (uint32_t)g.wx + ((uint32_t)w.vx >> 5);
            const uint32_t bit = 1u << (w.vx & 31);
            if (kind == OCC_RAY_HIT) {
                occ_or(hit + word, bit);
            } else {
                if (word != cur) {
                    if (cur != OCC_NO_WORD) occ_or(crossed + cur, bits);
                    cur = word;
                    bits = 0;
                }
                bits |= bit;
            }
        }
        if (cur != OCC_NO_WORD) occ_or(crossed + cur, bits);
    }
    wave_add_to(stats + 0, kind != OCC_RAY_IGNORED ? 1u : 0u);
    wave_add_to(stats + 1, kind == OCC_RAY_CUT ? 1u : 0u);
}

// the voxels of one word take their update; returns nothing, counts through nf / nh
__device__ __forceinline__ void occ_fold_word(const OccGrid& g, float* __restrict__ L, uint32_t word, uint32_t c, uint32_t h, uint32_t& nf,
                                              uint32_t& nh) {
    c &= ~h;
    nf += (uint32_t)__popc(c);
    nh += (uint32_t)__popc(h);
    const uint32_t row = word / (uint32_t)g.wx;
    float* base = L + (size_t)row * (size_t)g.nx + (size_t)(word - row * (uint32_t)g.wx) * 32u;
    uint32_t m = c | h;
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1;
        base[b] = occ_update(base[b], ((h >> b) & 1u) ? g.l_hit : g.l_miss, g.l_min, g.l_max);
    }
}

// n4: the uint4 groups of one bitmap (the word arrays are padded to a multiple of four; the padding stays zero)
__global__ __launch_bounds__(256) void occ_fold_kernel(float* __restrict__ L, uint4* __restrict__ crossed, uint4* __restrict__ hit, uint32_t n4,
                                                       OccGrid g, unsigned long long* stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nf = 0, nh = 0;
    if (i < n4) {
        const uint4 c = crossed[i], h = hit[i];
        if (c.x | c.y | c.z | c.w | h.x | h.y | h.z | h.w) {
            if (c.x | h.x) occ_fold_word(g, L, 4u * i, c.x, h.x, nf, nh);
            if (c.y | h.y) occ_fold_word(g, L, 4u * i + 1u, c.y, h.y, nf, nh);
            if (c.z | h.z) occ_fold_word(g, L, 4u * i + 2u, c.z, h.z, nf, nh);
            if (c.w | h.w) occ_fold_word(g, L, 4u * i + 3u, c.w, h.w, nf, nh);
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            if (c.x | c.y | c.z | c.w) crossed[i] = zero;
            if (h.x | h.y | h.z | h.w) hit[i] = zero;
        }
    }
    wave_add_to(stats + 2, nf);
    wave_add_to(stats + 3, nh);
}

// one lane per column (i, j); k0..k1 already clipped (k0 > k1: an empty band)
__global__ __launch_bounds__(256) void occ_project_kernel(const float* __restrict__ L, OccGrid g, int k0, int k1, float l_occ, float l_free,
                                                          int8_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t plane = (uint32_t)g.nx * (uint32_t)g.ny;
    if (c >= plane) return;
    out[c] = (int8_t)grid_project_column(L, plane, c, k0, k1, l_occ, l_free);
}

__global__ __launch_bounds__(256) void occ_query_kernel(const float* __restrict__ L, OccGrid g, const float* __restrict__ pts, uint32_t n,
                                                        float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int ci, cj, ck;
    out[i] = grid_cell_of(g, g.origin, g.resolution, false, pts + 3 * (size_t)i, ci, cj, ck) ? L[grid_at(g, ci, cj, ck)] : __uint_as_float(OCC_NAN_BITS);
}

}  // namespace

void OccStore::release() {
    d_L.release(); d_bits.release(); stats.release(); pts.release(); d_out.release(); d_proj.release();
    *this = OccStore();
}

int OccStore::configure(hipStream_t stream, const lv_occupancy_params& p) {
    LV_HIP(hipStreamSynchronize(stream));
    release();
    const OccGrid g = occ_grid_of(p);
    const size_t nv = grid_cells(g);
    const size_t nw = (((size_t)g.wx * (size_t)p.ny * (size_t)p.nz) + 3) & ~(size_t)3;
    int rc = d_L.need(nv);
    if (!rc) rc = d_bits.need(2 * nw);
    if (!rc) rc = d_proj.need((size_t)p.nx * (size_t)p.ny);
    if (!rc) rc = stats.need();
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(d_bits, 0, 2 * nw * sizeof(uint32_t), stream));
    prm = p;
    grid = g;
    n_vox = nv;
    n_words = nw;
    rc = clear(stream);
    if (rc) return rc;
    configured = true;
    return LV_OK;
}

int OccStore::clear(hipStream_t stream) {
    LV_HIP(hipMemsetD32Async((hipDeviceptr_t)d_L, (int)OCC_NAN_BITS, n_vox, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int OccStore::integrate(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t out[4]) {
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) total += views[v].n;
    int rc = LV_OK;
    if (total) {   // every view's returns in one upload
        rc = pts.reserve(stream, total);
        if (rc) return rc;
        for (size_t v = 0; v < n_views; ++v) pts.append(views[v].points, views[v].stride, views[v].n);
        rc = pts.upload(stream);
        if (rc) return rc;
    }
    rc = stats.zero(stream);
    if (rc) return rc;
    uint32_t* crossed = d_bits;
    uint32_t* hit = d_bits + n_words;
    size_t o = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const size_t n = views[v].n;
        int32_t qs[3];
        if (n && occ_view_origin(grid, views[v].t, qs)) {
            OccPose pose;
            std::memcpy(pose.R, views[v].R, sizeof(pose.R));
            std::memcpy(pose.t, views[v].t, sizeof(pose.t));
            hipLaunchKernelGGL(occ_march_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, pts.d + 3 * o, (uint32_t)n, grid, pose, qs[0], qs[1],
                               qs[2], crossed, hit, stats.d);
            hipLaunchKernelGGL(occ_fold_kernel, dim3(blocks_of(n_words / 4)), dim3(256), 0, stream, d_L, reinterpret_cast<uint4*>(crossed),
                               reinterpret_cast<uint4*>(hit), (uint32_t)(n_words / 4), grid, stats.d);
            LV_HIP(hipGetLastError());
        }
        o += n;
    }
    return stats.read(stream, out);
}

int OccStore::query(hipStream_t stream, const void* points, size_t stride, size_t n, float* logodds) {
    if (n == 0) return LV_OK;
    int rc = pts.reserve(stream, n);
    if (!rc) rc = d_out.need(n);
    if (rc) return rc;
    pts.append(points, stride, n);
    rc = pts.upload(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(occ_query_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, d_L, grid, pts.d, (uint32_t)n, d_out);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(logodds, d_out, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int OccStore::project(hipStream_t stream, int k_lo, int k_hi, int8_t* grid2d) {
    int k0, k1;
    grid_clip_band(k_lo, k_hi, grid.nz, k0, k1);
    const size_t plane = (size_t)grid.nx * (size_t)grid.ny;
    hipLaunchKernelGGL(occ_project_kernel, dim3(blocks_of(plane)), dim3(256), 0, stream, d_L, grid, k0, k1, prm.l_occ, prm.l_free, d_proj);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(grid2d, d_proj, plane, hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int OccStore::fetch(hipStream_t stream, float* logodds) {
    LV_HIP(hipMemcpyAsync(logodds, d_L, n_vox * sizeof(float), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int OccStore::load(hipStream_t stream, const float* logodds) {
    LV_HIP(hipMemcpyAsync(d_L, logodds, n_vox * sizeof(float), hipMemcpyHostToDevice, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

}  // namespace lv
