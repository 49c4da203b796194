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
//
// lv_volume_recentre (DESIGN.md "Rolling volumes") is ONE gather pass, occ_shift_kernel, into a second buffer of the grid's size
// that then changes places with the first: one lane per aligned group of four destination voxels and one 16-byte store per
// lane, so every destination voxel is written exactly once, the exposed ones with the NaN bits (no fill, no second pass).  The
// source of a group lies dx floats further along its row and is in general not aligned: four dword loads per lane, a
// wavefront's lanes reading one contiguous 1 KiB stretch; when nx % 4 == 0 and dx % 4 == 0 the source group is aligned as well
// and is one 16-byte load.  An exposed voxel also reads its mirror image in the old grid, which is a voxel that leaves the
// volume (grid_shift_mirror): that is how "held evidence and left" is counted without a pass over the old grid.
// lv_occ_mark is two kernels: occ_mark_count_kernel, one lane per source point and one integer atomicAdd into the per-voxel
// counts (the second buffer, zeroed over the box), and occ_mark_apply_kernel over the voxels of the box.
// The counts of both calls are folded per workgroup (block_fold4) by workgroups that stride over their items: two atomics each.
#include "lv_occupancy.hpp"

#include <cstring>
#include <utility>

#include "lv_host.hpp"

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

// ---- recentre.  The values move as bits: src and dst are the log-odds as uint32.
__device__ __forceinline__ uint32_t occ_evidence(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u ? 0u : 1u; }   // not NaN

// ALIGNED: nx % 4 == 0 and dx % 4 == 0 (a group and its source lie in one row each and are both 16-byte aligned; n_vox % 4 == 0).
// A workgroup strides over the groups and adds its two counts once: stats[1] += exposed voxels, stats[2] += those that left (an
// atomic per wavefront of a launch of one group per lane, 65536 wavefronts on three addresses, cost 0.8 - 1.2 ms on the default
// grid against 30 us for the bytes; DESIGN.md "Rolling volumes").  The kept voxels are the others: the host subtracts.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void occ_shift_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, GridDims g, int32_t dx,
                                                        int32_t dy, int32_t dz, uint32_t n_vox, unsigned long long* stats) {
    __shared__ unsigned long long sh[4][4];
    const uint32_t groups = (n_vox + 3u) / 4u;
    unsigned long long exposed = 0, left = 0;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < groups; t += gridDim.x * 256u) {
        const uint32_t c0 = 4u * t;
        int i, j, k, si, sj, sk;
        grid_ijk(g, c0, i, j, k);
        if (ALIGNED) {
            uint4 v = make_uint4(OCC_NAN_BITS, OCC_NAN_BITS, OCC_NAN_BITS, OCC_NAN_BITS);
            if (grid_shift_source(g, dx, dy, dz, i, j, k, si, sj, sk)) {
                v = *reinterpret_cast<const uint4*>(src + grid_at(g, si, sj, sk));
            } else {
                grid_shift_mirror(g, i + 3, j, k, si, sj, sk);   // the mirrors of i .. i + 3 start at that of i + 3: an aligned group too
                const uint4 m = *reinterpret_cast<const uint4*>(src + grid_at(g, si, sj, sk));
                exposed += 4;
                left += occ_evidence(m.x) + occ_evidence(m.y) + occ_evidence(m.z) + occ_evidence(m.w);
            }
            *reinterpret_cast<uint4*>(dst + c0) = v;
        } else {
            const uint32_t n = n_vox - c0 < 4u ? n_vox - c0 : 4u;
            uint32_t e[4] = {OCC_NAN_BITS, OCC_NAN_BITS, OCC_NAN_BITS, OCC_NAN_BITS};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                if (q < n) {
                    if (grid_shift_source(g, dx, dy, dz, i, j, k, si, sj, sk)) {
                        e[q] = src[grid_at(g, si, sj, sk)];
                    } else {
                        grid_shift_mirror(g, i, j, k, si, sj, sk);
                        left += occ_evidence(src[grid_at(g, si, sj, sk)]);
                        ++exposed;
                    }
                    if (++i == g.nx) {   // the next voxel of the group
                        i = 0;
                        if (++j == g.ny) {
                            j = 0;
                            ++k;
                        }
                    }
                }
            }
            if (n == 4u) {
                *reinterpret_cast<uint4*>(dst + c0) = make_uint4(e[0], e[1], e[2], e[3]);
            } else {   // the grid's last one to three voxels
#pragma unroll
                for (uint32_t q = 0; q < 3; ++q)
                    if (q < n) dst[c0 + q] = e[q];
            }
        }
    }
    unsigned long long a;
    if (block_fold4(sh, exposed, left, 0ull, 0ull, a) && threadIdx.x < 2 && a) atomicAdd(stats + 1 + threadIdx.x, a);
}

// ---- mark
struct OccBox {
    int lo[3], hi[3];   // inclusive, inside the grid
};

// source point i: a living map point (MAP: the map's float4 per id) or a packed caller point; false: nothing there
template <bool MAP>
__device__ __forceinline__ bool occ_mark_source(const void* __restrict__ src, uint32_t i, float p[3]) {
    if (MAP) {
        const float4 q = static_cast<const float4*>(src)[i];
        if (!pt_alive(q)) return false;
        p[0] = q.x;
        p[1] = q.y;
        p[2] = q.z;
    } else {
        const float* q = static_cast<const float*>(src) + 3 * (size_t)i;
        p[0] = q[0];
        p[1] = q[1];
        p[2] = q[2];
    }
    return true;
}

// cnt: one count per voxel of the grid, zero over the box
template <bool MAP>
__global__ __launch_bounds__(256) void occ_mark_count_kernel(const void* __restrict__ src, uint32_t n, OccGrid g, OccBox b, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float p[3];
    int ci, cj, ck;
    if (i < n && occ_mark_source<MAP>(src, i, p) && grid_cell_of(g, g.origin, g.resolution, false, p, ci, cj, ck) && ci >= b.lo[0] &&
        ci <= b.hi[0] && cj >= b.lo[1] && cj <= b.hi[1] && ck >= b.lo[2] && ck <= b.hi[2])
        atomicAdd(cnt + grid_at(g, ci, cj, ck), 1u);
}

// A workgroup strides over the voxels of the box (bd: its dimensions, n_box its voxels) and adds its counts once: stats[0] +=
// points used (every one of them raised exactly one count of the box), stats[1] += candidates << 32 | voxels marked (each below
// 2^28: the halves do not meet).  The voxels left alone are the candidates that were not marked.
__global__ __launch_bounds__(256) void occ_mark_apply_kernel(float* __restrict__ L, const uint32_t* __restrict__ cnt, OccGrid g, OccBox b, GridDims bd,
                                                             uint32_t n_box, uint32_t min_points, int only_unknown, float l_mark,
                                                             unsigned long long* stats) {
    __shared__ unsigned long long sh[4][4];
    unsigned long long used = 0, packed = 0;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < n_box; t += gridDim.x * 256u) {
        int i, j, k;
        grid_ijk(bd, t, i, j, k);
        const size_t at = grid_at(g, b.lo[0] + i, b.lo[1] + j, b.lo[2] + k);
        const uint32_t c = cnt[at];
        float v = L[at];
        bool candidate, observed;
        const bool marked = grid_mark_voxel(c, min_points, only_unknown != 0, l_mark, g.l_min, g.l_max, v, candidate, observed);
        if (marked) L[at] = v;
        used += c;
        packed += ((unsigned long long)(candidate ? 1u : 0u) << 32) + (marked ? 1u : 0u);
    }
    unsigned long long a;
    if (block_fold4(sh, used, packed, 0ull, 0ull, a) && threadIdx.x < 2 && a) atomicAdd(stats + threadIdx.x, a);
}

}  // namespace

void OccStore::release() {
    d_L.release(); d_L2.release(); d_bits.release(); stats.release(); pts.release(); d_out.release(); d_proj.release(); d_sbits.release();
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
    for (int a = 0; a < 3; ++a) origin0[a] = p.origin[a];
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

int OccStore::recentre(hipStream_t stream, const int32_t d[3], const int32_t s_new[3], const float origin_new[3], uint64_t out[4]) {
    int rc = d_L2.need(n_vox);   // (kept from the first recentre on)
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    const GridDims g{grid.nx, grid.ny, grid.nz};
    const uint32_t blocks = grid_stride_blocks((n_vox + 3) / 4);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(d_L.p);
    uint32_t* dst = reinterpret_cast<uint32_t*>(d_L2.p);
    if (grid.nx % 4 == 0 && d[0] % 4 == 0)
        hipLaunchKernelGGL(occ_shift_kernel<true>, dim3(blocks), dim3(256), 0, stream, src, dst, g, d[0], d[1], d[2], (uint32_t)n_vox, stats.d.p);
    else
        hipLaunchKernelGGL(occ_shift_kernel<false>, dim3(blocks), dim3(256), 0, stream, src, dst, g, d[0], d[1], d[2], (uint32_t)n_vox, stats.d.p);
    LV_HIP(hipGetLastError());
    uint64_t st[4];
    rc = stats.read(stream, st);   // (waits for the stream)
    if (rc) return rc;
    if (out) {
        out[0] = (uint64_t)n_vox - st[1];   // a voxel is kept or exposed
        out[1] = st[1];
        out[2] = st[2];
        out[3] = 0;
    }
    std::swap(d_L, d_L2);
    for (int a = 0; a < 3; ++a) {
        shift[a] = s_new[a];
        prm.origin[a] = origin_new[a];
        grid.origin[a] = origin_new[a];
    }
    return LV_OK;
}

int OccStore::mark(hipStream_t stream, const lv_occ_mark_params& p, const int lo[3], const int hi[3], const void* map_orig, uint32_t n_ids,
                   const void* points, size_t stride, size_t n, uint64_t out[4]) {
    const bool from = points == nullptr;
    int rc = pts.reserve(stream, from ? 0 : n);   // (synchronises the stream)
    if (!rc) rc = d_L2.need(n_vox);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    if (!from) {
        pts.append(points, stride, n);
        rc = pts.upload(stream);
        if (rc) return rc;
    }
    OccBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = lo[a];
        b.hi[a] = hi[a];
    }
    const GridDims bd{hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1};
    const size_t n_box = grid_cells(bd);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(d_L2.p);
    // the counts of the box start from zero: the stretch of the linear index from its first voxel to its last
    const size_t first = grid_at(grid, lo[0], lo[1], lo[2]), last = grid_at(grid, hi[0], hi[1], hi[2]);
    LV_HIP(hipMemsetAsync(cnt + first, 0, (last - first + 1) * sizeof(uint32_t), stream));
    const uint32_t ns = from ? n_ids : (uint32_t)n;
    if (ns) {
        if (from)
            hipLaunchKernelGGL(occ_mark_count_kernel<true>, dim3(blocks_of(ns)), dim3(256), 0, stream, map_orig, ns, grid, b, cnt);
        else
            hipLaunchKernelGGL(occ_mark_count_kernel<false>, dim3(blocks_of(ns)), dim3(256), 0, stream, (const void*)pts.d.p, ns, grid, b, cnt);
    }
    hipLaunchKernelGGL(occ_mark_apply_kernel, dim3(grid_stride_blocks(n_box)), dim3(256), 0, stream, d_L.p, (const uint32_t*)cnt, grid, b, bd, (uint32_t)n_box,
                       (uint32_t)p.min_points, p.only_unknown, p.l_mark, stats.d.p);
    LV_HIP(hipGetLastError());
    uint64_t st[4];
    rc = stats.read(stream, st);
    if (rc) return rc;
    const uint64_t candidates = st[1] >> 32, marked = st[1] & 0xFFFFFFFFull;
    out[0] = st[0];
    out[1] = candidates;
    out[2] = marked;
    out[3] = candidates - marked;
    return LV_OK;
}

}  // namespace lv
