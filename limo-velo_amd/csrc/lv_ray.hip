// lv_ray.hip — ray casting and view gain on the occupancy grid (include/limovelo_hip.h "Ray casting"; the rule's code is lv_ray.hpp).
//
// On the context's stream:
//   ray_classify_kernel  one lane per voxel of the x rows padded to whole words: the state of its voxel, sixteen lanes' states
//                        folded into one word of the packed volume (2 bits per voxel), stored by the first of them.  Runs in
//                        the first call after the grid changed.
//   ray_cast_kernel      one lane per ray: both ends quantised, then the walk of lv_ray.hpp through the packed states.  The
//                        lane keeps the word it stands in in a register and loads again only when the walk leaves it.  The
//                        result goes out as two 16-byte stores.
//   ray_gain_march_kernel  per view, one lane per return: occ_return, then the same walk, every in-grid cell before the stop
//                        into OccStore's first bitmap, by the march's own word-in-a-register and skip-if-set atomicOr.
//   ray_gain_fold_kernel per view, one lane per four words of that bitmap: the set voxels are classified against L and
//                        counted into the view's counters, non-zero words cleared.  OR is idempotent: a voxel counts once
//                        however many rays saw it, and the bitmap is all zero again when the call returns.
#include "lv_ray.hpp"

#include <cstring>

#include "lv_common.hpp"

namespace lv {

namespace {

constexpr uint32_t RAY_NO_WORD = 0xFFFFFFFFu;

struct RayPose {
    float R[9];
    float t[3];
};

// n: rows * wx16 * 16 lanes; lane id is voxel (id % (wx16 * 16)) of row id / (wx16 * 16).  A group of 16 lanes never straddles
// a row, nor a wavefront.
__global__ __launch_bounds__(256) void ray_classify_kernel(const float* __restrict__ L, uint32_t n, int nx, float l_free, float l_occ,
                                                           uint32_t* __restrict__ words) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t padded = (uint32_t)ray_wx16(nx) * 16u;
    const uint32_t row = id / padded, i = id - row * padded;
    uint32_t v = 0;
    if (id < n && i < (uint32_t)nx) v = ray_pack(fr_state_voxel(L[(size_t)row * (size_t)nx + i], l_free, l_occ), (int)i);
    for (int o = 8; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    if (id < n && (i & 15u) == 0) words[id >> 4] = v;
}

// pts: n `from` points, then n `to` points, packed
__global__ __launch_bounds__(256) void ray_cast_kernel(const float* __restrict__ pts, uint32_t n, OccGrid g, int stop_unknown,
                                                       const uint32_t* __restrict__ words, lv_ray_result* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = pts + 3 * (size_t)i;
    const float* b = pts + 3 * ((size_t)n + i);
    const float from[3] = {a[0], a[1], a[2]}, to[3] = {b[0], b[1], b[2]};
    RayStates st(words);
    lv_ray_result r;
    ray_cast(g, from, to, stop_unknown != 0, st, r);
    int4* o = reinterpret_cast<int4*>(out + i);
    o[0] = make_int4(r.status, r.cell, r.steps, r.axis);
    o[1] = make_int4(r.n_free, r.n_unknown, r.num, r.den);
}

// The cells a lane has seen, word by word (occ_march_kernel's scheme)
struct RaySeenBits {
    const OccGrid& g;
    uint32_t* bitmap;
    uint32_t cur, bits;
    __device__ RaySeenBits(const OccGrid& grid, uint32_t* b) : g(grid), bitmap(b), cur(RAY_NO_WORD), bits(0) {}
    __device__ void flush() {
        if (cur != RAY_NO_WORD && (bitmap[cur] & bits) != bits) atomicOr(bitmap + cur, bits);
    }
    __device__ void operator()(int i, int j, int k) {
        const uint32_t word = ((uint32_t)k * (uint32_t)g.ny + (uint32_t)j) * (uint32_t)g.wx + ((uint32_t)i >> 5);
        if (word != cur) {
            flush();
            cur = word;
            bits = 0;
        }
        bits |= 1u << (i & 31);
    }
};

// pts: the n returns of one view; qs: its quantised origin; gain: the view's four counters
__global__ __launch_bounds__(256) void ray_gain_march_kernel(const float* __restrict__ pts, uint32_t n, OccGrid g, RayPose pose, int32_t qsx,
                                                             int32_t qsy, int32_t qsz, const uint32_t* __restrict__ words, uint32_t* seen_bits,
                                                             unsigned long long* gain) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int kind = OCC_RAY_IGNORED;
    int32_t qe[3] = {0, 0, 0};
    if (i < n) kind = occ_return(g, pose.R, pose.t, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], qe);
    uint32_t stopped = 0;
    if (kind != OCC_RAY_IGNORED) {
        const int32_t qs[3] = {qsx, qsy, qsz};
        RayStates st(words);
        RaySeenBits seen(g, seen_bits);
        lv_ray_result r;
        ray_walk(g, qs, qe, false, st, seen, r);
        seen.flush();
        stopped = r.status == LV_RAY_STOPPED ? 1u : 0u;
    }
    wave_add_to(gain + 0, kind != OCC_RAY_IGNORED ? 1u : 0u);
    wave_add_to(gain + 1, stopped);
}

// the set voxels of one bitmap word against L
__device__ __forceinline__ void ray_gain_word(const OccGrid& g, const float* __restrict__ L, uint32_t word, uint32_t m, float l_free, float l_occ,
                                              uint32_t& nu, uint32_t& nf) {
    const uint32_t row = word / (uint32_t)g.wx;
    const float* base = L + (size_t)row * (size_t)g.nx + (size_t)(word - row * (uint32_t)g.wx) * 32u;
    while (m) {
        const int b = __ffs((int)m) - 1;
        m &= m - 1;
        const int s = fr_state_voxel(base[b], l_free, l_occ);
        nu += s == FR_UNKNOWN;
        nf += s == FR_FREE;
    }
}

// n4: the uint4 groups of the bitmap (padded to a multiple of four words; the padding stays zero)
__global__ __launch_bounds__(256) void ray_gain_fold_kernel(const float* __restrict__ L, uint4* __restrict__ seen_bits, uint32_t n4, OccGrid g,
                                                            float l_free, float l_occ, unsigned long long* gain) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nu = 0, nf = 0;
    if (i < n4) {
        const uint4 c = seen_bits[i];
        if (c.x | c.y | c.z | c.w) {
            if (c.x) ray_gain_word(g, L, 4u * i, c.x, l_free, l_occ, nu, nf);
            if (c.y) ray_gain_word(g, L, 4u * i + 1u, c.y, l_free, l_occ, nu, nf);
            if (c.z) ray_gain_word(g, L, 4u * i + 2u, c.z, l_free, l_occ, nu, nf);
            if (c.w) ray_gain_word(g, L, 4u * i + 3u, c.w, l_free, l_occ, nu, nf);
            seen_bits[i] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    wave_add_to(gain + 2, nu);
    wave_add_to(gain + 3, nf);
}

}  // namespace

void RayStore::release() {
    d_states.release(); pts.release(); d_res.release(); d_gain.release(); h_gain.release();
    *this = RayStore();
}

int RayStore::classify(hipStream_t stream, OccStore& occ) {
    if (packed) return LV_OK;
    const OccGrid& g = occ.grid;
    const size_t rows = (size_t)g.ny * (size_t)g.nz, n_words = rows * (size_t)ray_wx16(g.nx);
    const int rc = d_states.need(n_words);
    if (rc) return rc;
    hipLaunchKernelGGL(ray_classify_kernel, dim3(blocks_of(n_words * 16)), dim3(256), 0, stream, occ.d_L, (uint32_t)(n_words * 16), g.nx,
                       occ.prm.l_free, occ.prm.l_occ, d_states.p);
    LV_HIP(hipGetLastError());
    packed = true;
    return LV_OK;
}

int RayStore::raycast(hipStream_t stream, OccStore& occ, const lv_ray_params& p, const void* from, size_t from_stride, const void* to,
                      size_t to_stride, size_t n, lv_ray_result* out) {
    if (n == 0) return LV_OK;
    int rc = pts.reserve(stream, 2 * n);
    if (!rc) rc = d_res.need(n);
    if (!rc) rc = classify(stream, occ);
    if (rc) return rc;
    pts.append(from, from_stride, n);
    pts.append(to, to_stride, n);
    rc = pts.upload(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(ray_cast_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, pts.d, (uint32_t)n, occ.grid, p.stop_unknown, d_states.p, d_res.p);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(out, d_res, n * sizeof(lv_ray_result), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

int RayStore::view_gain(hipStream_t stream, OccStore& occ, const lv_view* views, size_t n_views, uint64_t* gain) {
    size_t total = 0;
    for (size_t v = 0; v < n_views; ++v) total += views[v].n;
    int rc = pts.reserve(stream, total);   // (synchronises the stream: h_gain is free as well)
    if (!rc) rc = d_gain.need(4 * OCC_MAX_VIEWS);
    if (!rc) rc = h_gain.need(4 * OCC_MAX_VIEWS);
    if (!rc) rc = classify(stream, occ);
    if (rc) return rc;
    for (size_t v = 0; v < n_views; ++v) pts.append(views[v].points, views[v].stride, views[v].n);
    rc = pts.upload(stream);
    if (rc) return rc;
    LV_HIP(hipMemsetAsync(d_gain, 0, 4 * n_views * sizeof(unsigned long long), stream));
    const OccGrid& g = occ.grid;
    uint32_t* seen = occ.d_bits;   // the first bitmap: all zero between the views of lv_occ_integrate, and between these
    size_t o = 0;
    for (size_t v = 0; v < n_views; ++v) {
        const size_t n = views[v].n;
        int32_t qs[3];
        if (n && occ_view_origin(g, views[v].t, qs)) {
            RayPose pose;
            std::memcpy(pose.R, views[v].R, sizeof(pose.R));
            std::memcpy(pose.t, views[v].t, sizeof(pose.t));
            hipLaunchKernelGGL(ray_gain_march_kernel, dim3(blocks_of(n)), dim3(256), 0, stream, pts.d + 3 * o, (uint32_t)n, g, pose, qs[0], qs[1], qs[2],
                               d_states.p, seen, d_gain.p + 4 * v);
            hipLaunchKernelGGL(ray_gain_fold_kernel, dim3(blocks_of(occ.n_words / 4)), dim3(256), 0, stream, occ.d_L, reinterpret_cast<uint4*>(seen),
                               (uint32_t)(occ.n_words / 4), g, occ.prm.l_free, occ.prm.l_occ, d_gain.p + 4 * v);
            LV_HIP(hipGetLastError());
        }
        o += n;
    }
    LV_HIP(hipMemcpyAsync(h_gain.p, d_gain.p, 4 * n_views * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < 4 * n_views; ++i) gain[i] = (uint64_t)h_gain.p[i];
    return LV_OK;
}

}  // namespace lv
