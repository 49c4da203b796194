// lv_place.hip — place recognition (include/limovelo_hip.h "Place recognition"): Scan Context descriptors of scans and of the
// map, and their brute-force retrieval over every yaw shift.
//
// Four kernels, no float atomics (a bin keeps the maximum of non-negative f32 values, which order like their bit patterns, so a
// u32 atomicMax takes it whatever the order):
//   place_scan_kernel   one lane per scan point: the workgroup's bins in LDS, then one global atomicMax per non-empty bin;
//   place_map_kernel    one lane per map id: the places of the call whose 2-D grid cell (side >= rmax) neighbours the point's, one
//                       global atomicMax per bin the point raises (a relaxed read first skips the bins it cannot raise);
//   place_score_kernel  one wavefront per place: lane c holds place column c in registers, the query sits column-major in LDS
//                       (one broadcast ds_read_b128 per four rings); for each query column j every lane forms the cosine of
//                       (query j, place c), and lane s takes the one of place column (j + s) mod n_sectors through ds_bpermute,
//                       so lane s sums d(s) for its shift in the order of j.  A wave minimum gives the place its key;
//   place_topk_kernel   k rounds of a workgroup minimum over 4096 keys per workgroup (16 per lane), repeated on the survivors
//                       until one workgroup is left: the k smallest keys in order, on the device.
#include "lv_place.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace lv {

namespace {

constexpr float PLACE_PI = 3.14159265358979323846f;

// The binning of the rule: the bin of q (relative to the place's centre) and its value v, or -1 when the point does not count.
// Every operation in f32, nothing fused (-ffp-contract=off).
__device__ __forceinline__ int place_bin(const PlaceRule& r, float qx, float qy, float qz, float& v) {
    const float rho = sqrtf(qx * qx + qy * qy);
    v = qz + r.z_offset;
    if (!(rho >= r.rmin && rho < r.rmax && v > 0.f)) return -1;
    int ring = (int)floorf((rho - r.rmin) / r.ring_w);
    ring = ring < 0 ? 0 : (ring > r.n_rings - 1 ? r.n_rings - 1 : ring);
    int sec = (int)floorf((atan2f(qy, qx) + PLACE_PI) / r.sector_w);
    sec = sec < 0 ? 0 : (sec > r.n_sectors - 1 ? r.n_sectors - 1 : sec);
    return ring * r.n_sectors + sec;
}

// grid-stride over the scan; out: n_bins dwords, zeroed by the caller
__global__ __launch_bounds__(256) void place_scan_kernel(const float4* __restrict__ pts, uint32_t n, PlaceFrame f, PlaceRule r,
                                                         uint32_t* __restrict__ out) {
    __shared__ uint32_t bins[PLACE_MAX_BINS];
    for (int i = threadIdx.x; i < r.n_bins; i += blockDim.x) bins[i] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = pts[i];
        const float qx = f.M[0] * p.x + f.M[1] * p.y + f.M[2] * p.z;
        const float qy = f.M[3] * p.x + f.M[4] * p.y + f.M[5] * p.z;
        const float qz = f.M[6] * p.x + f.M[7] * p.y + f.M[8] * p.z;
        float v;
        const int b = place_bin(r, qx, qy, qz, v);
        if (b >= 0) atomicMax(&bins[b], __float_as_uint(v));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < r.n_bins; i += blockDim.x) {
        const uint32_t v = bins[i];
        if (v) atomicMax(&out[i], v);
    }
}

// The call's centres binned into cells of side `side` over [x0, x0 + nx side) x [y0, y0 + ny side)
struct PlaceGrid {
    float x0, y0, side;
    int nx, ny;
};

// one lane per id (dead ids read x = +-inf and are skipped); out: the call's k descriptors, zeroed by the caller
__global__ __launch_bounds__(256) void place_map_kernel(const float4* __restrict__ orig, uint32_t n_ids, const float4* __restrict__ cent,
                                                        const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ citems, PlaceGrid g,
                                                        PlaceRule r, uint32_t* __restrict__ out) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const float4 p = orig[id];
    const float inf = __uint_as_float(0x7F800000u);
    if (!(p.x < inf && p.x > -inf)) return;
    const float fx = floorf((p.x - g.x0) / g.side), fy = floorf((p.y - g.y0) / g.side);
    if (!(fx >= -1.f && fx <= (float)g.nx && fy >= -1.f && fy <= (float)g.ny)) return;
    const int cx = (int)fx, cy = (int)fy;
    for (int y = cy - 1; y <= cy + 1; ++y) {
        if (y < 0 || y >= g.ny) continue;
        for (int x = cx - 1; x <= cx + 1; ++x) {
            if (x < 0 || x >= g.nx) continue;
            const uint32_t c = (uint32_t)y * (uint32_t)g.nx + (uint32_t)x;
            for (uint32_t k = cstart[c]; k < cstart[c + 1]; ++k) {
                const uint32_t pi = citems[k];
                const float4 o = cent[pi];
                float v;
                const int b = place_bin(r, p.x - o.x, p.y - o.y, p.z - o.z, v);
                if (b < 0) continue;
                uint32_t* d = out + pi * (uint32_t)r.n_bins + (uint32_t)b;
                const uint32_t bits = __float_as_uint(v);
                if (__hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(d, bits);
            }
        }
    }
}

// RP: n_rings rounded up to a multiple of 4 (the rows beyond n_rings are zero on both sides and add +0 to every sum).
// qbits: the query's n_bins values (f32 bits, ring-major); keys[p] = (d bits << 32) | (p << 6) | shift.
template <int RP>
__global__ __launch_bounds__(256) void place_score_kernel(const float* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ qbits,
                                                          PlaceRule r, uint64_t* __restrict__ keys) {
    __shared__ float4 qT4[PLACE_MAX_SECTORS * RP / 4];   // the query column-major: column j at qT[j * RP .. j * RP + RP)
    __shared__ float qn[PLACE_MAX_SECTORS];              // its column norms
    float* qT = reinterpret_cast<float*>(qT4);
    const int R = r.n_rings, S = r.n_sectors, B = r.n_bins;
    for (int i = threadIdx.x; i < S * RP; i += blockDim.x) {
        const int j = i / RP, rr = i - j * RP;
        qT[i] = rr < R ? __uint_as_float(qbits[rr * S + j]) : 0.f;
    }
    __syncthreads();
    if ((int)threadIdx.x < S) {
        float s = 0.f;
        for (int rr = 0; rr < R; ++rr) s = s + qT[threadIdx.x * RP + rr] * qT[threadIdx.x * RP + rr];
        qn[threadIdx.x] = sqrtf(s);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    // lane s (< S) reads lane (j + s) mod S; the others read themselves
    for (uint32_t p = blockIdx.x * waves + wave; p < n; p += gridDim.x * waves) {
        const float* P = desc + (size_t)p * (size_t)B;
        float col[RP];
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) col[rr] = (rr < R && lane < S) ? P[rr * S + lane] : 0.f;
        float pn2 = 0.f;
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) pn2 = pn2 + col[rr] * col[rr];
        const float pn = sqrtf(pn2);
        float acc = 0.f;
        int cnt = 0;
        int src = lane;
        for (int j = 0; j < S; ++j) {
            float dot = 0.f;
#pragma unroll
            for (int rr = 0; rr < RP; rr += 4) {
                const float4 q = qT4[(j * RP + rr) >> 2];
                dot = dot + q.x * col[rr];
                dot = dot + q.y * col[rr + 1];
                dot = dot + q.z * col[rr + 2];
                dot = dot + q.w * col[rr + 3];
            }
            const float qj = qn[j];
            const float c = (qj > 0.f && pn > 0.f) ? dot / (qj * pn) : -1.f;   // -1: no valid pair (a cosine here is >= 0)
            if (lane < S) src = lane + j < S ? lane + j : lane + j - S;
            const float cs = __shfl(c, src);
            if (cs >= 0.f) {
                acc = acc + cs;
                ++cnt;
            }
        }
        float d = cnt ? 1.f - acc / (float)cnt : 1.f;
        if (!(d > 0.f)) d = d <= 0.f ? 0.f : 1.f;   // below 0 by rounding: 0; NaN (values whose squares overflow): 1
        uint64_t key = lane < S ? ((uint64_t)__float_as_uint(d) << 32) | ((uint64_t)p << 6) | (uint64_t)lane : ~0ull;
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const uint64_t other = __shfl_xor(key, o);
            key = other < key ? other : key;
        }
        if (lane == 0) keys[p] = key;
    }
}

// Workgroup b: the k smallest of in[b * 4096 .. min(n, (b + 1) * 4096)) to out[b * k .. b * k + k), ascending (~0 where the
// chunk holds fewer than k).  Keys are distinct apart from ~0.
__global__ __launch_bounds__(256) void place_topk_kernel(const uint64_t* __restrict__ in, uint32_t n, int k, uint64_t* __restrict__ out) {
    constexpr int PER = PLACE_TOPK_CHUNK / 256;
    __shared__ uint64_t wmin[2][4];
    uint64_t v[PER];
    const uint32_t base = blockIdx.x * PLACE_TOPK_CHUNK;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const uint32_t idx = base + (uint32_t)i * 256u + threadIdx.x;
        v[i] = idx < n ? in[idx] : ~0ull;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int round = 0; round < k; ++round) {
        uint64_t m = v[0];
#pragma unroll
        for (int i = 1; i < PER; ++i) m = v[i] < m ? v[i] : m;
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const uint64_t other = __shfl_xor(m, o);
            m = other < m ? other : m;
        }
        const int b = round & 1;   // (double-buffered: a round's writes never meet the previous round's reads)
        if (lane == 0) wmin[b][wave] = m;
        __syncthreads();
        uint64_t sel = wmin[b][0];
        for (int w = 1; w < 4; ++w) sel = wmin[b][w] < sel ? wmin[b][w] : sel;
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (v[i] == sel) v[i] = ~0ull;
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * (size_t)k + (size_t)round] = sel;
    }
}

void rot_of(const double* q, double R[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - z * w);
    R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);
    R[7] = 2.0 * (y * z + x * w);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

}  // namespace

void place_frame(const lv_state& x, PlaceFrame* f, double centre[3]) {
    double A[9], B[9];
    rot_of(x.rot, A);
    rot_of(x.offset_R_L_I, B);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) f->M[i * 3 + j] = (float)(A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j]);
        centre[i] = A[i * 3] * x.offset_T_L_I[0] + A[i * 3 + 1] * x.offset_T_L_I[1] + A[i * 3 + 2] * x.offset_T_L_I[2] + x.pos[i];
    }
}

PlaceRule PlaceStore::rule() const {
    PlaceRule r;
    r.n_rings = prm.n_rings;
    r.n_sectors = prm.n_sectors;
    r.n_bins = prm.n_rings * prm.n_sectors;
    r.rmin = prm.rmin;
    r.rmax = prm.rmax;
    r.z_offset = prm.z_offset;
    r.ring_w = (prm.rmax - prm.rmin) / (float)prm.n_rings;
    r.sector_w = (2.f * PLACE_PI) / (float)prm.n_sectors;
    return r;
}

int PlaceStore::reserve(hipStream_t stream, size_t want) {
    int rc = d_q.need(PLACE_MAX_BINS);
    const size_t stage = (PLACE_MAX_COUNT / PLACE_TOPK_CHUNK) * PLACE_MAX_K;
    if (!rc) rc = d_top[0].need(stage);
    if (!rc) rc = d_top[1].need(stage);
    if (rc) return rc;
    const size_t B = (size_t)bins();
    if (want * B <= d_desc.cap) return d_keys.need(want);
    size_t places = std::max<size_t>(want, std::min(PLACE_MAX_COUNT, std::max<size_t>(1024, 2 * (d_desc.cap / B))));
    DevBuf<float> grown;   // (the first n places move over before the old buffer goes)
    rc = grown.need(places * B);
    if (rc) return rc;
    if (n) LV_HIP(hipMemcpyAsync(grown, d_desc, n * B * sizeof(float), hipMemcpyDeviceToDevice, stream));
    LV_HIP(hipStreamSynchronize(stream));
    d_desc.release();
    d_desc = grown;
    return d_keys.need(places);
}

int PlaceStore::describe(const ScanStore& scan, hipStream_t stream, const PlaceFrame& f, uint32_t* out) {
    const PlaceRule r = rule();
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(1024, (scan.n + 1023) / 1024));
    hipLaunchKernelGGL(place_scan_kernel, dim3(grid), dim3(256), 0, stream, scan.d_sorted, scan.n, f, r, out);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

int PlaceStore::add_scan(const ScanStore& scan, hipStream_t stream, const PlaceFrame& f, const double centre[3], uint32_t* id) {
    int rc = reserve(stream, n + 1);
    if (rc) return rc;
    const size_t B = (size_t)bins();
    uint32_t* out = reinterpret_cast<uint32_t*>(d_desc + n * B);
    LV_HIP(hipMemsetAsync(out, 0, B * sizeof(uint32_t), stream));
    rc = describe(scan, stream, f, out);
    if (rc) return rc;
    LV_HIP(hipStreamSynchronize(stream));
    centres.insert(centres.end(), centre, centre + 3);
    if (id) *id = (uint32_t)n;
    ++n;
    return LV_OK;
}

int PlaceStore::add_map(const MapStore& map, hipStream_t stream, const double* cs, size_t k, uint32_t* first_id) {
    int rc = reserve(stream, n + k);
    if (rc) return rc;
    const size_t B = (size_t)bins();
    uint32_t* out = reinterpret_cast<uint32_t*>(d_desc + n * B);
    LV_HIP(hipMemsetAsync(out, 0, k * B * sizeof(uint32_t), stream));
    if (map.built && map.m > 0) {
        const PlaceRule r = rule();
        // the call's centres in f32 on a 2-D grid of cells at least rmax wide (1 % and 1 cm of slack over rmax cover the rounding of
        // the point's cell), at most 1024 x 1024 cells: a point's places lie in the 3 x 3 cells around its own
        std::vector<float4> cf(k);
        float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
        for (size_t i = 0; i < k; ++i) {
            cf[i] = make_float4((float)cs[3 * i], (float)cs[3 * i + 1], (float)cs[3 * i + 2], 0.f);
            lo[0] = std::min(lo[0], cf[i].x);
            lo[1] = std::min(lo[1], cf[i].y);
            hi[0] = std::max(hi[0], cf[i].x);
            hi[1] = std::max(hi[1], cf[i].y);
        }
        PlaceGrid g;
        const double extent = std::max((double)hi[0] - lo[0], (double)hi[1] - lo[1]);
        g.side = (float)std::max((double)prm.rmax * 1.01 + 0.01, extent / 1023.0);
        g.x0 = lo[0];
        g.y0 = lo[1];
        auto cell_of = [&](double v, float o, int nmax) {
            const int c = (int)std::floor((v - (double)o) / (double)g.side);
            return c < 0 ? 0 : (c > nmax - 1 ? nmax - 1 : c);
        };
        g.nx = (int)std::floor(((double)hi[0] - lo[0]) / g.side) + 1;
        g.ny = (int)std::floor(((double)hi[1] - lo[1]) / g.side) + 1;
        const size_t cells = (size_t)g.nx * (size_t)g.ny;
        std::vector<uint32_t> start(cells + 1, 0), items(k), cell(k);
        for (size_t i = 0; i < k; ++i) {
            cell[i] = (uint32_t)(cell_of(cf[i].y, g.y0, g.ny) * g.nx + cell_of(cf[i].x, g.x0, g.nx));
            ++start[cell[i] + 1];
        }
        for (size_t c = 0; c < cells; ++c) start[c + 1] += start[c];
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (size_t i = 0; i < k; ++i) items[fill[cell[i]]++] = (uint32_t)i;
        rc = d_cent.need(k);
        if (!rc) rc = d_cstart.need(cells + 1 + k);
        if (rc) return rc;
        d_citems = d_cstart + cells + 1;
        LV_HIP(hipMemcpyAsync(d_cent, cf.data(), k * sizeof(float4), hipMemcpyHostToDevice, stream));
        LV_HIP(hipMemcpyAsync(d_cstart, start.data(), (cells + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        LV_HIP(hipMemcpyAsync(d_citems, items.data(), k * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(place_map_kernel, dim3((map.n_ids + 255) / 256), dim3(256), 0, stream, map.d_orig, map.n_ids, d_cent, d_cstart,
                           d_citems, g, r, out);
        LV_HIP(hipGetLastError());
    }
    LV_HIP(hipStreamSynchronize(stream));   // (the host vectors above are the copies' sources)
    centres.insert(centres.end(), cs, cs + 3 * k);
    if (first_id) *first_id = (uint32_t)n;
    n += k;
    return LV_OK;
}

int PlaceStore::query(hipStream_t stream, int k, uint32_t* ids, int32_t* shifts, float* dist) {
    const PlaceRule r = rule();
    const uint32_t grid = (uint32_t)std::min<size_t>((n + 3) / 4, 2048);
    const int rp = (r.n_rings + 3) & ~3;
#define LV_PLACE_SCORE(RP)                                                                                                          \
    case RP:                                                                                                                        \
        hipLaunchKernelGGL(place_score_kernel<RP>, dim3(grid), dim3(256), 0, stream, d_desc, (uint32_t)n, d_q, r, d_keys);         \
        break;
    switch (rp) {
        LV_PLACE_SCORE(4)
        LV_PLACE_SCORE(8)
        LV_PLACE_SCORE(12)
        LV_PLACE_SCORE(16)
        LV_PLACE_SCORE(20)
        LV_PLACE_SCORE(24)
        LV_PLACE_SCORE(28)
        LV_PLACE_SCORE(32)
        default: set_error("n_rings %d", r.n_rings); return LV_EINVAL;
    }
#undef LV_PLACE_SCORE
    LV_HIP(hipGetLastError());
    const uint64_t* in = d_keys;
    uint32_t count = (uint32_t)n;
    int side = 0;
    for (;;) {
        const uint32_t blocks = (count + PLACE_TOPK_CHUNK - 1) / PLACE_TOPK_CHUNK;
        hipLaunchKernelGGL(place_topk_kernel, dim3(blocks), dim3(256), 0, stream, in, count, k, d_top[side]);
        LV_HIP(hipGetLastError());
        in = d_top[side];
        side ^= 1;
        if (blocks == 1) break;
        count = blocks * (uint32_t)k;
    }
    uint64_t top[PLACE_MAX_K];
    LV_HIP(hipMemcpyAsync(top, in, (size_t)k * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < k; ++i) {
        const uint32_t lo = (uint32_t)(top[i] & 0xFFFFFFFFull), hi = (uint32_t)(top[i] >> 32);
        if (ids) ids[i] = lo >> 6;
        if (shifts) shifts[i] = (int32_t)(lo & 63u);
        if (dist) std::memcpy(&dist[i], &hi, 4);
    }
    return LV_OK;
}

int PlaceStore::load(hipStream_t stream, const float* desc, const double* cs, size_t k) {
    int rc = reserve(stream, n + k);
    if (rc) return rc;
    const size_t B = (size_t)bins();
    LV_HIP(hipMemcpyAsync(d_desc + n * B, desc, k * B * sizeof(float), hipMemcpyHostToDevice, stream));
    LV_HIP(hipStreamSynchronize(stream));
    centres.insert(centres.end(), cs, cs + 3 * k);
    n += k;
    return LV_OK;
}

int PlaceStore::fetch(hipStream_t stream, float* desc, double* cs) const {
    if (n == 0) return LV_OK;
    if (desc) {
        LV_HIP(hipMemcpyAsync(desc, d_desc, n * (size_t)bins() * sizeof(float), hipMemcpyDeviceToHost, stream));
        LV_HIP(hipStreamSynchronize(stream));
    }
    if (cs) std::memcpy(cs, centres.data(), 3 * n * sizeof(double));
    return LV_OK;
}

void PlaceStore::release() {
    d_desc.release(); d_q.release(); d_keys.release(); d_top[0].release(); d_top[1].release(); d_cent.release(); d_cstart.release();
    *this = PlaceStore();
}

}  // namespace lv
