// lv_surface.hip — lv_map_normals / lv_map_remove_outliers: the k nearest living neighbours of every living map point and a
// small reduction over them (include/limovelo_hip.h "Surface normals and outlier removal").
//
// The queries ARE the map's points:
//   surf_ladder_kernel  one wavefront per id walks knn_ladder (lv_query_dev.hpp; radius_source / stream_radius for the radius
//                       count) around its own point and reduces in place:
//                       the top-k sits one neighbour per lane, so each lane forms its own f64 offset and square root and leaves
//                       them in 1 KiB of LDS per wavefront; distance sum, mean and covariance are then summed in neighbour
//                       order, six lanes owning one covariance entry each.  The rule that needs distances only gathers nothing.
//                       (The same sums as uniform loops over v_readlane, without LDS, measured slower: DESIGN.md §2.)
//   surf_finish_kernel  one lane per id turns the covariance into the normal and the curvature (sym3_eig, lv_surface.hpp): the
//                       eigen-solve is lane-per-point work.
// Outliers: the ladder kernel keeps only the point's value (mean distance, or the count inside the radius);
//   surf_stat_kernel    block partials of sum d / sum (d - mu)^2 over the finite values, f64, folded in block order on the host;
//   surf_classify_kernel one lane per id: flag at the living rank, the outliers appended to the map's dead list (dead_list_append,
//                       lv_query_dev.hpp), retired by MapStore::retire_dead_list.
// A workgroup-per-voxel kernel over LDS-staged bucket runs was built and measured at 4.2 times the ladder's time;
// it is not shipped.  No scratch, no float atomics: every output is a pure function of the living points and the rule.
#include "lv_surface.hpp"

#include "lv_query_dev.hpp"

#include <cmath>
#include <cstring>

namespace lv {

namespace {

constexpr int SWAVES = 4;   // wavefronts per workgroup
constexpr int STHREADS = SWAVES * 64;
constexpr int STAT_BLOCKS = 256;

// what one wavefront needs to sum over its neighbours in order
struct WaveScratch {
    double o[SURF_MAX_K][3];
    double r[SURF_MAX_K];   // sqrt((double)d2): one square root per lane, then summed in neighbour order
};

// The reduction over a finished top-k (t.top ascending over the lanes: the n neighbours sit in lanes 0 .. n - 1)
__device__ __forceinline__ void surf_reduce(const MapView& map, const TopK& t, int lane, float px, float py, float pz, uint32_t id,
                                            const SurfRule& q, const uint32_t* __restrict__ rank, WaveScratch& s, double* __restrict__ val,
                                            float* __restrict__ mean_dist, int32_t* __restrict__ n_used) {
    const bool real = !is_none(t.top) && lane < t.k;
    const int n = __popcll(__ballot(real));
    wave_lds_fence();   // the previous point's readers are done
    if (real && q.job == 1) s.r[lane] = sqrt((double)__uint_as_float(key_hi(t.top)));
    if (real && q.job == 0) {
        const float4 x = map.orig[key_lo(t.top)];
        s.o[lane][0] = (double)x.x - (double)px;
        s.o[lane][1] = (double)x.y - (double)py;
        s.o[lane][2] = (double)x.z - (double)pz;
        s.r[lane] = sqrt((double)__uint_as_float(key_hi(t.top)));
    }
    wave_lds_fence();
    double dsum = 0.0;
    for (int j = 0; j < n; ++j) dsum += s.r[j];
    const double inf = (double)pos_inf();
    if (q.job == 1) {   // the point and k others, or it has no finite value
        if (lane == 0) val[id] = n == q.k ? dsum / (double)(n - 1) : inf;
        return;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < n; ++j) {
        sx += s.o[j][0];
        sy += s.o[j][1];
        sz += s.o[j][2];
    }
    const double dn = (double)n;
    const double mx = sx / dn, my = sy / dn, mz = sz / dn;
    // lane e of 0..5 owns C(a, b): (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    const int e = lane % 6;
    const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e : (e < 5 ? e - 2 : 2);
    const double ma = a == 0 ? mx : (a == 1 ? my : mz), mb = b == 0 ? mx : (b == 1 ? my : mz);
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc += (s.o[j][a] - ma) * (s.o[j][b] - mb);
    if (lane < 6) val[6 * (size_t)id + lane] = acc / dn;
    if (lane == 0) {
        const uint32_t r = rank_of(rank, id);
        mean_dist[r] = n > 1 ? (float)(dsum / (double)(n - 1)) : pos_inf();
        n_used[r] = n;
    }
}

// one wavefront per id: knn_ladder (RADIUS: the fixed-radius walk) for the map point `id`
template <bool RADIUS>
__global__ __launch_bounds__(STHREADS) void surf_ladder_kernel(MapView map, SurfRule q, const uint32_t* __restrict__ rank,
                                                               double* __restrict__ val,
                                                               float* __restrict__ mean_dist, int32_t* __restrict__ n_used) {
    __shared__ uint32_t s_pref[SWAVES][64], s_start[SWAVES][64];
    __shared__ WaveScratch s_ws[SWAVES];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const uint32_t id = blockIdx.x * (uint32_t)SWAVES + (uint32_t)w;
    if (id >= map.n_ids) return;   // (wavefront-uniform, as the dead ids below)
    const float4 P = map.orig[id];
    if (!pt_alive(P)) return;
    const float qx = P.x, qy = P.y, qz = P.z;
    const float max_d2 = q.max_dist * q.max_dist;
    const QGeom geo = make_geom(map, qx, qy, qz);
    if (RADIUS) {
        const float radius = q.max_dist;
        uint32_t got = 0;
        auto visit = [&](float x, float y, float z, uint32_t cid, bool ok) {
            const float d = calc_dist(qx, qy, qz, Xyz{x, y, z});
            got += (uint32_t)__popcll(__ballot(ok && admitted(d, max_d2) && cid != id));
        };
        stream_radius(map, radius_source(map, geo, qx, qy, qz, radius), geo, lane, s_pref[w], s_start[w], visit);
        if (lane == 0) val[id] = (double)got;
        return;
    }
    TopK t;
    t.k = q.k;
    t.reset();
    auto visit = [&](float x, float y, float z, uint32_t cid, bool ok) {
        const float d = calc_dist(qx, qy, qz, Xyz{x, y, z});
        t.offer(ok && admitted(d, max_d2) ? make_key(d, cid) : none_key(), lane);
    };
    knn_ladder(map, geo, t, max_d2, lane, s_pref[w], s_start[w], visit);
    surf_reduce(map, t, lane, qx, qy, qz, id, q, rank, s_ws[w], val, mean_dist, n_used);
}

// one lane per id: covariance -> normal and curvature at the living rank
__global__ __launch_bounds__(256) void surf_finish_kernel(const float4* __restrict__ orig, uint32_t n_ids, SurfRule q, const uint32_t* __restrict__ rank,
                                                          const double* __restrict__ val, const int32_t* __restrict__ n_used,
                                                          float* __restrict__ normals, float* __restrict__ curv) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_ids) return;
    const float4 p = orig[id];
    if (!pt_alive(p)) return;
    const uint32_t r = rank_of(rank, id);
    const double* c = val + 6 * (size_t)id;
    float n0, n1, n2, cv;
    surf_normal(c[0], c[1], c[2], c[3], c[4], c[5], n_used[r], q.min_neighbours, q.orient, q.viewpoint[0] - (double)p.x, q.viewpoint[1] - (double)p.y,
                q.viewpoint[2] - (double)p.z, n0, n1, n2, cv);
    normals[3 * (size_t)r] = n0;
    normals[3 * (size_t)r + 1] = n1;
    normals[3 * (size_t)r + 2] = n2;
    curv[r] = cv;
}

// part[2 b], part[2 b + 1] of block b: pass 0: sum of the finite values and their number; pass 1: sum of (value - mu)^2
__global__ __launch_bounds__(256) void surf_stat_kernel(const float4* __restrict__ orig, uint32_t n_ids, const double* __restrict__ val, double mu,
                                                        int pass, double* __restrict__ part) {
    __shared__ double s_s[256], s_c[256];
    double s = 0.0, c = 0.0;
    for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < n_ids; id += gridDim.x * blockDim.x) {
        if (!pt_alive(orig[id])) continue;
        const double v = val[id];
        if (!(v < (double)pos_inf())) continue;
        if (pass == 0) { s += v; c += 1.0; }
        else { const double d = v - mu; s += d * d; }
    }
    s_s[threadIdx.x] = s;
    s_c[threadIdx.x] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_s[threadIdx.x] += s_s[threadIdx.x + h];
            s_c[threadIdx.x] += s_c[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s_s[0];
        part[2 * blockIdx.x + 1] = s_c[0];
    }
}

// One lane per id.  Outlier: job 1: value > threshold; job 2: value < threshold (the count against min_neighbours).  flags
// (optional) at the point's rank; remove: the outliers go to the dead list (x, y, z, id) and read x = +inf from here on.
__global__ __launch_bounds__(256) void surf_classify_kernel(float4* __restrict__ orig, uint32_t n_ids, const double* __restrict__ val, int job,
                                                            double threshold, const uint32_t* __restrict__ rank, uint8_t* __restrict__ flags,
                                                            int remove, float4* __restrict__ dead, uint32_t dead_cap, MapCounters* cnt) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool gone = false;
    if (id < n_ids) p = orig[id];
    if (id < n_ids && pt_alive(p)) {
        const double v = val[id];
        const bool out = job == 1 ? v > threshold : v < threshold;
        if (flags) flags[rank_of(rank, id)] = out ? 1 : 0;
        gone = remove && out;
    }
    dead_list_append(gone, p, id, orig, dead, dead_cap, cnt);
}

}  // namespace

int SurfaceStore::ensure(size_t n_ids, size_t m, int job) {
    int rc = d_val.need((job == 0 ? 6 : 1) * n_ids);
    if (!rc) rc = d_flags.need(m);
    if (!rc && job == 0) {
        rc = d_normals.need(3 * m);
        if (!rc) rc = d_curv.need(m);
        if (!rc) rc = d_mean.need(m);
        if (!rc) rc = d_used.need(m);
    }
    if (!rc) rc = d_part.need(2 * STAT_BLOCKS);
    if (!rc) rc = h_part.need(2 * STAT_BLOCKS);
    return rc;
}

void SurfaceStore::release() {
    d_val.release(); d_part.release(); d_normals.release(); d_curv.release(); d_mean.release(); d_used.release(); d_flags.release();
    h_part.release();
    *this = SurfaceStore();
}

int surface_search(const MapStore& map, hipStream_t stream, SurfaceStore& st, const SurfRule& q, const uint32_t* rank) {
    const MapView v = map.view;
    if (!v.bt[0].table || v.m == 0 || map.n_ids == 0) return LV_OK;
    // (one wavefront per id: a launch takes fewer than 2^32 threads)
    if (map.n_ids > 0x03FFFFF0u) { set_error("map of %u ids: the surface search takes at most %u", map.n_ids, 0x03FFFFF0u); return LV_EINVAL; }
    if (q.job == 2) hipLaunchKernelGGL(surf_ladder_kernel<true>, dim3(blocks_of(map.n_ids, SWAVES)), dim3(STHREADS), 0, stream, v, q, rank, st.d_val, st.d_mean, st.d_used);
    else hipLaunchKernelGGL(surf_ladder_kernel<false>, dim3(blocks_of(map.n_ids, SWAVES)), dim3(STHREADS), 0, stream, v, q, rank, st.d_val, st.d_mean, st.d_used);
    LV_HIP(hipGetLastError());
    st.val_gen = map.gen;
    st.val_rule = q;
    return LV_OK;
}

int surface_finish(const MapStore& map, hipStream_t stream, SurfaceStore& st, const SurfRule& q, const uint32_t* rank) {
    if (map.n_ids == 0) return LV_OK;
    hipLaunchKernelGGL(surf_finish_kernel, dim3(blocks_of(map.n_ids, 256)), dim3(256), 0, stream, map.d_orig, map.n_ids, q, rank, st.d_val, st.d_used,
                       st.d_normals, st.d_curv);
    LV_HIP(hipGetLastError());
    return LV_OK;
}

// the block partials of one statistics pass, folded in block order
static int stat_pass(const MapStore& map, hipStream_t stream, SurfaceStore& st, double mu, int pass, double* sum, double* num) {
    hipLaunchKernelGGL(surf_stat_kernel, dim3(STAT_BLOCKS), dim3(256), 0, stream, map.d_orig, map.n_ids, st.d_val, mu, pass, st.d_part);
    LV_HIP(hipGetLastError());
    LV_HIP(hipMemcpyAsync(st.h_part, st.d_part, 2 * STAT_BLOCKS * sizeof(double), hipMemcpyDeviceToHost, stream));
    LV_HIP(hipStreamSynchronize(stream));
    double s = 0.0, c = 0.0;
    for (int b = 0; b < STAT_BLOCKS; ++b) { s += st.h_part[2 * b]; c += st.h_part[2 * b + 1]; }
    *sum = s;
    *num = c;
    return LV_OK;
}

int surface_outliers(MapStore& map, hipStream_t stream, SurfaceStore& st, SurfRule& q, const uint32_t* rank, bool want_flags, bool remove,
                     uint32_t* n_removed, double stats[3], bool reuse_values) {
    if (n_removed) *n_removed = 0;
    if (stats) stats[0] = stats[1] = stats[2] = 0.0;
    if (!map.built || map.m == 0) return LV_OK;
    int rc = st.ensure(map.n_ids, map.m, q.job);
    const bool have = reuse_values && st.val_gen == map.gen && st.val_rule.job == q.job && st.val_rule.k == q.k && st.val_rule.max_dist == q.max_dist;
    if (!rc && !have) rc = surface_search(map, stream, st, q, rank);
    if (rc) return rc;
    if (q.job == 1) {
        double mu = 0.0, sigma = 0.0;
        if (!q.fixed_threshold) {
            double s = 0.0, nf = 0.0, s2 = 0.0, unused = 0.0;
            rc = stat_pass(map, stream, st, 0.0, 0, &s, &nf);
            if (rc) return rc;
            mu = nf > 0.0 ? s / nf : 0.0;
            rc = stat_pass(map, stream, st, mu, 1, &s2, &unused);
            if (rc) return rc;
            sigma = nf > 1.0 ? std::sqrt(s2 / (nf - 1.0)) : 0.0;
            q.threshold = mu + (double)q.std_mul * sigma;
            q.fixed_threshold = 1;
        }
        if (stats) { stats[0] = mu; stats[1] = sigma; stats[2] = q.threshold; }
    }
    rc = map.ensure_counters();
    if (rc) return rc;
    rc = map.reset_batch_counters(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(surf_classify_kernel, dim3(blocks_of(map.n_ids, 256)), dim3(256), 0, stream, map.d_orig, map.n_ids, st.d_val, q.job, q.threshold,
                       rank, want_flags ? st.d_flags.p : nullptr, remove ? 1 : 0, map.d_dead, (uint32_t)map.d_dead.cap, map.d_cnt);
    LV_HIP(hipGetLastError());
    if (!remove) {
        LV_HIP(hipStreamSynchronize(stream));
        return LV_OK;
    }
    return map.retire_dead_list(stream, n_removed);
}

}  // namespace lv
