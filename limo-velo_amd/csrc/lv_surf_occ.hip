// lv_surf_occ.hip — the occupancy grid filled from the TSDF surface (include/limovelo_hip.h "Occupancy from the surface"; the rule's
// code is lv_surf_occ.hpp; DESIGN.md "Occupancy from the surface").
//
// Three passes on the context's stream, none with an atomic on the volume or the grid:
//   surf_occ_classify_kernel  one lane per TSDF voxel, 32 consecutive x per word as in OccStore::d_bits: the wavefront's two
//                             ballots are two whole words of the SOLID bitmap and two of the OPEN bitmap.
//   surf_occ_grow_kernel      reach > 0 only.  The cube of Chebyshev radius `reach` is separable: along x the SOLID words are OR-ed
//                             with themselves shifted by 1..reach bits either way, the carries coming from the two neighbouring
//                             words of the row; along y, then z, up to 2 * reach + 1 rows are OR-ed word by word.  One lane per word,
//                             one launch per axis, between the SOLID bitmap and a third one.
//   surf_occ_write_kernel     one wavefront per row (j, k) of the box, its lanes along x: what the row shares (j, k, the TSDF row its
//                             centres fall into) is worked out once per row, a voxel costs one quantisation, two bits, the mode's
//                             write rule and a store only where the 32 bits change.  A workgroup strides over its rows and adds
//                             its four counts as two packed words once (block_fold4).
// Passes 1 and 2 cover only the slab of the volume that the box can fall into (surf_occ_axis_range per axis, whole words in x),
// widened by `reach` where a pass reads its neighbours: a strip of the grid costs a strip of the volume.  Bits outside the slab
// are stale and are never read.
#include "lv_surf_occ.hpp"

#include "lv_host.hpp"
#include "lv_tsdf.hpp"

namespace lv {

namespace {

// words w0 .. w0 + nw - 1 of rows j0 .. j0 + nj - 1 of layers k0 .. k0 + nk - 1 of the volume's bitmaps
struct SurfSlab {
    int w0, nw, j0, nj, k0, nk;
};

// word w of the slab (x words fastest, then j, then k) as a word of the volume's bitmap, and where it lies
__device__ __forceinline__ uint32_t surf_occ_word(const OccGrid& tg, const SurfSlab& r, uint32_t w, int& xw, int& j, int& k) {
    const uint32_t row = w / (uint32_t)r.nw;
    xw = r.w0 + (int)(w - row * (uint32_t)r.nw);
    const uint32_t kk = row / (uint32_t)r.nj;
    j = r.j0 + (int)(row - kk * (uint32_t)r.nj);
    k = r.k0 + (int)kk;
    return ((uint32_t)k * (uint32_t)tg.ny + (uint32_t)j) * (uint32_t)tg.wx + (uint32_t)xw;
}

// n_words: the words of the slab.  A wavefront holds two of them, lanes 0..31 the first; a workgroup eight.
__global__ __launch_bounds__(256) void surf_occ_classify_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ W, OccGrid tg, SurfSlab r,
                                                                uint32_t n_words, int32_t min_weight, int32_t band, uint32_t* __restrict__ solid,
                                                                uint32_t* __restrict__ open) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t w = t >> 5;
    int cls = SURF_VOX_UNKNOWN;
    uint32_t word = 0;
    if (w < n_words) {
        int xw, j, k;
        word = surf_occ_word(tg, r, w, xw, j, k);
        const int i = xw * 32 + (int)(t & 31u);
        if (i < tg.nx) {
            const size_t at = grid_at(tg, i, j, k);
            cls = surf_occ_class_of_voxel(S[at], W[at], min_weight, band);
        }
    }
    const unsigned long long ms = __ballot(cls == SURF_VOX_SOLID), mo = __ballot(cls == SURF_VOX_OPEN);
    if (w < n_words && (t & 31u) == 0) {
        const int half = (int)(threadIdx.x & 32u);   // the wavefront's second word sits in the ballots' upper halves
        solid[word] = (uint32_t)(ms >> half);
        open[word] = (uint32_t)(mo >> half);
    }
}

// out = in grown by `reach` along `axis` over the slab r.  `in` is valid over r widened by reach rows along axis 1 or 2 (clipped to
// the volume); along x over the words v0..v1 alone: a word beyond them counts as empty (it lies further than `reach` from every bit
// that is read later).
__global__ __launch_bounds__(256) void surf_occ_grow_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, OccGrid tg, SurfSlab r,
                                                            uint32_t n_words, int reach, int axis, int v0, int v1) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n_words) return;
    int xw, j, k;
    const uint32_t word = surf_occ_word(tg, r, w, xw, j, k);
    uint32_t v = in[word];
    if (axis == 0) {
        const uint32_t prev = xw > v0 ? in[word - 1] : 0u, next = xw < v1 ? in[word + 1] : 0u, cur = v;
        for (int s = 1; s <= reach; ++s) v |= (cur << s) | (prev >> (32 - s)) | (cur >> s) | (next << (32 - s));
    } else {
        const int at = axis == 1 ? j : k, n = axis == 1 ? tg.ny : tg.nz;
        const uint32_t step = axis == 1 ? (uint32_t)tg.wx : (uint32_t)tg.wx * (uint32_t)tg.ny;
        for (int d = 1; d <= reach; ++d) {
            if (at - d >= 0) v |= in[word - (uint32_t)d * step];
            if (at + d < n) v |= in[word + (uint32_t)d * step];
        }
    }
    out[word] = v;
}

struct SurfBox {
    int lo[3];
};

// bd: the box's dimensions; a wavefront takes row (j, k) of the box, then the row 4 * gridDim.x further on.  stats[0] += OCCUPIED << 32
// | FREE, stats[1] += changed << 32 | OUTSIDE (each count below 2^28: the halves do not meet).
__global__ __launch_bounds__(256) void surf_occ_write_kernel(float* __restrict__ L, const uint32_t* __restrict__ grown, const uint32_t* __restrict__ open,
                                                             OccGrid og, OccGrid tg, SurfBox b, GridDims bd, int mode, float l_solid, float l_open,
                                                             unsigned long long* stats) {
    __shared__ unsigned long long sh[4][4];
    const float ca = surf_occ_clamped(l_solid, og.l_min, og.l_max), cb = surf_occ_clamped(l_open, og.l_min, og.l_max);
    const uint32_t n_rows = (uint32_t)bd.ny * (uint32_t)bd.nz, lane = threadIdx.x & 63u;
    unsigned long long classes = 0, edits = 0;
    for (uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6); row < n_rows; row += gridDim.x * 4u) {
        const uint32_t kk = row / (uint32_t)bd.ny;
        const int j = b.lo[1] + (int)(row - kk * (uint32_t)bd.ny), k = b.lo[2] + (int)kk;
        int uj = 0, uk = 0;
        const bool j_in = surf_occ_axis_of(og.origin[1], og.resolution, tg.origin[1], tg.resolution, tg.ny, j, uj);
        const bool row_in = surf_occ_axis_of(og.origin[2], og.resolution, tg.origin[2], tg.resolution, tg.nz, k, uk) && j_in;
        const uint32_t words = ((uint32_t)uk * (uint32_t)tg.ny + (uint32_t)uj) * (uint32_t)tg.wx;   // (read only where row_in)
        float* __restrict__ Lrow = L + grid_at(og, b.lo[0], j, k);
        for (uint32_t x = lane; x < (uint32_t)bd.nx; x += 64u) {
            int ui = 0, cls = SURF_OCC_NONE;
            if (surf_occ_axis_of(og.origin[0], og.resolution, tg.origin[0], tg.resolution, tg.nx, b.lo[0] + (int)x, ui) && row_in) {
                const uint32_t word = words + ((uint32_t)ui >> 5), bit = 1u << (ui & 31);
                if (grown[word] & bit) cls = SURF_OCC_OCCUPIED;
                else if (open[word] & bit) cls = SURF_OCC_FREE;
            } else {
                edits += 1ull;
            }
            classes += cls == SURF_OCC_OCCUPIED ? 1ull << 32 : (cls == SURF_OCC_FREE ? 1ull : 0ull);
            float v;
            if (surf_occ_write(mode, cls, Lrow[x], ca, cb, l_solid, l_open, og.l_min, og.l_max, v)) {
                Lrow[x] = v;
                edits += 1ull << 32;
            }
        }
    }
    unsigned long long a;
    if (block_fold4(sh, classes, edits, 0ull, 0ull, a) && threadIdx.x < 2 && a) atomicAdd(stats + threadIdx.x, a);
}

}  // namespace

// lo..hi: already clipped to the grid, not empty.  Reads t's S and W and writes nothing of it; waits for the stream.
int OccStore::from_surface(hipStream_t stream, const TsdfStore& t, const lv_occ_surface_params& p, const int lo[3], const int hi[3], uint64_t out[4]) {
    const OccGrid& tg = t.grid.occ;
    const size_t nw = (size_t)tg.wx * (size_t)tg.ny * (size_t)tg.nz;   // words of one bitmap of the volume
    int rc = d_sbits.need(3 * nw);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    uint32_t* solid = d_sbits.p;
    uint32_t* open = d_sbits.p + nw;
    uint32_t* spare = d_sbits.p + 2 * nw;
    const uint32_t* grown = solid;

    // the TSDF voxels the box can fall into, per axis; no bit is read where an axis has none (every voxel is then OUTSIDE)
    const int n[3] = {tg.nx, tg.ny, tg.nz};
    int u0[3], u1[3];
    bool any = true;
    for (int a = 0; a < 3; ++a) {
        surf_occ_axis_range(grid.origin[a], grid.resolution, tg.origin[a], tg.resolution, lo[a], hi[a], n[a], u0[a], u1[a]);
        any = any && u0[a] <= u1[a];
    }
    if (any) {
        const int reach = p.reach;
        // the slab widened by `by` voxels per axis, clipped to the volume; x in whole words
        auto slab_of = [&](int by_i, int by_j, int by_k) {
            int w0[3], w1[3];
            const int by[3] = {by_i, by_j, by_k};
            for (int a = 0; a < 3; ++a) {
                w0[a] = u0[a] - by[a] < 0 ? 0 : u0[a] - by[a];
                w1[a] = u1[a] + by[a] >= n[a] ? n[a] - 1 : u1[a] + by[a];
            }
            return SurfSlab{w0[0] >> 5, (w1[0] >> 5) - (w0[0] >> 5) + 1, w0[1], w1[1] - w0[1] + 1, w0[2], w1[2] - w0[2] + 1};
        };
        auto words_of = [](const SurfSlab& r) { return (uint32_t)((size_t)r.nw * (size_t)r.nj * (size_t)r.nk); };
        const SurfSlab all = slab_of(reach, reach, reach);
        const uint32_t n_all = words_of(all);
        hipLaunchKernelGGL(surf_occ_classify_kernel, dim3(blocks_of(n_all, 8)), dim3(256), 0, stream, (const int32_t*)t.d_S.p, (const int32_t*)t.d_W.p, tg, all,
                           n_all, (int32_t)p.min_weight, (int32_t)p.band, solid, open);
        if (reach) {
            const SurfSlab ry = slab_of(0, 0, reach), rz = slab_of(0, 0, 0);
            const int v0 = all.w0, v1 = all.w0 + all.nw - 1;
            hipLaunchKernelGGL(surf_occ_grow_kernel, dim3(blocks_of(n_all)), dim3(256), 0, stream, (const uint32_t*)solid, spare, tg, all, n_all, reach, 0, v0, v1);
            hipLaunchKernelGGL(surf_occ_grow_kernel, dim3(blocks_of(words_of(ry))), dim3(256), 0, stream, (const uint32_t*)spare, solid, tg, ry, words_of(ry), reach,
                               1, v0, v1);
            hipLaunchKernelGGL(surf_occ_grow_kernel, dim3(blocks_of(words_of(rz))), dim3(256), 0, stream, (const uint32_t*)solid, spare, tg, rz, words_of(rz), reach,
                               2, v0, v1);
            grown = spare;
        }
    }
    SurfBox b;
    for (int a = 0; a < 3; ++a) b.lo[a] = lo[a];
    const GridDims bd{hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1};
    const size_t n_rows = (size_t)bd.ny * (size_t)bd.nz;
    hipLaunchKernelGGL(surf_occ_write_kernel, dim3(grid_stride_blocks(64 * n_rows)), dim3(256), 0, stream, d_L.p, grown, (const uint32_t*)open, grid, tg, b, bd,
                       p.mode, p.l_solid, p.l_open, stats.d.p);
    LV_HIP(hipGetLastError());
    uint64_t st[4];
    rc = stats.read(stream, st);
    if (rc) return rc;
    out[0] = st[0] >> 32;
    out[1] = st[0] & 0xFFFFFFFFull;
    out[2] = st[1] >> 32;
    out[3] = st[1] & 0xFFFFFFFFull;
    return LV_OK;
}

}  // namespace lv
