// lv_grid.hpp — the dense grid the occupancy tools share (lv_occupancy, lv_distance, lv_plan, lv_frontier): each rule of its
// arithmetic once (DESIGN.md "Grid helpers").
//
// The first part is plain __host__ __device__ code: the cell index with its inverse and inside test, the quantisation of a world
// coordinate, the cell of a world point, the projection of a column over a band of layers, and the LDS tile with a one-cell halo
// that the planner and the frontier labelling work in.  tests/emu/grid_emu.cpp compiles it with g++ through
// tests/emu/hip/hip_runtime.h and tests/test_grid_host.py holds it to numpy by equality.
// The rolling volumes' rule (the origin at an accumulated shift, the limits, the source cell of a shifted voxel, the box clip, the
// rule of a marked voxel: lv_volume_recentre, lv_occ_mark) is in that part too; tests/emu/recentre_emu.cpp and
// tests/test_recentre_host.py hold it to tests/recentre_ref.py.
// The second part (hipcc only) is the wavefront folds and what the kernels build from them.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define LV_OCC_HD __host__ __device__ inline

namespace lv {

// ---- cells.  G: any struct with nx, ny, nz (OccGrid, DistGrid, PlanGrid, FrontierGrid, PlanView, GridDims)
struct GridDims {
    int nx, ny, nz;
};

// the linear index: x runs fastest
template <class G>
LV_OCC_HD size_t grid_at(const G& g, int i, int j, int k) {
    return ((size_t)k * (size_t)g.ny + (size_t)j) * (size_t)g.nx + (size_t)i;
}

template <class G>
LV_OCC_HD bool grid_inside(const G& g, int i, int j, int k) {
    return (uint32_t)i < (uint32_t)g.nx && (uint32_t)j < (uint32_t)g.ny && (uint32_t)k < (uint32_t)g.nz;
}

// grid_at's inverse, in 32-bit arithmetic: a grid has at most 2^28 cells
template <class G>
LV_OCC_HD void grid_ijk(const G& g, uint32_t cell, int& i, int& j, int& k) {
    const uint32_t plane = (uint32_t)g.nx * (uint32_t)g.ny;
    const uint32_t c = cell / plane, r = cell - c * plane, b = r / (uint32_t)g.nx;
    i = (int)(r - b * (uint32_t)g.nx);
    j = (int)b;
    k = (int)c;
}

template <class G>
LV_OCC_HD size_t grid_cells(const G& g) {
    return (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
}

// ---- quantisation.  The order of the f32 operations is the contract with tests/occupancy_ref.py (-ffp-contract=off).
constexpr float OCC_SUB = 256.0f;            // sub-units per voxel (Q)
constexpr float OCC_Q_LIMIT = 16777216.0f;   // 2^24: a coordinate quantising to this or beyond is ignored

// The quantised coordinate as f32, before the cast: floorf(((p - origin) / resolution) * 256) in exactly that order
LV_OCC_HD float occ_quant_f(float p, float origin, float resolution) { return floorf(((p - origin) / resolution) * OCC_SUB); }

// false: non-finite, or too far to be cast (only a world point farther than 65536 voxels from the origin is)
LV_OCC_HD bool occ_quant(float p, float origin, float resolution, int32_t& q) {
    const float f = occ_quant_f(p, origin, resolution);
    if (!(fabsf(f) < OCC_Q_LIMIT)) return false;
    q = (int32_t)f;
    return true;
}

// The cell of world point p; false: a coordinate does not quantise, or the cell is outside the grid.  planar: z is neither
// quantised nor tested (it may be NaN) and k = 0.
template <class G>
LV_OCC_HD bool grid_cell_of(const G& g, const float origin[3], float resolution, bool planar, const float p[3], int& i, int& j, int& k) {
    int32_t q[3] = {0, 0, 0};
    bool ok = true;
    for (int a = 0; a < (planar ? 2 : 3); ++a) ok = occ_quant(p[a], origin[a], resolution, q[a]) && ok;
    if (!ok) return false;
    i = q[0] >> 8;
    j = q[1] >> 8;
    k = q[2] >> 8;   // (planar: 0, which is inside whatever nz)
    return grid_inside(g, i, j, k);
}

// ---- projection (lv_occ_project's rule; the planar distance field and the planar frontier run on it)
// the layers k_lo..k_hi clipped to the grid; k0 > k1: the band misses the grid
LV_OCC_HD void grid_clip_band(int k_lo, int k_hi, int nz, int& k0, int& k1) {
    k0 = k_lo < 0 ? 0 : k_lo;
    k1 = k_hi >= nz ? nz - 1 : k_hi;
}

// Column c of the plane over the clipped layers k0..k1: 100 if any L >= l_occ, else 0 if any L <= l_free, else -1 (NaN compares
// false twice; an empty band gives -1)
LV_OCC_HD int grid_project_column(const float* L, size_t plane, size_t c, int k0, int k1, float l_occ, float l_free) {
    bool occ = false, fre = false;
    for (int k = k0; k <= k1; ++k) {
        const float v = L[(size_t)k * plane + c];
        occ |= v >= l_occ;
        fre |= v <= l_free;
    }
    return occ ? 100 : fre ? 0 : -1;
}

// ---- rolling volumes (DESIGN.md "Rolling volumes"): a volume keeps the origin it was configured with and a whole-voxel shift s
constexpr int32_t GRID_SHIFT_LIMIT = 1 << 20;   // of one recentre and of the accumulated shift, per axis

// The origin at accumulated shift s: f32, unfused, in exactly this order.  A function of s alone, so no path leaves a residue.
LV_OCC_HD float grid_shift_origin(float origin0, int32_t s, float resolution) { return origin0 + (float)s * resolution; }

// A recentre by d of a volume at accumulated shift s.  NULL: legal, s_new and origin_new are filled; otherwise what is wrong
// (and nothing is to change).  d is tested before it is added: it may be any int32.
LV_OCC_HD const char* grid_shift_check(const float origin0[3], float resolution, const int32_t s[3], const int32_t d[3], int32_t s_new[3],
                                       float origin_new[3]) {
    for (int a = 0; a < 3; ++a)
        if (d[a] < -GRID_SHIFT_LIMIT || d[a] > GRID_SHIFT_LIMIT) return "shift: each component within +-2^20 voxels";
    for (int a = 0; a < 3; ++a) {
        s_new[a] = s[a] + d[a];
        if (s_new[a] < -GRID_SHIFT_LIMIT || s_new[a] > GRID_SHIFT_LIMIT) return "shift: the accumulated shift stays within +-2^20 voxels";
        origin_new[a] = grid_shift_origin(origin0[a], s_new[a], resolution);
        if (!(fabsf(origin_new[a]) < __builtin_huge_valf())) return "shift: the new origin must be finite";
    }
    return nullptr;
}

// The old voxel whose contents new voxel (i, j, k) takes after a recentre by (dx, dy, dz); false: it lies outside the grid and
// the new voxel is never observed
template <class G>
LV_OCC_HD bool grid_shift_source(const G& g, int32_t dx, int32_t dy, int32_t dz, int i, int j, int k, int& si, int& sj, int& sk) {
    si = i + dx;
    sj = j + dy;
    sk = k + dz;
    return grid_inside(g, si, sj, sk);
}

// The old voxel that new voxel (i, j, k) answers for when it is exposed: (i, j, k) mirrored in the grid.  c + d lies outside
// exactly when mirror(c) - d does, so the exposed new voxels and the old voxels that leave the volume pair off one to one.
template <class G>
LV_OCC_HD void grid_shift_mirror(const G& g, int i, int j, int k, int& mi, int& mj, int& mk) {
    mi = g.nx - 1 - i;
    mj = g.ny - 1 - j;
    mk = g.nz - 1 - k;
}

// the inclusive voxel box lo..hi clipped to the grid; false: nothing is left
template <class G>
LV_OCC_HD bool grid_clip_box(const G& g, const int lo[3], const int hi[3], int clo[3], int chi[3]) {
    const int n[3] = {g.nx, g.ny, g.nz};
    bool any = true;
    for (int a = 0; a < 3; ++a) {
        clo[a] = lo[a] < 0 ? 0 : lo[a];
        chi[a] = hi[a] >= n[a] ? n[a] - 1 : hi[a];
        any = any && clo[a] <= chi[a];
    }
    return any;
}

// lv_occ_mark's rule for a voxel that holds `count` points; true: L is rewritten.  observed: the voxel was a candidate and was
// left alone because it had been observed.
LV_OCC_HD bool grid_mark_voxel(uint32_t count, uint32_t min_points, bool only_unknown, float l_mark, float l_min, float l_max, float& L,
                               bool& candidate, bool& observed) {
    candidate = count >= min_points;
    observed = false;
    if (!candidate) return false;
    const bool unknown = L != L;
    if (only_unknown) {
        if (!unknown) {
            observed = true;
            return false;
        }
        L = fminf(fmaxf(l_mark, l_min), l_max);
        return true;
    }
    L = fminf(fmaxf((unknown ? 0.0f : L) + l_mark, l_min), l_max);
    return true;
}

// ---- A workgroup's tile of TX x TY x TZ cells with its one-cell halo, as it lies in LDS.  Local coordinates run -1 .. T.
template <int TX, int TY, int TZ>
struct HaloTile {
    static constexpr int HZ = TZ > 1 ? 1 : 0;   // a planar field has no halo in z
    static constexpr int LX = TX + 2, LY = TY + 2, LZ = TZ + 2 * HZ;
    static constexpr int CELLS = TX * TY * TZ, LCELLS = LX * LY * LZ;

    // the LDS slot of local cell (i, j, k); a neighbour's slot is at((i, j, k)) + (dz * LY + dy) * LX + dx
    LV_OCC_HD static int at(int i, int j, int k) { return ((k + HZ) * LY + (j + 1)) * LX + (i + 1); }

    // at's inverse: LDS slot l as an offset from the tile's origin
    LV_OCC_HD static void halo_of(int l, int& di, int& dj, int& dk) {
        di = l % LX - 1;
        dj = (l / LX) % LY - 1;
        dk = l / (LX * LY) - HZ;
    }

    // interior cell c = 0 .. CELLS - 1 (a lane's q-th cell is c = lane + q * 256), x fastest
    LV_OCC_HD static void local_of(int c, int& i, int& j, int& k) {
        i = c % TX;
        j = (c / TX) % TY;
        k = c / (TX * TY);
    }

    // the tiles that cover g form a grid themselves: grid_at / grid_inside / grid_ijk number them
    template <class G>
    LV_OCC_HD static GridDims tile_dims(const G& g) {
        return GridDims{(g.nx + TX - 1) / TX, (g.ny + TY - 1) / TY, (g.nz + TZ - 1) / TZ};
    }

    template <class G>
    LV_OCC_HD static size_t tiles(const G& g) {
        return grid_cells(tile_dims(g));
    }

    // tile t's coordinates among the tiles; its origin is the cell (tx * TX, ty * TY, tz * TZ)
    template <class G>
    LV_OCC_HD static void origin_of(const G& g, uint32_t t, int& tx, int& ty, int& tz) {
        grid_ijk(tile_dims(g), t, tx, ty, tz);
    }
};

#ifdef __HIPCC__

// ---- wavefront folds: every lane of the wavefront calls them, every lane gets the result
// over the aligned groups of G lanes (a power of two, 1..64): every lane gets its own group's result
template <int G, class T, class Op>
__device__ __forceinline__ T group_fold(T v, Op op) {
    for (int o = G / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
template <int G, class T>
__device__ __forceinline__ T group_min(T v) {
    return group_fold<G>(v, [](T a, T b) { return b < a ? b : a; });
}
template <class T, class Op>
__device__ __forceinline__ T wave_fold(T v, Op op) {
    return group_fold<64>(v, op);
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    return wave_fold(v, [](T a, T b) { return a + b; });
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
    return wave_fold(v, [](T a, T b) { return b < a ? b : a; });
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
    return wave_fold(v, [](T a, T b) { return b > a ? b : a; });
}

// wave-wide sum of a per-lane count, one 64-bit atomic (by lane 0) per wavefront that has anything to add
template <class T>
__device__ __forceinline__ void wave_add_to(unsigned long long* dst, T v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

// The workgroups of a launch that strides over its items and folds its counts once per workgroup (the recentre and mark passes):
// 8 workgroups of 256 lanes on each of the 256 CUs fill the chip; more would only add atomics on the counters
constexpr uint32_t GRID_STRIDE_BLOCKS = 2048;
__host__ inline uint32_t grid_stride_blocks(size_t items) {
    const size_t need = (items + 255) / 256;
    return (uint32_t)(need < GRID_STRIDE_BLOCKS ? need : GRID_STRIDE_BLOCKS);
}

// Two sums (s0, s1) and two maxima (m0, m1) over a workgroup of W wavefronts, per wavefront and then across them through sh.
// true in threads 0..3, where `out` is counter threadIdx.x of (s0, s1, m0, m1).  Integer folds: the order does not matter.
template <int W>
__device__ __forceinline__ bool block_fold4(unsigned long long (&sh)[W][4], unsigned long long s0, unsigned long long s1, unsigned long long m0,
                                            unsigned long long m1, unsigned long long& out) {
    const unsigned long long v[4] = {wave_sum(s0), wave_sum(s1), wave_max(m0), wave_max(m1)};
    if ((threadIdx.x & 63u) == 0)
        for (int c = 0; c < 4; ++c) sh[threadIdx.x >> 6][c] = v[c];
    __syncthreads();
    if (threadIdx.x >= 4) return false;
    const uint32_t c = threadIdx.x;
    unsigned long long a = sh[0][c];
    for (uint32_t w = 1; w < (uint32_t)W; ++w) a = c < 2 ? a + sh[w][c] : (sh[w][c] > a ? sh[w][c] : a);
    out = a;
    return true;
}

#endif   // __HIPCC__

}  // namespace lv
