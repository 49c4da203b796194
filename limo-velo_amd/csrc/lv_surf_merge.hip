// lv_surf_merge.hip — lv_surf_merge: a TSDF submap resampled into the volume under a rigid pose (include/limovelo_hip.h "Submap
// merging"; the rule's code is lv_surf_merge.hpp).
//
// One call, on the context's stream: the submap's S and W interleaved into pinned memory as (S, W) pairs and copied once, then ONE
// kernel:
//   surf_merge_kernel   one lane per destination voxel of the box of voxels the submap's box can reach (surf_merge_box).  A
//                       workgroup owns a tile of 16 x 4 x 4 voxels, a wavefront one z layer of it: 16 x 4 voxels, x fastest
//                       across lanes.  The wavefront's stores are four runs of 64 contiguous bytes in S and in W; its gather
//                       falls into a patch of about 17 x 5 x 2 source voxels at equal resolution, turned by the pose: under a
//                       yaw of 30 degrees some 12 source rows of one or two 128-byte lines (16 pairs) each, where a tile of
//                       64 x 1 would cross some 35 rows; the four wavefronts of a workgroup sit on top of each other, so a
//                       source layer one of them reads as its upper corners is the next one's lower corners, out of the same CU's
//                       cache.  A workgroup whose tile cannot meet the submap (surf_merge_tile_outside) leaves before it reads
//                       anything.  A lane runs steps 1 to 7 for its voxel, a corner one 8-byte load, and folds, reading and
//                       writing S and W only where dW > 0.  No atomics on the volume, no use of the scratch words: the voxel has
//                       one owner.  The four statistics are summed per wavefront, then per workgroup through LDS, and added with
//                       one 64-bit atomic per counter and workgroup.
// Neither shortcut changes a result: both are conservative by margins far above the f64 rounding of steps 2 and 3, and a voxel
// that is kept is judged by the full rule.  Nothing else depends on the launch geometry.
#include "lv_surf_merge.hpp"

#include <cstring>

namespace lv {

namespace {

// the voxels [x0, x1) x [y0, y1) x [z0, z1) of one launch
struct MergeBox {
    int x0, y0, z0, x1, y1, z1;
};

// grid (x tiles, y tiles, z tiles) of the box; sw: the staged submap; stats[0] += voxels not OUTSIDE, stats[1] += voxels with
// dW > 0, stats[2] += the sum of dW, stats[3] += voxels DROPPED
__global__ __launch_bounds__(256) void surf_merge_kernel(int32_t* __restrict__ S, int32_t* __restrict__ W, TsdfGrid g, MergeBox b, SurfMergeRule q,
                                                         const MergePair* __restrict__ sw, unsigned long long* stats) {
    __shared__ unsigned long long sh[4][4];
    const int i0 = b.x0 + (int)blockIdx.x * MERGE_TILE_X, j0 = b.y0 + (int)blockIdx.y * MERGE_TILE_Y, k0 = b.z0 + (int)blockIdx.z * MERGE_TILE_Z;
    const float res = g.occ.resolution;
    {   // (the same for every lane of the workgroup: all leave, or none)
        const int i1 = min(i0 + MERGE_TILE_X, b.x1) - 1, j1 = min(j0 + MERGE_TILE_Y, b.y1) - 1, k1 = min(k0 + MERGE_TILE_Z, b.z1) - 1;
        const float lo[3] = {colour_centre(g.occ.origin[0], res, i0), colour_centre(g.occ.origin[1], res, j0), colour_centre(g.occ.origin[2], res, k0)};
        const float hi[3] = {colour_centre(g.occ.origin[0], res, i1), colour_centre(g.occ.origin[1], res, j1), colour_centre(g.occ.origin[2], res, k1)};
        if (surf_merge_tile_outside(q, lo, hi)) return;
    }
    const int i = i0 + (int)(threadIdx.x & 15u), j = j0 + (int)((threadIdx.x >> 4) & 3u), k = k0 + (int)(threadIdx.x >> 6);
    uint32_t inside = 0, touched = 0, dropped = 0;
    unsigned long long added = 0;
    if (i < b.x1 && j < b.y1 && k < b.z1) {
        const float p[3] = {colour_centre(g.occ.origin[0], res, i), colour_centre(g.occ.origin[1], res, j), colour_centre(g.occ.origin[2], res, k)};
        int64_t dS, dW;
        const int st = surf_merge_voxel(q, g.T, p, sw, dS, dW);
        inside = st != MERGE_OUTSIDE;
        dropped = st == MERGE_KNOWN && dW == 0;
        if (dW > 0) {
            const size_t at = grid_at(g.occ, i, j, k);
            int32_t s = S[at], w = W[at];
            tsdf_fold(g.max_weight, dS, dW, s, w);
            S[at] = s;
            W[at] = w;
            touched = 1;
            added = (unsigned long long)dW;
        }
    }
    const unsigned long long sum[4] = {wave_sum((unsigned long long)inside), wave_sum((unsigned long long)touched), wave_sum(added),
                                       wave_sum((unsigned long long)dropped)};
    if ((threadIdx.x & 63u) == 0)
        for (int c = 0; c < 4; ++c) sh[threadIdx.x >> 6][c] = sum[c];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long a = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (a) atomicAdd(stats + threadIdx.x, a);
    }
}

}  // namespace

int TsdfStore::merge(hipStream_t stream, const lv_surf_submap& sub, const SurfMergeRule& q, const int lo[3], const int hi[3], uint64_t out[4]) {
    const size_t nv = (size_t)q.nx * (size_t)q.ny * (size_t)q.nz;
    // (every merge ends in stats.read, which waits for the stream: nothing of an earlier call still reads the two buffers)
    int rc = merged.d_sw.need(2 * nv);
    if (!rc) rc = merged.h_sw.need(2 * nv);
    if (!rc) rc = stats.zero(stream);
    if (rc) return rc;
    surf_merge_stage(sub, reinterpret_cast<MergePair*>(merged.h_sw.p));
    LV_HIP(hipMemcpyAsync(merged.d_sw, merged.h_sw, nv * sizeof(MergePair), hipMemcpyHostToDevice, stream));
    const MergeBox b{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    const dim3 tiles((uint32_t)((b.x1 - b.x0 + MERGE_TILE_X - 1) / MERGE_TILE_X), (uint32_t)((b.y1 - b.y0 + MERGE_TILE_Y - 1) / MERGE_TILE_Y),
                     (uint32_t)((b.z1 - b.z0 + MERGE_TILE_Z - 1) / MERGE_TILE_Z));
    hipLaunchKernelGGL(surf_merge_kernel, tiles, dim3(256), 0, stream, d_S.p, d_W.p, grid, b, q, reinterpret_cast<const MergePair*>(merged.d_sw.p), stats.d.p);
    LV_HIP(hipGetLastError());
    return stats.read(stream, out);   // (waits for the stream)
}

}  // namespace lv
