// lv_volumes.hpp — the volume tools of a context: the occupancy grid, what is built from it (distance field, plan, frontier, the
// rays' packed states), what runs on those (rollouts, localisation), the TSDF volume with its mesh, and the rolling of both
// volumes.  lv_ctx holds one VolumeTools; every lv_occ_*, lv_tsdf_*, lv_depth_*, lv_colour_* and lv_volume_* entry point of lv_api.hip judges what it
// judges before the context, checks the context, and makes one call here.  Host code only: tests/emu/volumes_emu.cpp compiles
// it with g++ against tests/emu/hip/hip_runtime.h and its own stand-ins for the stores' member functions, and
// tests/test_volumes_host.py holds it to the rules below.
//
// WHAT MAKES WHAT STALE.  The products are snapshots: each shows its source as it was at the build.  "where built": a product
// that does not exist is not marked.  The code is this table; nothing else writes `stale`, `packed` or a product's `shift`
// (but the stores themselves: a build() clears `stale`, RayStore sets `packed`, a release() starts the store over).
//
//   event                                     | when                                        | effect
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   lv_occ_integrate, lv_occ_load (after its  | before the store call, whatever it returns  | GRID EDIT: ray.packed = false;
//     value check), lv_occ_clear              |                                             |   dist.stale = 1 and
//   lv_volume_recentre (OCC)                  | after success, and only for a non-zero      |   frontier.stale = 1 where built
//                                             |   shift (a zero shift touches no store and  |
//                                             |   zeroes stats)                             |
//   lv_occ_mark                               | after success, and only if it wrote a voxel |
//                                             |   (st[2] != 0)                              |
//   lv_occ_from_surface                       | after success, and only if it changed a     |
//                                             |   voxel's bits (st[2] != 0); it marks       |
//                                             |   nothing on the surface side               |
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   lv_occ_distance_build, _build_cells       | before the build, whatever it returns        | FIELD EDIT: plan.stale = 1
//     (after its plane-size check)            |                                             |   where built
//   lv_occ_distance_clear                     | after the synchronise and the release       |
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   lv_occ_plan_build (after its connectivity | before the store call, whatever it returns  | PLAN EDIT: lattice.stale = 1
//     check)                                  |                                             |   where built
//   lv_occ_plan_clear                         | after the synchronise and the release       |
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   a build of field, plan, frontier or       | after success only                          | dist.shift = occ.shift;
//     lattice                                 |                                             |   plan.shift = dist.shift;
//                                             |                                             |   frontier.shift = occ.shift;
//                                             |                                             |   lattice.shift = plan.shift
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   lv_occ_configure                          | after one hipStreamSynchronize              | releases dist, plan, frontier,
//                                             |                                             |   ray, rollout, mcl, lattice in
//                                             |                                             |   that order, then occ.configure
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   lv_tsdf_integrate, lv_tsdf_load (after    | before the store call                       | SURFACE EDIT: mesh.stale = 1
//     tsdf_check_volume), lv_tsdf_clear       |                                             |   where built
//   lv_volume_recentre (SURFACE)              | after success, non-zero shift               |
//   lv_depth_integrate (after its argument    | before the store call, whatever it returns  |
//     checks)                                 |                                             |
//   lv_surf_merge (after its argument checks, | before the box is looked at and before the  |   and, for lv_surf_merge, which
//     the volume and the resolution ratio)    |   store call, whatever it returns           |   TsdfStore::merge leaves to this
//                                             |                                             |   file: tsdf.rays.packed = false
//   ------------------------------------------+---------------------------------------------+---------------------------------
//   lv_colour_integrate (after its argument   | before the store call, whatever it returns  | COLOUR EDIT: mesh.stale = 1
//     checks), lv_colour_load (after its      |                                             |   where built
//     value check), lv_colour_clear (with a   |                                             |
//     layer)                                  |                                             |
//
// The colour layer lives inside TsdfStore, which looks after it in its own calls: load() and clear() zero it (colours of another
// volume mean nothing), integrate() leaves it alone, configure() and release() free it, recentre() moves it with S and W (new
// voxel (i, j, k) holds what (i + d) held, or four zeros; no surviving bit changes; a zero shift touches nothing), mesh_build()
// reads it for the vertex colours.  No call of the tables above gains a store call for it.
//
// A grid edit does not touch the plan: the plan shows the FIELD, and the field says of itself that it is stale.  In the same way
// a field edit or a grid edit does not touch the lattice: it shows the PLAN.
//
// WHAT A CALL ASKS FOR, in this order, after whatever its entry point judges before the context (LV_ESTATE and the message of
// the macros below unless said otherwise; then the arguments the entry point left, LV_EINVAL):
//   grid      every lv_occ_* call but lv_occ_configure: GRID.  lv_occ_integrate, _query, _load judge their arguments after it.
//   field     _build, _build_cells, _info, _clear: GRID.  _fetch, _query: GRID, FIELD.
//   plan      _build: GRID, FIELD, then the connectivity against the field (LV_EINVAL).  _fetch, _paths: GRID, PLAN.
//   frontier  _build: GRID.  _fetch, _clusters: GRID, FRONTIER.  _rank: GRID, FRONTIER, PLAN, then plan and frontier of one
//             shape, then frontier, plan and grid at one shift (both LV_ESTATE), then the capacity.
//   rays      GRID.
//   lattice   _build: GRID, PLAN, a planar plan (LV_ESTATE), then nx * ny * H <= 2^28 (LV_EINVAL).  _fetch, _paths: GRID, LATTICE,
//             then their arguments.  _info, _clear: GRID.
//   rollout   GRID, PLAN, a planar plan; with a footprint FIELD, then a planar field of the plan's nx, ny (all LV_ESTATE).
//   mcl       GRID, FIELD.
//   surface   every lv_tsdf_* call but lv_tsdf_configure: SURFACE, then its arguments.  lv_tsdf_mesh_fetch: SURFACE, MESH.
//   colour    every lv_colour_* call and lv_mesh_colours: SURFACE, then what is its own.  _integrate: band <= T (LV_EINVAL).
//             _fetch, _query: LAYER (LV_ESTATE), then the capacity.  _load: n and the values (LV_EINVAL).  _clear without a layer:
//             LV_OK, nothing done.  lv_mesh_colours: MESH, a mesh built with the layer present (both LV_ESTATE), the capacity.
//   surface rays  lv_surf_raycast, lv_surf_raycast_views: SURFACE; everything else was judged before the context.  They read the
//             volume, the layer and the store's packed states (which TsdfStore itself keeps: its integrate, load, clear and recentre
//             mark them not packed) and touch no `stale`.
//   surface registration  lv_surf_sample, lv_surf_align: SURFACE; everything else was judged before the context; reads the live
//             volume, marks nothing.
//   depth     lv_depth_integrate: SURFACE; everything else was judged before the context.  TsdfStore's integrate_depth marks the rays'
//             packed states not packed, as its integrate does, and leaves the colour layer alone.
//   rolling   lv_volume_recentre: the volume it names, then grid_shift_check (LV_EINVAL).  lv_volume_shift_info: nothing; a volume
//             that is not configured and a product that is not built (or whose grid is not configured) report zeros.
//   mark      GRID, then the box clipped to the grid (an empty one: LV_OK, zero stats, before the point map is looked at).
//   from surface  lv_occ_from_surface: GRID, SURFACE, then the box clipped to the grid (an empty one: LV_OK, zero stats, no store
//             call); the parameters were judged before the context.  It reads the live volume and writes nothing of it.
//   merge     lv_surf_merge: SURFACE, then the resolution ratio against the volume (surf_merge_scale, LV_EINVAL), then the marks of
//             the table, then the voxels the submap's box can reach (none: LV_OK, zero stats, no store call); everything else was
//             judged before the context.  It leaves the colour layer alone and touches nothing of the occupancy side.
#pragma once
#include <cstring>

#include "lv_colour.hpp"
#include "lv_distance.hpp"
#include "lv_frontier.hpp"
#include "lv_lattice.hpp"
#include "lv_mcl.hpp"
#include "lv_occupancy.hpp"
#include "lv_plan.hpp"
#include "lv_ray.hpp"
#include "lv_rollout.hpp"
#include "lv_rules.hpp"
#include "lv_surf_merge.hpp"
#include "lv_tsdf.hpp"

namespace lv {

// The states the methods below ask for
#define LV_GRID_CONFIGURED LV_REQUIRE(occ.configured, LV_ESTATE, "no occupancy grid: call lv_occ_configure first")
#define LV_DIST_BUILT LV_REQUIRE(dist.built, LV_ESTATE, "no distance field: call lv_occ_distance_build first")
#define LV_PLAN_BUILT LV_REQUIRE(plan.built, LV_ESTATE, "no plan: call lv_occ_plan_build first")
#define LV_FRONTIER_BUILT LV_REQUIRE(frontier.built, LV_ESTATE, "no frontier: call lv_occ_frontier_build first")
#define LV_LATTICE_BUILT LV_REQUIRE(lattice.built, LV_ESTATE, "no lattice: call lv_occ_lattice_build first")
#define LV_SURFACE_CONFIGURED LV_REQUIRE(tsdf.configured, LV_ESTATE, "no TSDF volume: call lv_tsdf_configure first")
#define LV_COLOUR_PRESENT LV_REQUIRE(tsdf.colour.present, LV_ESTATE, "no colour layer: call lv_colour_integrate or lv_colour_load first")

// What lv_distance_info, lv_plan_info and lv_frontier_info share; true: s is built (the caller adds what is its own)
template <class Info, class Store>
inline bool occ_fill_info(Info* out, const Store& s, bool planar) {
    *out = Info{};
    if (!s.built) return false;
    out->built = 1;
    out->planar = planar;
    out->nx = s.grid.nx;
    out->ny = s.grid.ny;
    out->nz = s.grid.nz;
    out->stale = s.stale;
    out->params = s.prm;
    return true;
}

struct VolumeTools {
    OccStore occ;             // lv_occ_*: the occupancy grid and its buffers (lv_occupancy.hip); nothing allocated before lv_occ_configure
    DistStore dist;           // lv_occ_distance_*: the distance field over that grid (lv_distance.hip); nothing allocated before the first build
    PlanStore plan;           // lv_occ_plan_*: the cost-to-go over that field (lv_plan.hip); nothing allocated before the first build
    FrontierStore frontier;   // lv_occ_frontier_*: the frontier clusters of that grid (lv_frontier.hip); nothing allocated before the first build
    RayStore ray;             // lv_occ_raycast / lv_occ_view_gain: the packed cell states of that grid (lv_ray.hip); nothing allocated before the first call
    RolloutStore rollout;     // lv_occ_rollout: its own buffers (lv_rollout.hip); nothing allocated before the first call
    MclStore mcl;             // lv_occ_mcl_weigh: its own buffers (lv_mcl.hip); nothing allocated before the first call
    LatticeStore lattice;     // lv_occ_lattice_*: the cost-to-go over (cell, heading) of the planar plan (lv_lattice.hip); nothing allocated before the first build
    TsdfStore tsdf;           // lv_tsdf_*: the TSDF volume, its mesh and its buffers (lv_tsdf.hip); nothing allocated before lv_tsdf_configure.
                              // lv_colour_*: its colour layer (lv_colour.hip); nothing allocated before the first lv_colour_integrate / _load

    // ---- the table's four edits and its stamps
    void grid_edited() {
        ray.packed = false;
        if (dist.built) dist.stale = 1;
        if (frontier.built) frontier.stale = 1;
    }
    void field_edited() {
        if (plan.built) plan.stale = 1;
    }
    void plan_edited() {
        if (lattice.built) lattice.stale = 1;
    }
    void surface_edited() {
        if (tsdf.mesh.built) tsdf.mesh.stale = 1;
    }
    void colour_edited() {
        if (tsdf.mesh.built) tsdf.mesh.stale = 1;
    }
    // a product remembers the accumulated shift of what it was built from ("Rolling volumes"); hands rc on
    static int built_at(int rc, int32_t product[3], const int32_t source[3]) {
        if (rc == LV_OK) std::memcpy(product, source, 3 * sizeof(int32_t));
        return rc;
    }

    // ---- Occupancy grid (lv_occupancy.hip)
    int occ_configure(hipStream_t stream, const lv_occupancy_params& p) {
        LV_HIP(hipStreamSynchronize(stream));
        dist.release();       // (the field belongs to the grid it was built from)
        plan.release();       // (and the plan to the field)
        frontier.release();   // (the frontier to the grid too)
        ray.release();        // (and the packed states)
        rollout.release();    // (and the rollouts' buffers)
        mcl.release();        // (and the localisation's)
        lattice.release();    // (the lattice belongs to the plan)
        return occ.configure(stream, p);
    }

    int occ_integrate(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        if (!views) { set_error("null argument"); return LV_EINVAL; }
        if (n_views < 1 || n_views > (size_t)OCC_MAX_VIEWS) { set_error("n_views = %zu: must be in 1..%d", n_views, OCC_MAX_VIEWS); return LV_EINVAL; }
        if (int rc = views_ok(views, n_views, "", false, 0xFFFFFFF0ull / 4)) return rc;   // (t is not judged: lv_rules.hpp)
        grid_edited();
        return occ.integrate(stream, views, n_views, stats);
    }

    int occ_query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* logodds) {
        LV_GRID_CONFIGURED;
        if (n && (!pts || !logodds || stride < 12)) { set_error("bad point array (stride %zu) or null output", stride); return LV_EINVAL; }
        if (n > 0xFFFFFFF0ull / 4) { set_error("too many points"); return LV_EINVAL; }
        return occ.query(stream, pts, stride, n, logodds);
    }

    int occ_project(hipStream_t stream, int k_lo, int k_hi, int8_t* grid2d, size_t capacity) {
        LV_GRID_CONFIGURED;
        const size_t plane = (size_t)occ.grid.nx * (size_t)occ.grid.ny;
        if (!grid2d || capacity < plane) { set_error("grid2d: room for nx * ny = %zu values needed", plane); return LV_EINVAL; }
        if (k_lo > k_hi) { set_error("layers %d..%d: k_lo <= k_hi", k_lo, k_hi); return LV_EINVAL; }
        return occ.project(stream, k_lo, k_hi, grid2d);
    }

    int occ_fetch(hipStream_t stream, float* logodds, size_t capacity) {
        LV_GRID_CONFIGURED;
        if (!logodds || capacity < occ.n_vox) { set_error("logodds: room for nx * ny * nz = %zu values needed", occ.n_vox); return LV_EINVAL; }
        return occ.fetch(stream, logodds);
    }

    int occ_load(hipStream_t stream, const float* logodds, size_t n) {
        LV_GRID_CONFIGURED;
        if (!logodds || n != occ.n_vox) { set_error("lv_occ_load: %zu values for a grid of %zu voxels", n, occ.n_vox); return LV_EINVAL; }
        const float lo = occ.prm.l_min, hi = occ.prm.l_max;
        for (size_t i = 0; i < n; ++i) {
            const float v = logodds[i];
            if (!(v != v) && !(v >= lo && v <= hi)) { set_error("lv_occ_load: value %g at %zu outside [%g, %g]", v, i, lo, hi); return LV_EINVAL; }
        }
        grid_edited();
        return occ.load(stream, logodds);
    }

    int occ_clear(hipStream_t stream) {
        LV_GRID_CONFIGURED;
        grid_edited();
        return occ.clear(stream);
    }

    int occ_get_params(lv_occupancy_params* out) {
        LV_GRID_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        *out = occ.prm;
        return LV_OK;
    }

    // lv_occ_mark, first half: the box clipped to the grid.  *any false: nothing to mark, stats are zeroed and the call is over
    // (the point map is not settled or polled for it)
    int occ_mark_box(const lv_occ_mark_params& p, int lo[3], int hi[3], uint64_t stats[4], bool* any) {
        LV_GRID_CONFIGURED;
        *any = grid_clip_box(occ.grid, p.lo, p.hi, lo, hi);
        if (!*any && stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
        return LV_OK;
    }

    // ... second half: the caller's points, or without them (pts null) the point map's as lv_api.hip read them
    int occ_mark(hipStream_t stream, const lv_occ_mark_params& p, const int lo[3], const int hi[3], const void* map_orig, uint32_t n_ids,
                 const void* pts, size_t stride, size_t n, uint64_t stats[4]) {
        uint64_t st[4] = {0, 0, 0, 0};
        const int rc = pts ? occ.mark(stream, p, lo, hi, nullptr, 0, pts, stride, n, st) : occ.mark(stream, p, lo, hi, map_orig, n_ids, nullptr, 0, 0, st);
        if (rc) return rc;
        if (st[2]) grid_edited();
        if (stats)
            for (int i = 0; i < 4; ++i) stats[i] = st[i];
        return LV_OK;
    }

    // ---- Occupancy from the surface (lv_surf_occ.hip).  Only this method reaches the store's from_surface.  Its entry point has
    // judged the parameters (surf_occ_check_params).
    int occ_from_surface(hipStream_t stream, const lv_occ_surface_params& p, uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        LV_SURFACE_CONFIGURED;
        uint64_t st[4] = {0, 0, 0, 0};
        int lo[3], hi[3];
        if (grid_clip_box(occ.grid, p.lo, p.hi, lo, hi)) {
            if (int rc = occ.from_surface(stream, tsdf, p, lo, hi, st)) return rc;
            if (st[2]) grid_edited();
        }
        if (stats)
            for (int i = 0; i < 4; ++i) stats[i] = st[i];
        return LV_OK;
    }

    // ---- Distance field (lv_distance.hip)
    int distance_build(hipStream_t stream, const lv_distance_params& p, uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        field_edited();
        return built_at(dist.build(stream, occ, p, nullptr, stats), dist.shift, occ.shift);
    }

    // The planar distance field over the caller's cells ("Elevation map": distance from cells); everything but the source of the
    // obstacles is lv_occ_distance_build's
    int distance_build_cells(hipStream_t stream, const lv_distance_params& p, const int8_t* cells, size_t n, uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        const size_t plane = (size_t)occ.grid.nx * (size_t)occ.grid.ny;
        if (n != plane) { set_error("lv_occ_distance_build_cells: %zu cells for a plane of nx * ny = %zu", n, plane); return LV_EINVAL; }
        field_edited();
        return built_at(dist.build(stream, occ, p, cells, stats), dist.shift, occ.shift);
    }

    int distance_fetch(hipStream_t stream, int32_t* s2, float* metres, size_t capacity) {
        LV_GRID_CONFIGURED;
        LV_DIST_BUILT;
        if (capacity < dist.n_vox) { set_error("lv_occ_distance_fetch: room for %zu values needed", dist.n_vox); return LV_EINVAL; }
        return dist.fetch(stream, s2, metres);
    }

    int distance_query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* d, float* grad) {
        LV_GRID_CONFIGURED;
        LV_DIST_BUILT;
        if (n && (!pts || !d || stride < 12)) { set_error("bad point array (stride %zu) or null output", stride); return LV_EINVAL; }
        if (n > 0xFFFFFFF0ull / 4) { set_error("too many points"); return LV_EINVAL; }
        return dist.query(stream, pts, stride, n, d, grad);
    }

    int distance_info(lv_distance_info* out) {
        LV_GRID_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        occ_fill_info(out, dist, dist.prm.planar != 0);
        return LV_OK;
    }

    int distance_clear(hipStream_t stream) {
        LV_GRID_CONFIGURED;
        LV_HIP(hipStreamSynchronize(stream));
        dist.release();
        field_edited();
        return LV_OK;
    }

    // ---- Planner (lv_plan.hip)
    int plan_build(hipStream_t stream, const lv_plan_params& p, const uint8_t* cost, size_t n_cost, const void* goals, size_t stride, size_t n_goals,
                   uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        LV_DIST_BUILT;
        if (const char* why = plan_check_field(p.connectivity, dist.prm.planar != 0)) { set_error("lv_occ_plan_build: %s", why); return LV_EINVAL; }
        plan_edited();
        return built_at(plan.build(stream, dist, p, cost, n_cost, goals, stride, n_goals, stats), plan.shift, dist.shift);   // (the plan lies where its field does)
    }

    int plan_fetch(hipStream_t stream, uint32_t* potential, uint8_t* cell_cost, size_t capacity) {
        LV_GRID_CONFIGURED;
        LV_PLAN_BUILT;
        if (capacity < plan.n_cells) { set_error("lv_occ_plan_fetch: room for %zu values needed", plan.n_cells); return LV_EINVAL; }
        return plan.fetch(stream, potential, cell_cost);
    }

    int plan_paths(hipStream_t stream, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets, int32_t* cells,
                   size_t capacity, size_t* total) {
        LV_GRID_CONFIGURED;
        LV_PLAN_BUILT;
        if (!offsets || !total || (n && (!starts || !status || !cost || stride < 12))) {
            set_error("bad start array (stride %zu) or null status / cost / offsets / total", stride);
            return LV_EINVAL;
        }
        if (n >= (size_t)0x7FFFFFFF) { set_error("%zu starts: one call takes fewer than 2^31 - 1", n); return LV_EINVAL; }
        return plan.paths(stream, starts, stride, n, status, cost, offsets, cells, capacity, total);
    }

    int plan_info(lv_plan_info* out) {
        LV_GRID_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        if (occ_fill_info(out, plan, plan.grid.planar != 0)) out->rounds = plan.rounds;
        return LV_OK;
    }

    int plan_clear(hipStream_t stream) {
        LV_GRID_CONFIGURED;
        LV_HIP(hipStreamSynchronize(stream));
        plan.release();
        plan_edited();
        return LV_OK;
    }

    // ---- Lattice planner (lv_lattice.hip).  Only these methods reach the store's out-of-line members.
    int lattice_build(hipStream_t stream, const lv_lattice_params& p, const lv_lattice_prim* prims, const void* goals, size_t stride, size_t n_goals,
                      uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        LV_PLAN_BUILT;
        const PlanGrid& g = plan.grid;
        if (!g.planar) { set_error("lv_occ_lattice_build: the plan is 3-D: the lattice runs on a planar plan"); return LV_ESTATE; }
        const size_t n_states = (size_t)g.nx * (size_t)g.ny * (size_t)p.H;
        if (n_states > LAT_MAX_STATES) { set_error("lv_occ_lattice_build: nx * ny * H = %zu states: at most 2^28", n_states); return LV_EINVAL; }
        return built_at(lattice.build(stream, plan, p, prims, goals, stride, n_goals, stats), lattice.shift, plan.shift);   // (the lattice lies where its plan does)
    }

    int lattice_fetch(hipStream_t stream, uint32_t* V, size_t capacity) {
        LV_GRID_CONFIGURED;
        LV_LATTICE_BUILT;
        if (capacity < lattice.n_states) { set_error("lv_occ_lattice_fetch: room for %zu values needed", lattice.n_states); return LV_EINVAL; }
        return lattice.fetch(stream, V);
    }

    int lattice_paths(hipStream_t stream, const void* starts, size_t stride, size_t n, int32_t* status, uint32_t* cost, size_t* offsets, int32_t* states,
                      uint8_t* prims, size_t capacity, size_t* total) {
        LV_GRID_CONFIGURED;
        LV_LATTICE_BUILT;
        if (!offsets || !total || (n && (!starts || !status || !cost || stride < 16))) {
            set_error("lv_occ_lattice_paths: bad start array (stride %zu) or null status / cost / offsets / total", stride);
            return LV_EINVAL;
        }
        if (n >= (size_t)0x7FFFFFFF) { set_error("lv_occ_lattice_paths: %zu starts: one call takes fewer than 2^31 - 1", n); return LV_EINVAL; }
        return lattice.paths(stream, starts, stride, n, status, cost, offsets, states, prims, capacity, total);
    }

    int lattice_info(lv_lattice_info* out) {
        LV_GRID_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        *out = lv_lattice_info{};
        if (!lattice.built) return LV_OK;
        out->built = 1;
        out->nx = lattice.grid.nx;
        out->ny = lattice.grid.ny;
        out->H = lattice.grid.H;
        out->P = lattice.grid.P;
        out->stale = lattice.stale;
        out->rounds = lattice.rounds;
        out->tile = lattice.tile;
        out->reach = lattice.reach;
        out->params = lattice.prm;
        return LV_OK;
    }

    int lattice_clear(hipStream_t stream) {
        LV_GRID_CONFIGURED;
        LV_HIP(hipStreamSynchronize(stream));
        lattice.release();
        return LV_OK;
    }

    // ---- Frontiers (lv_frontier.hip)
    int frontier_build(hipStream_t stream, const lv_frontier_params& p, uint64_t stats[4]) {
        LV_GRID_CONFIGURED;
        return built_at(frontier.build(stream, occ, p, stats), frontier.shift, occ.shift);
    }

    int frontier_fetch(hipStream_t stream, int32_t* labels, size_t capacity) {
        LV_GRID_CONFIGURED;
        LV_FRONTIER_BUILT;
        if (capacity < frontier.n_cells) { set_error("lv_occ_frontier_fetch: room for %zu values needed", frontier.n_cells); return LV_EINVAL; }
        return frontier.fetch(stream, labels);
    }

    int frontier_clusters(hipStream_t stream, lv_frontier_cluster* out, size_t capacity, size_t* n) {
        LV_GRID_CONFIGURED;
        LV_FRONTIER_BUILT;
        *n = frontier.n_clusters;
        if (!out) return LV_OK;   // count only
        if (capacity < frontier.n_clusters) { set_error("capacity %zu < %zu clusters", capacity, frontier.n_clusters); return LV_EINVAL; }
        return frontier.clusters(stream, out);
    }

    int frontier_rank(hipStream_t stream, int reach, uint32_t* best_p, int32_t* best_cell, size_t capacity) {
        LV_GRID_CONFIGURED;
        LV_FRONTIER_BUILT;
        LV_PLAN_BUILT;
        const FrontierGrid& f = frontier.grid;
        const PlanGrid& g = plan.grid;
        if ((f.planar != 0) != (g.planar != 0) || f.nx != g.nx || f.ny != g.ny || f.nz != g.nz) {
            set_error("lv_occ_frontier_rank: the plan (%d x %d x %d, planar %d) is not of the frontier's cells (%d x %d x %d, planar %d)", g.nx, g.ny, g.nz,
                      g.planar, f.nx, f.ny, f.nz, f.planar);
            return LV_ESTATE;
        }
        // (cell indices of different boxes do not pair, and the cells handed back are read in the grid's box of now)
        if (std::memcmp(frontier.shift, plan.shift, sizeof(plan.shift)) != 0 || std::memcmp(frontier.shift, occ.shift, sizeof(occ.shift)) != 0) {
            set_error("lv_occ_frontier_rank: the frontier was built at grid shift (%d, %d, %d), the plan at (%d, %d, %d), the grid is at (%d, %d, %d): "
                      "rebuild the field, the plan and the frontier", frontier.shift[0], frontier.shift[1], frontier.shift[2], plan.shift[0],
                      plan.shift[1], plan.shift[2], occ.shift[0], occ.shift[1], occ.shift[2]);
            return LV_ESTATE;
        }
        if (capacity < frontier.n_clusters) { set_error("capacity %zu < %zu clusters", capacity, frontier.n_clusters); return LV_EINVAL; }
        return frontier.rank(stream, plan, reach, best_p, best_cell);
    }

    int frontier_info(lv_frontier_info* out) {
        LV_GRID_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        if (occ_fill_info(out, frontier, frontier.grid.planar != 0)) out->n_clusters = (int)frontier.n_clusters;
        return LV_OK;
    }

    int frontier_clear(hipStream_t stream) {
        LV_GRID_CONFIGURED;
        LV_HIP(hipStreamSynchronize(stream));
        frontier.release();
        return LV_OK;
    }

    // ---- Ray casting (lv_ray.hip)
    int raycast(hipStream_t stream, const lv_ray_params& p, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                lv_ray_result* out) {
        LV_GRID_CONFIGURED;
        return ray.raycast(stream, occ, p, from, from_stride, to, to_stride, n, out);
    }

    int view_gain(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t* gain) {
        LV_GRID_CONFIGURED;
        return ray.view_gain(stream, occ, views, n_views, gain);
    }

    // ---- Rollouts (lv_rollout.hip)
    int rollout_run(hipStream_t stream, const lv_rollout_params& p, const float* start, const float* controls, size_t K, const float* footprint,
                    size_t n_fp, lv_rollout_result* results, float* poses, uint64_t* score, int64_t* best) {
        LV_GRID_CONFIGURED;
        LV_PLAN_BUILT;
        const PlanGrid& g = plan.grid;
        if (!g.planar) { set_error("lv_occ_rollout: the plan is 3-D: rollouts run on a planar plan"); return LV_ESTATE; }
        if (n_fp) {
            LV_DIST_BUILT;
            const DistGrid& f = dist.grid;
            if (!dist.prm.planar || f.nx != g.nx || f.ny != g.ny) {
                set_error("lv_occ_rollout: the distance field (%d x %d, planar %d) is not of the plan's cells (%d x %d, planar)", f.nx, f.ny,
                          dist.prm.planar, g.nx, g.ny);
                return LV_ESTATE;
            }
        }
        return rollout.run(stream, plan, dist, p, start, controls, K, footprint, n_fp, results, poses, score, best);
    }

    // ---- Localisation (lv_mcl.hip)
    int mcl_weigh(hipStream_t stream, const lv_mcl_params& p, const float* poses, size_t K, const float* beams, size_t B, const uint32_t* table,
                  size_t n_table, uint64_t* score, uint32_t* n_in, int64_t* best) {
        LV_GRID_CONFIGURED;
        LV_DIST_BUILT;
        return mcl.run(stream, dist, p, poses, K, beams, B, table, n_table, score, n_in, best);
    }

    // ---- TSDF and mesh (lv_tsdf.hip)
    int tsdf_configure(hipStream_t stream, const lv_tsdf_params& p) { return tsdf.configure(stream, p); }

    int tsdf_integrate(hipStream_t stream, const lv_view* views, size_t n_views, uint64_t stats[4]) {
        LV_SURFACE_CONFIGURED;
        if (!views) { set_error("lv_tsdf_integrate: null argument"); return LV_EINVAL; }
        if (n_views < 1 || n_views > (size_t)OCC_MAX_VIEWS) { set_error("lv_tsdf_integrate: n_views = %zu: must be in 1..%d", n_views, OCC_MAX_VIEWS); return LV_EINVAL; }
        if (int rc = views_ok(views, n_views, "lv_tsdf_integrate: ", false, TSDF_MAX_RETURNS)) return rc;   // (t is not judged: lv_rules.hpp)
        surface_edited();
        return tsdf.integrate(stream, views, n_views, stats);
    }

    int tsdf_query(hipStream_t stream, const void* pts, size_t stride, size_t n, float* metres, int32_t* weight) {
        LV_SURFACE_CONFIGURED;
        if (!metres && !weight) { set_error("lv_tsdf_query: metres and weight are both null"); return LV_EINVAL; }
        if (n && (!pts || stride < 12)) { set_error("lv_tsdf_query: bad point array (stride %zu)", stride); return LV_EINVAL; }
        if (n > 0xFFFFFFF0ull / 4) { set_error("lv_tsdf_query: too many points"); return LV_EINVAL; }
        return tsdf.query(stream, pts, stride, n, metres, weight);
    }

    int tsdf_fetch(hipStream_t stream, int32_t* S, int32_t* W, float* metres, size_t capacity) {
        LV_SURFACE_CONFIGURED;
        if (!S && !W && !metres) { set_error("lv_tsdf_fetch: S, W and metres are all null"); return LV_EINVAL; }
        if (capacity < tsdf.n_vox) { set_error("lv_tsdf_fetch: room for nx * ny * nz = %zu values needed", tsdf.n_vox); return LV_EINVAL; }
        return tsdf.fetch(stream, S, W, metres);
    }

    int tsdf_load(hipStream_t stream, const int32_t* S, const int32_t* W, size_t n) {
        LV_SURFACE_CONFIGURED;
        if (!S || !W || n != tsdf.n_vox) { set_error("lv_tsdf_load: %zu values for a volume of %zu voxels, or a null array", n, tsdf.n_vox); return LV_EINVAL; }
        const size_t bad = tsdf_check_volume(tsdf.grid, S, W, n);
        if (bad != n) {
            set_error("lv_tsdf_load: voxel %zu: S = %d, W = %d: 0 <= W <= max_weight and |S| <= T * W", bad, S[bad], W[bad]);
            return LV_EINVAL;
        }
        surface_edited();
        return tsdf.load(stream, S, W);
    }

    int tsdf_clear(hipStream_t stream) {
        LV_SURFACE_CONFIGURED;
        surface_edited();
        return tsdf.clear(stream);
    }

    int tsdf_get_params(lv_tsdf_params* out) {
        LV_SURFACE_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        *out = tsdf.prm;
        return LV_OK;
    }

    int mesh_build(hipStream_t stream, int min_weight, uint64_t counts[4]) {
        LV_SURFACE_CONFIGURED;
        if (min_weight < 1) { set_error("lv_tsdf_mesh_build: min_weight = %d: at least 1", min_weight); return LV_EINVAL; }
        return tsdf.mesh_build(stream, min_weight, counts);
    }

    int mesh_fetch(hipStream_t stream, float* xyz, int32_t* sub, uint32_t* tri, size_t cap_vertices, size_t cap_triangles) {
        LV_SURFACE_CONFIGURED;
        LV_REQUIRE(tsdf.mesh.built, LV_ESTATE, "no mesh: call lv_tsdf_mesh_build first");
        if (!xyz && !sub && !tri) { set_error("lv_tsdf_mesh_fetch: xyz, sub and tri are all null"); return LV_EINVAL; }
        const TsdfMesh& m = tsdf.mesh;
        if ((xyz || sub) && cap_vertices < m.counts[0]) { set_error("lv_tsdf_mesh_fetch: room for %llu vertices needed", (unsigned long long)m.counts[0]); return LV_EINVAL; }
        if (tri && cap_triangles < m.counts[1]) { set_error("lv_tsdf_mesh_fetch: room for %llu triangles needed", (unsigned long long)m.counts[1]); return LV_EINVAL; }
        return tsdf.mesh_fetch(stream, xyz, sub, tri);
    }

    int mesh_info(lv_mesh_info* out) {
        LV_SURFACE_CONFIGURED;
        if (!out) { set_error("null argument"); return LV_EINVAL; }
        const TsdfMesh& m = tsdf.mesh;
        *out = lv_mesh_info{};
        if (!m.built) return LV_OK;
        out->built = 1;
        out->stale = m.stale;
        out->min_weight = m.min_weight;
        out->vertices = m.counts[0];
        out->triangles = m.counts[1];
        out->active_cells = m.counts[2];
        out->refused_edges = m.counts[3];
        out->reserved = m.coloured ? 1 : 0;
        return LV_OK;
    }

    int mesh_clear(hipStream_t stream) {
        LV_SURFACE_CONFIGURED;
        LV_HIP(hipStreamSynchronize(stream));
        tsdf.mesh_release();
        return LV_OK;
    }

    // ---- Depth fusion (lv_depth.hip).  Only this method reaches the store's integrate_depth.  Its entry point has judged what
    // needs no context: null arguments, the views and parameters (depth_rule).
    int depth_integrate(hipStream_t stream, const lv_depth_view* views, const DepthCam* cams, const DepthRule& q, uint64_t stats[4]) {
        LV_SURFACE_CONFIGURED;
        surface_edited();
        return tsdf.integrate_depth(stream, views, cams, q, stats);
    }

    // ---- Colour layer (lv_colour.hip).  Only these methods reach the store's colour members.  Their entry points have judged
    // what needs no context: null arguments, the views and parameters (colour_rule), the point array.
    int colour_integrate(hipStream_t stream, const lv_camera_view* views, const PaintCam* cams, const PaintRule& q, const lv_colour_params& p,
                         uint64_t stats[4]) {
        LV_SURFACE_CONFIGURED;
        if (p.band > tsdf.grid.T) { set_error("lv_colour_integrate: band = %d: must be in 1..T = %d", p.band, tsdf.grid.T); return LV_EINVAL; }
        colour_edited();
        return tsdf.colour_integrate(stream, views, cams, q, p.band, p.min_weight, p.max_weight, stats);
    }

    int colour_fetch(hipStream_t stream, uint32_t* sums, uint8_t* rgba, size_t capacity) {
        LV_SURFACE_CONFIGURED;
        LV_COLOUR_PRESENT;
        if (capacity < tsdf.n_vox) { set_error("lv_colour_fetch: room for nx * ny * nz = %zu voxels needed", tsdf.n_vox); return LV_EINVAL; }
        return tsdf.colour_fetch(stream, sums, rgba);
    }

    int colour_load(hipStream_t stream, const uint32_t* sums, size_t n) {
        LV_SURFACE_CONFIGURED;
        if (n != tsdf.n_vox) { set_error("lv_colour_load: %zu voxels for a volume of %zu", n, tsdf.n_vox); return LV_EINVAL; }
        const size_t bad = colour_check_layer(sums, n);
        if (bad != n) {
            set_error("lv_colour_load: voxel %zu: C = %u, %u, %u, Wc = %u: Wc <= 65535 and C <= 255 * Wc", bad, sums[4 * bad], sums[4 * bad + 1],
                      sums[4 * bad + 2], sums[4 * bad + 3]);
            return LV_EINVAL;
        }
        colour_edited();
        return tsdf.colour_load(stream, sums);
    }

    int colour_query(hipStream_t stream, const void* pts, size_t stride, size_t n, uint8_t* rgba) {
        LV_SURFACE_CONFIGURED;
        LV_COLOUR_PRESENT;
        return tsdf.colour_query(stream, pts, stride, n, rgba);
    }

    int colour_clear(hipStream_t stream) {
        LV_SURFACE_CONFIGURED;
        if (!tsdf.colour.present) return LV_OK;
        colour_edited();
        return tsdf.colour_clear(stream);
    }

    int colour_info(hipStream_t stream, struct lv_colour_info* out) {
        LV_SURFACE_CONFIGURED;
        *out = {};
        out->voxels = tsdf.n_vox;
        if (!tsdf.colour.present) return LV_OK;
        out->present = 1;
        return tsdf.colour_count(stream, &out->coloured);
    }

    int mesh_colours(hipStream_t stream, uint8_t* rgba, size_t cap_vertices) {
        LV_SURFACE_CONFIGURED;
        LV_REQUIRE(tsdf.mesh.built, LV_ESTATE, "no mesh: call lv_tsdf_mesh_build first");
        LV_REQUIRE(tsdf.mesh.coloured, LV_ESTATE, "the mesh was built without a colour layer: call lv_tsdf_mesh_build after lv_colour_integrate");
        if (cap_vertices < tsdf.mesh.counts[0]) { set_error("lv_mesh_colours: room for %llu vertices needed", (unsigned long long)tsdf.mesh.counts[0]); return LV_EINVAL; }
        return tsdf.mesh_colours(stream, rgba);
    }

    // ---- Surface ray casting (lv_tsdf_ray.hip).  Only these methods reach the store's ray members.  Their entry points have judged
    // what needs no context: the parameters, null and short arguments, the views, the capacity.
    int tsdf_raycast(hipStream_t stream, const lv_tsdf_ray_params& p, const void* from, size_t from_stride, const void* to, size_t to_stride, size_t n,
                     lv_tsdf_ray_result* out, float* normals, uint8_t* rgba) {
        LV_SURFACE_CONFIGURED;
        return tsdf.raycast(stream, p.min_weight, from, from_stride, to, to_stride, n, out, normals, rgba);
    }

    int tsdf_raycast_views(hipStream_t stream, const lv_tsdf_ray_params& p, const lv_view* views, size_t n_views, lv_tsdf_ray_result* out,
                           float* normals, uint8_t* rgba, uint64_t stats[4]) {
        LV_SURFACE_CONFIGURED;
        return tsdf.raycast_views(stream, p.min_weight, views, n_views, out, normals, rgba, stats);
    }

    // ---- Surface registration (lv_surf_align.hip).  Only these methods reach the store's registration members.  Their entry points
    // have judged what needs no context: the parameters, null and short arguments, the guesses.
    int surf_sample(hipStream_t stream, int min_weight, const void* pts, size_t stride, size_t n, double* out, uint8_t* status) {
        LV_SURFACE_CONFIGURED;
        return tsdf.surf_sample(stream, min_weight, pts, stride, n, out, status);
    }

    int surf_align(hipStream_t stream, const lv_surf_align_params& p, const void* src, size_t stride, size_t n_src, const lv_graph_pose* guesses,
                   size_t K, lv_surf_align_result* results, int32_t best[2]) {
        LV_SURFACE_CONFIGURED;
        return tsdf.surf_align(stream, p, src, stride, n_src, guesses, K, results, best);
    }

    // ---- Submap merging (lv_surf_merge.hip).  Only this method reaches the store's merge.  Its entry point has judged what needs
    // no context (surf_merge_rule): q is that rule, kq still open.
    int surf_merge(hipStream_t stream, const lv_surf_submap& sub, const SurfMergeRule& q, uint64_t stats[4]) {
        LV_SURFACE_CONFIGURED;
        SurfMergeRule r = q;
        if (int rc = surf_merge_scale(sub.resolution, tsdf.grid.occ.resolution, &r.kq)) return rc;
        surface_edited();
        tsdf.rays.packed = false;
        int lo[3], hi[3];
        if (!surf_merge_box(tsdf.grid, r, lo, hi)) {   // the submap cannot meet the volume: nothing is staged, nothing runs
            if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
            return LV_OK;
        }
        return tsdf.merge(stream, sub, r, lo, hi, stats);
    }

    // ---- Rolling volumes (lv_grid.hpp's rule; lv_occupancy.hip, lv_tsdf.hip).  volume: LV_VOLUME_OCC or LV_VOLUME_SURFACE
    int recentre(hipStream_t stream, int volume, const int32_t shift[3], uint64_t stats[4]) {
        const bool grid = volume == LV_VOLUME_OCC;
        if (grid) LV_GRID_CONFIGURED;
        else LV_SURFACE_CONFIGURED;
        int32_t s_new[3];
        float origin_new[3];
        const char* why = grid ? grid_shift_check(occ.origin0, occ.prm.resolution, occ.shift, shift, s_new, origin_new)
                               : grid_shift_check(tsdf.origin0, tsdf.prm.resolution, tsdf.shift, shift, s_new, origin_new);
        if (why) { set_error("lv_volume_recentre: %s", why); return LV_EINVAL; }
        if (!(shift[0] | shift[1] | shift[2])) {   // nothing moves: nothing goes stale, no buffer is touched
            if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
            return LV_OK;
        }
        // (what was built from the volume goes stale once it has moved: a call that fails has changed nothing)
        const int rc = grid ? occ.recentre(stream, shift, s_new, origin_new, stats) : tsdf.recentre(stream, shift, s_new, origin_new, stats);
        if (rc != LV_OK) return rc;
        if (grid) grid_edited();
        else surface_edited();
        return LV_OK;
    }

    void shift_info(lv_volume_shifts* out) const {
        *out = lv_volume_shifts{};
        for (int a = 0; a < 3; ++a) {
            if (occ.configured) out->grid[a] = occ.shift[a];
            if (tsdf.configured) out->surface[a] = tsdf.shift[a];
            if (occ.configured && dist.built) out->field[a] = dist.shift[a];
            if (occ.configured && plan.built) out->plan[a] = plan.shift[a];
            if (occ.configured && frontier.built) out->frontier[a] = frontier.shift[a];
        }
    }

    // lv_destroy (after hipSetDevice)
    void release() {
        ray.release();
        rollout.release();
        mcl.release();
        lattice.release();
        frontier.release();
        plan.release();
        dist.release();
        occ.release();
        tsdf.release();
    }
};

#undef LV_GRID_CONFIGURED
#undef LV_DIST_BUILT
#undef LV_PLAN_BUILT
#undef LV_FRONTIER_BUILT
#undef LV_LATTICE_BUILT
#undef LV_SURFACE_CONFIGURED
#undef LV_COLOUR_PRESENT

}  // namespace lv
