// lv_maptools.hpp — the tools that run on the point map of a context: free-space removal, normals and outlier removal, clustering
// and removal by cluster, plane segmentation, painting and the three queries, with the one place where a call orders itself against
// an incremental insert still in flight on the side stream and against a background rebuild (lv_rebuild.hpp).  lv_ctx holds one
// MapTools; every entry point of lv_api.hip named below checks the context and makes one call here.  Host code only:
// tests/emu/maptools_emu.cpp compiles it with g++ against tests/emu/hip/hip_runtime.h, with its own stand-ins for the stores'
// member functions and for the rebuild (the template parameter: the product instantiates MapRebuild<MapStore>, as lv_rebuild.hpp
// is itself instantiated with a fake store by rebuild_emu.cpp), and tests/test_maptools_host.py holds it to the tables below.
//
// READY (MapSide::ready): MapStore::settle on the context's stream, then Rebuild::poll, which adopts a finished rebuild or drops a
// failed one.  The first failure is returned; a poll does not follow a failed settle.  A wrong order gives a silently wrong map: a
// removal the worker's copy never replays comes back at adoption.
//
// WHAT EACH CALL ASKS FOR, IN ORDER.  Nothing is judged before the context.  "rule": the argument rule of lv_rules.hpp /
// lv_planes.hpp (LV_EINVAL with its message, the map not looked at: neither settle nor poll).  "empty": the map is not built or
// holds no living point: LV_OK, no store is grown, ensure_rank does not run.  m, n_ids: of the active store after READY.
//
//   call                    | before READY                      | after READY
//   ------------------------+-----------------------------------+------------------------------------------------------------------
//   lv_map_remove_dynamic   | *n_removed = 0, THEN the rule     | empty; VisStore::build; [removal: journal, below]; m read again;
//                           |                                   |   with hits: ensure_hits(m), ensure_rank; vis_classify; hits out
//                           |                                   |   (m bytes); *n_removed
//   lv_map_normals          | the rule                          | capacity < m: LV_EINVAL; empty; ensure_rank; SurfaceStore::ensure
//                           |                                   |   (job 0); surface_search; surface_finish if normals or curvature
//                           |                                   |   are asked for; the outputs asked for; one synchronise
//   lv_map_remove_outliers  | the rule, THEN *n_removed = 0 and | empty; [removal: the dry pass (job 1 only), ensure, journal,
//                           |   stats = 0                       |   below]; m read again; with flags: ensure_rank; surface_outliers
//                           |                                   |   (dry_pass: the values of the dry pass stand); flags out (m
//                           |                                   |   bytes); *n_removed; stats (job 1 only): of the dry pass when
//                           |                                   |   removing, of the one pass in a dry run; other jobs leave zeros
//   lv_map_cluster          | the rule                          | labels && capacity < m: LV_EINVAL (*n_clusters untouched);
//   lv_map_planes           |                                   |   *n_clusters / *n_planes = 0; empty; ensure_rank; the store's
//                           |                                   |   ensure; the mask up if given; cluster_components + cluster_labels
//                           |                                   |   / planes_extract; labels, sizes / planes (as many as there is
//                           |                                   |   room for), the count
//   lv_map_remove_clusters  | the rule, q.seeded = seeds given, | empty; [removal: status(wait = 1), below]; m read again;
//                           |   THEN *n_removed = 0             |   ensure_rank; ClusterStore::ensure; mask, seeds up if given;
//                           |                                   |   cluster_components; cluster_remove; flags out (m bytes);
//                           |                                   |   *n_removed
//   lv_map_paint            | the rule                          | empty, or rgb, depth and n_seen all null: LV_OK; ensure_rank;
//                           |                                   |   PaintStore::run; the outputs asked for; one synchronise
//   lv_map_knn, _radius_    | nothing                           | QueryStore::knn / radius / box, which judge their arguments
//     search, _box_search   |                                   |
//
// Every step that fails ends the call with its code and nothing after it.
//
// WHAT EACH REMOVAL DOES TO THE BACKGROUND REBUILD.  The worker's copy must go through what the active store goes through.
//   a dry run               nothing: no journal, no order, no status.
//   lv_map_remove_dynamic   journal_replay of VisStore::d_blob, vis_blob_bytes(q) bytes (the poses and window-min images); the
//                           replay runs vis_classify(remove, no rank, no hits) on the copy: the same pure rule of the
//                           coordinates.  Then order() on the context's stream (the removal must not overtake a snapshot being
//                           taken on the side stream).  Then m is read AGAIN: the journal adopts a copy it finds ready.
//   lv_map_remove_outliers  the rule as the ACTIVE store resolved it (the dry pass fixes a job-1 threshold) goes to
//                           SurfaceStore::d_part, sizeof(SurfRule) bytes, and is journaled from there; the replay reads it back
//                           and runs surface_outliers(remove) with a SurfaceStore of its own (the worker runs beside the caller),
//                           released on success and on failure.  Then order(), then m again, as above.
//   lv_map_remove_clusters  status(wait = 1): mask and seeds are per-point arrays in the ACTIVE store's map order, which a replay
//                           could only honour by carrying both arrays and the copy's own ranks along.  So the removal waits
//                           until a rebuild in flight has landed (adopted with everything journaled so far replayed; adoption
//                           keeps the map order) and acts on the one store there is.  Then m is read.
//
// THE MAP SOURCE (MapSide::source; lv_elev_build, lv_ndt_build, lv_ndt_add, lv_occ_mark with pts == NULL; their stores stay in
// lv_ctx).  Given pts never touch the map: no settle, no poll.  Without them: READY, then MapSide::points(): the points by id
// (dead ones included), n_ids and m where the map is built and m > 0, else a null pointer and zeros.  lv_place_add_map judges its
// arguments and the database's room, then READY, then PlaceStore::add_map on the active store.
//
// THE ODDITIES AS THEY ARE (recorded, not fixed):
//   lv_map_fetch settles without polling: it may read the store a finished rebuild is about to replace (the same points).
//   lv_map_size settles and polls by hand and swallows both results (its poll runs after a failed settle too); it answers m as
//     it stands.
//   lv_occ_mark looks at the map only once its box clipped to the grid is not empty (lv_volumes.hpp "mark").
//   lv_map_build, lv_map_relinearise and lv_set_stream settle without polling: the first two cancel the rebuild instead.  So do
//     lv_reserve_stream, lv_iterate, lv_update, lv_update_begin, lv_correct and lv_fetch_knn: the update runs on the store it
//     finds (LV_SETTLE_MAP in lv_api.hip).
#pragma once
#include <cstring>

#include "lv_cluster.hpp"
#include "lv_host.hpp"
#include "lv_paint.hpp"
#include "lv_planes.hpp"
#include "lv_rebuild.hpp"
#include "lv_rules.hpp"
#include "lv_surface.hpp"
#include "lv_visibility.hpp"

namespace lv {

// What a map tool sees of the context: the active store, the rebuild, the context's streams as the rebuild takes them
template <class Rebuild>
struct MapSide {
    MapStore& map;
    Rebuild& rebuild;
    CtxStreams cs;
    hipStream_t stream;   // the context's stream (== cs.stream)

    int ready() {
        if (int rs = map.settle(stream)) return rs;   // (an incremental insert leaves its outcome in flight: MapStore::settle)
        return rebuild.poll(map, cs);
    }
    bool points(const float4** d, uint32_t* n_ids, uint32_t* m) const {
        const bool any = map.built && map.m > 0;
        *d = any ? map.d_orig.p : nullptr;
        *n_ids = any ? map.n_ids : 0u;
        *m = any ? map.m : 0u;
        return any;
    }
    int source(const void* pts, const float4** d, uint32_t* n_ids, uint32_t* m) {
        *d = nullptr;
        *n_ids = *m = 0;
        if (pts) return LV_OK;
        if (int rc = ready()) return rc;
        points(d, n_ids, m);
        return LV_OK;
    }
};

// m bytes of the caller's (pageable) memory at living ranks (a mask, seeds) -> the device, waited for
inline int upload_rank_bytes(hipStream_t stream, uint8_t* dst, const uint8_t* src, size_t m) {
    LV_HIP(hipMemcpyAsync(dst, src, m, hipMemcpyHostToDevice, stream));
    LV_HIP(hipStreamSynchronize(stream));
    return LV_OK;
}

template <class Rebuild>
struct MapTools {
    using Side = MapSide<Rebuild>;
    QueryStore query;       // lv_map_knn / lv_map_radius_search / lv_map_box_search: their own buffers (lv_query.hip); the ranks of every tool
    VisStore vis;           // lv_map_remove_dynamic: its own buffers (lv_visibility.hip)
    PaintStore paint;       // lv_map_paint: its own buffers (lv_paint.hip)
    SurfaceStore surface;   // lv_map_normals / lv_map_remove_outliers: their own buffers (lv_surface.hip)
    ClusterStore cluster;   // lv_map_cluster / lv_map_remove_clusters: their own buffers (lv_cluster.hip)
    PlaneStore planes;      // lv_map_planes: its own buffers (lv_planes.hip); nothing allocated before the first call

    void release() { release_all(query, vis, paint, surface, cluster, planes); }   // (lv_destroy's order)

    // ---- Free-space removal (lv_visibility.hip)
    int remove_dynamic(Side ms, const lv_view* views, size_t n_views, const lv_visibility_params* p, uint8_t* hits, size_t* n_removed) {
        if (n_removed) *n_removed = 0;
        VisRule q{};
        int rc = visibility_rule(views, n_views, p, &q);
        if (rc) return rc;
        rc = ms.ready();
        if (rc) return rc;
        if (!ms.map.built || ms.map.m == 0) return LV_OK;
        rc = vis.build(ms.stream, views, n_views, q);
        if (rc) return rc;
        const bool remove = p->dry_run == 0;
        if (remove) {
            rc = ms.rebuild.journal_replay(ms.map, ms.cs, vis.d_blob, vis_blob_bytes(q), [q](MapStore& S, hipStream_t s, const void* blob) {
                return vis_classify(S, s, blob, q, nullptr, nullptr, true, nullptr);
            });
            if (!rc) rc = ms.rebuild.order(ms.cs, ms.stream);
            if (rc) return rc;
        }
        const size_t m = ms.map.m;   // (the store that acts: a copy adopted by the journal included)
        const uint32_t* rank = nullptr;
        if (hits) {
            rc = vis.ensure_hits(m);
            if (!rc) rc = query.ensure_rank(ms.map, ms.stream, &rank);
            if (rc) return rc;
        }
        uint32_t nr = 0;
        rc = vis_classify(ms.map, ms.stream, vis.d_blob, q, rank, hits ? vis.d_hits.p : nullptr, remove, &nr);
        if (rc) return rc;
        if (hits) LV_HIP(hipMemcpy(hits, vis.d_hits, m, hipMemcpyDeviceToHost));
        if (n_removed) *n_removed = nr;
        return LV_OK;
    }

    // ---- Surface normals and outlier removal (lv_surface.hip)
    int normals(Side ms, const lv_surface_params* p, float* normals, float* curvature, float* mean_dist, int32_t* n_used, size_t capacity) {
        SurfRule q{};
        int rc = surface_rule(p, &q);
        if (rc) return rc;
        rc = ms.ready();
        if (rc) return rc;
        const size_t m = ms.map.m;
        if (capacity < m) { set_error("capacity %zu < %zu living points", capacity, m); return LV_EINVAL; }
        if (!ms.map.built || m == 0) return LV_OK;
        const uint32_t* rank = nullptr;
        rc = query.ensure_rank(ms.map, ms.stream, &rank);
        if (!rc) rc = surface.ensure(ms.map.n_ids, m, 0);
        if (!rc) rc = surface_search(ms.map, ms.stream, surface, q, rank);
        if (!rc && (normals || curvature)) rc = surface_finish(ms.map, ms.stream, surface, q, rank);
        if (rc) return rc;
        if (normals) LV_HIP(hipMemcpyAsync(normals, surface.d_normals, 3 * m * sizeof(float), hipMemcpyDeviceToHost, ms.stream));
        if (curvature) LV_HIP(hipMemcpyAsync(curvature, surface.d_curv, m * sizeof(float), hipMemcpyDeviceToHost, ms.stream));
        if (mean_dist) LV_HIP(hipMemcpyAsync(mean_dist, surface.d_mean, m * sizeof(float), hipMemcpyDeviceToHost, ms.stream));
        if (n_used) LV_HIP(hipMemcpyAsync(n_used, surface.d_used, m * sizeof(int32_t), hipMemcpyDeviceToHost, ms.stream));
        LV_HIP(hipStreamSynchronize(ms.stream));
        return LV_OK;
    }

    int remove_outliers(Side ms, const lv_outlier_params* p, uint8_t* flags, size_t* n_removed, double* stats) {
        SurfRule q{};
        int rc = outlier_rule(p, &q);
        if (rc) return rc;
        // (valid from here on: the outputs are written)
        if (n_removed) *n_removed = 0;
        if (stats) stats[0] = stats[1] = stats[2] = 0.0;
        rc = ms.ready();
        if (rc) return rc;
        if (!ms.map.built || ms.map.m == 0) return LV_OK;
        const bool remove = p->dry_run == 0;
        const uint32_t* rank = nullptr;
        double st3[3] = {0.0, 0.0, 0.0};
        bool dry_pass = false;
        if (remove) {
            // the rule as the active store resolves it: a dry pass (mode 1 is resolved as it stands)
            if (q.job == 1) {
                rc = surface_outliers(ms.map, ms.stream, surface, q, nullptr, false, false, nullptr, st3);
                if (rc) return rc;
                dry_pass = true;
            }
            rc = surface.ensure(ms.map.n_ids, ms.map.m, q.job);
            if (rc) return rc;
            static_assert(sizeof(SurfRule) <= 2 * 256 * sizeof(double), "the rule is journaled out of SurfaceStore::d_part");
            LV_HIP(hipMemcpyAsync(surface.d_part, &q, sizeof(SurfRule), hipMemcpyHostToDevice, ms.stream));
            LV_HIP(hipStreamSynchronize(ms.stream));   // (q lives on this frame)
            rc = ms.rebuild.journal_replay(ms.map, ms.cs, surface.d_part, sizeof(SurfRule), [](MapStore& S, hipStream_t s, const void* blob) {
                // (the worker runs beside the caller: its own rule copy and buffers, nothing of the context's SurfaceStore)
                SurfRule r{};
                LV_HIP(hipMemcpyAsync(&r, blob, sizeof(SurfRule), hipMemcpyDeviceToHost, s));
                LV_HIP(hipStreamSynchronize(s));
                SurfaceStore own;
                const int rr = surface_outliers(S, s, own, r, nullptr, false, true, nullptr, nullptr);
                own.release();   // (on every path: surface_outliers returns its errors, it does not throw)
                return rr;
            });
            if (!rc) rc = ms.rebuild.order(ms.cs, ms.stream);
            if (rc) return rc;
        }
        const size_t m = ms.map.m;   // (the store that acts: a copy adopted by the journal included)
        if (flags) {
            rc = query.ensure_rank(ms.map, ms.stream, &rank);
            if (rc) return rc;
        }
        uint32_t nr = 0;
        double st_act[3];
        // (the dry pass's values stand unless the journal call adopted a rebuilt copy: the map's stamp tells)
        rc = surface_outliers(ms.map, ms.stream, surface, q, rank, flags != nullptr, remove, &nr, st_act, dry_pass);
        if (rc) return rc;
        if (flags) LV_HIP(hipMemcpy(flags, surface.d_flags, m, hipMemcpyDeviceToHost));
        if (n_removed) *n_removed = nr;
        if (stats && q.job == 1) { const double* src = remove ? st3 : st_act; stats[0] = src[0]; stats[1] = src[1]; stats[2] = src[2]; }
        return LV_OK;
    }

    // ---- Map clustering (lv_cluster.hip)
    int cluster_map(Side ms, const lv_cluster_params* p, const uint8_t* mask, int32_t* labels, size_t capacity, uint32_t* sizes, size_t sizes_capacity,
                    size_t* n_clusters) {
        ClusterRule q{};
        int rc = cluster_rule(p, &q);
        if (rc) return rc;
        rc = ms.ready();
        if (rc) return rc;
        const size_t m = ms.map.m;
        if (labels && capacity < m) { set_error("capacity %zu < %zu living points", capacity, m); return LV_EINVAL; }
        if (n_clusters) *n_clusters = 0;
        if (!ms.map.built || m == 0) return LV_OK;
        const uint32_t* rank = nullptr;
        rc = query.ensure_rank(ms.map, ms.stream, &rank);
        if (!rc) rc = cluster.ensure(ms.map.n_ids, m);
        if (!rc && mask) rc = upload_rank_bytes(ms.stream, cluster.d_mask, mask, m);
        if (!rc) rc = cluster_components(ms.map, ms.stream, cluster, q, rank, mask ? cluster.d_mask.p : nullptr);
        size_t C = 0;
        if (!rc) rc = cluster_labels(ms.map, ms.stream, cluster, q, rank, labels != nullptr, &C);
        if (rc) return rc;
        if (labels) LV_HIP(hipMemcpyAsync(labels, cluster.d_labels, m * sizeof(int32_t), hipMemcpyDeviceToHost, ms.stream));
        const size_t ns = C < sizes_capacity ? C : sizes_capacity;
        if (sizes && ns) LV_HIP(hipMemcpyAsync(sizes, cluster.d_sizes, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, ms.stream));
        LV_HIP(hipStreamSynchronize(ms.stream));
        if (n_clusters) *n_clusters = C;
        return LV_OK;
    }

    int remove_clusters(Side ms, const lv_cluster_params* p, const uint8_t* mask, const uint8_t* seeds, uint8_t* flags, size_t* n_removed) {
        ClusterRule q{};
        int rc = cluster_rule(p, &q);
        if (rc) return rc;
        q.seeded = seeds ? 1 : 0;
        // (valid from here on: the outputs are written)
        if (n_removed) *n_removed = 0;
        rc = ms.ready();
        if (rc) return rc;
        if (!ms.map.built || ms.map.m == 0) return LV_OK;
        const bool remove = p->dry_run == 0;
        if (remove) {
            rc = ms.rebuild.status(ms.map, ms.cs, 1, nullptr);
            if (rc) return rc;
        }
        const size_t m = ms.map.m;   // (the store that acts: an adopted copy included; adoption keeps the map order)
        const uint32_t* rank = nullptr;
        rc = query.ensure_rank(ms.map, ms.stream, &rank);
        if (!rc) rc = cluster.ensure(ms.map.n_ids, m);
        if (!rc && mask) rc = upload_rank_bytes(ms.stream, cluster.d_mask, mask, m);
        if (!rc && seeds) rc = upload_rank_bytes(ms.stream, cluster.d_seeds, seeds, m);
        if (!rc) rc = cluster_components(ms.map, ms.stream, cluster, q, rank, mask ? cluster.d_mask.p : nullptr);
        uint32_t nr = 0;
        if (!rc) rc = cluster_remove(ms.map, ms.stream, cluster, q, rank, cluster.d_seeds, flags ? cluster.d_flags.p : nullptr, remove, &nr);
        if (rc) return rc;
        if (flags) LV_HIP(hipMemcpy(flags, cluster.d_flags, m, hipMemcpyDeviceToHost));
        if (n_removed) *n_removed = nr;
        return LV_OK;
    }

    // ---- Plane segmentation (lv_planes.hip)
    int extract_planes(Side ms, const lv_plane_params* p, const uint8_t* mask, int32_t* labels, size_t capacity, lv_plane* out, size_t planes_capacity,
                       size_t* n_planes) {
        PlaneRule q{};
        int rc = plane_rule(p, &q);
        if (rc) return rc;
        rc = ms.ready();
        if (rc) return rc;
        const size_t m = ms.map.m;
        if (labels && capacity < m) { set_error("capacity %zu < %zu living points", capacity, m); return LV_EINVAL; }
        if (n_planes) *n_planes = 0;
        if (!ms.map.built || m == 0) return LV_OK;
        const uint32_t* rank = nullptr;
        rc = query.ensure_rank(ms.map, ms.stream, &rank);
        if (!rc) rc = planes.ensure(ms.map.n_ids, m, q.iterations);
        if (!rc && mask) rc = upload_rank_bytes(ms.stream, planes.d_mask, mask, m);
        lv_plane found[PLANE_MAX_PLANES];
        size_t P = 0;
        if (!rc) rc = planes_extract(ms.map, ms.stream, planes, q, rank, mask ? planes.d_mask.p : nullptr, labels != nullptr, found, &P);
        if (rc) return rc;
        if (labels) LV_HIP(hipMemcpy(labels, planes.d_labels, m * sizeof(int32_t), hipMemcpyDeviceToHost));
        const size_t np = P < planes_capacity ? P : planes_capacity;
        if (out && np) std::memcpy(out, found, np * sizeof(lv_plane));
        if (n_planes) *n_planes = P;
        return LV_OK;
    }

    // ---- Map painting (lv_paint.hip)
    int paint_map(Side ms, const lv_camera_view* views, size_t n_views, const lv_paint_params* p, float* rgb, float* depth, uint8_t* n_seen) {
        PaintRule q{};
        PaintCam cams[PAINT_MAX_VIEWS];
        int rc = paint_rule(views, n_views, p, &q, cams);
        if (rc) return rc;
        rc = ms.ready();
        if (rc) return rc;
        if (!ms.map.built || ms.map.m == 0 || !(rgb || depth || n_seen)) return LV_OK;
        const size_t m = ms.map.m;
        const uint32_t* rank = nullptr;
        rc = query.ensure_rank(ms.map, ms.stream, &rank);
        if (!rc) rc = paint.run(ms.map, ms.stream, views, cams, q, rank, rgb != nullptr, depth != nullptr, n_seen != nullptr);
        if (rc) return rc;
        if (rgb) LV_HIP(hipMemcpyAsync(rgb, paint.d_rgb, 3 * m * sizeof(float), hipMemcpyDeviceToHost, ms.stream));
        if (depth) LV_HIP(hipMemcpyAsync(depth, paint.d_depth, m * sizeof(float), hipMemcpyDeviceToHost, ms.stream));
        if (n_seen) LV_HIP(hipMemcpyAsync(n_seen, paint.d_seen, m, hipMemcpyDeviceToHost, ms.stream));
        LV_HIP(hipStreamSynchronize(ms.stream));
        return LV_OK;
    }

    // ---- Map queries (lv_query.hip)
    int knn(Side ms, const void* q, size_t stride, size_t n, int k, float max_dist, uint32_t* idx, float* d2, int32_t* found) {
        if (int rc = ms.ready()) return rc;
        return query.knn(ms.map, ms.stream, q, stride, n, k, max_dist, idx, d2, found);
    }
    int radius_search(Side ms, const void* q, size_t stride, size_t n, float radius, size_t* offsets, uint32_t* idx, float* d2, size_t capacity,
                      size_t* total) {
        if (int rc = ms.ready()) return rc;
        return query.radius(ms.map, ms.stream, q, stride, n, radius, offsets, idx, d2, capacity, total);
    }
    int box_search(Side ms, const float lo[3], const float hi[3], uint32_t* idx, float* xyz, size_t capacity, size_t* n_out) {
        if (int rc = ms.ready()) return rc;
        return query.box(ms.map, ms.stream, lo, hi, idx, xyz, capacity, n_out);
    }
};

}  // namespace lv
