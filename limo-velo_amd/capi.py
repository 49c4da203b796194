"""ctypes binding of the C-ABI (include/limovelo_hip.h) for tests, smoke() and bench.py.

This is plumbing, not the product: the product is liblimovelo_hip.so (HIP, gfx950) and the C++
Mapper / Localizator shim in limo-velo_amd/host/.  There is NO CPU fallback: loading fails loudly if
the HIP library has not been built, and Context() fails if no GPU is present.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LV_LIB_PATH: another build of the same library, for A/B measurements of two builds in one box — scripts/gpu_ab_multi.sh)
LIB_PATH = os.environ.get("LV_LIB_PATH") or os.path.join(_HERE, "liblimovelo_hip.so")

LV_OK = 0
PEER_HANDLE_BYTES = 128   # LV_PEER_HANDLE_BYTES: two HIP IPC handles (gather buffers, flag word)
SUMS_LEN = 96
NS = 23

# every symbol include/limovelo_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "lv_default_params", "lv_last_error", "lv_version", "lv_create", "lv_destroy", "lv_set_stream", "lv_get_stream",
    "lv_synchronize", "lv_map_build", "lv_map_add", "lv_map_add_scan", "lv_map_evict_box", "lv_map_evict_oldest", "lv_map_relinearise", "lv_map_get_stats",
    "lv_map_size", "lv_map_fetch", "lv_scan_set", "lv_scan_deskew", "lv_scan_downsample", "lv_scan_size", "lv_scan_route", "lv_scan_fetch", "lv_iterate", "lv_pseudo_measurement",
    "lv_map_relinearise_async", "lv_map_reserve_rebuild", "lv_map_rebuild_status", "lv_update", "lv_filter_set", "lv_filter_get", "lv_predict", "lv_correct", "lv_get_degeneracy_values", "lv_update_begin", "lv_pass_reduce", "lv_sums_device_ptr", "lv_set_sums_buffer", "lv_pass_solve", "lv_update_end",
    "lv_set_capture", "lv_fetch_knn", "lv_fetch_matches", "lv_fetch_neighbors", "lv_set_record_dump", "lv_last_update_fused", "lv_last_passes", "lv_set_fused_pass", "lv_set_option", "lv_get_pass_clocks", "lv_pass_geometry", "lv_fetch_rows", "lv_calculate_H", "lv_get_timing", "lv_set_profiling", "lv_get_phase_clocks", "lv_get_solve_clocks", "lv_get_level_histogram",
    "lv_comm_unique_id", "lv_comm_init", "lv_comm_destroy", "lv_comm_world", "lv_comm_set_shard_max", "lv_set_comm_fused", "lv_comm_set_host_gather", "lv_comm_peer_export", "lv_comm_peer_init",
    "lv_cloud_format_preset", "lv_cloud_ingest", "lv_cloud_size", "lv_cloud_fetch", "lv_cloud_clear", "lv_cloud_reserve", "lv_reserve_stream", "lv_scan_deskew_window",
    "lv_map_knn", "lv_map_radius_search", "lv_map_box_search",
    "lv_iterate_batch", "lv_update_batch",
    "lv_default_visibility_params", "lv_map_remove_dynamic",
    "lv_default_paint_params", "lv_map_paint",
    "lv_default_surface_params", "lv_default_outlier_params", "lv_map_normals", "lv_map_remove_outliers",
    "lv_default_cluster_params", "lv_map_cluster", "lv_map_remove_clusters",
    "lv_default_plane_params", "lv_map_planes",
    "lv_default_place_params", "lv_place_configure", "lv_place_describe", "lv_place_add_scan", "lv_place_add_map", "lv_place_query",
    "lv_place_count", "lv_place_clear", "lv_place_fetch", "lv_place_load",
    "lv_default_occupancy_params", "lv_occ_configure", "lv_occ_integrate", "lv_occ_query", "lv_occ_project", "lv_occ_fetch", "lv_occ_load",
    "lv_occ_clear", "lv_occ_get_params",
    "lv_default_distance_params", "lv_occ_distance_build", "lv_occ_distance_fetch", "lv_occ_distance_query", "lv_occ_distance_info",
    "lv_occ_distance_clear",
    "lv_default_plan_params", "lv_occ_plan_build", "lv_occ_plan_fetch", "lv_occ_plan_paths", "lv_occ_plan_info", "lv_occ_plan_clear",
    "lv_default_lattice_params", "lv_occ_lattice_build", "lv_occ_lattice_fetch", "lv_occ_lattice_paths", "lv_occ_lattice_info",
    "lv_occ_lattice_clear",
    "lv_default_frontier_params", "lv_occ_frontier_build", "lv_occ_frontier_fetch", "lv_occ_frontier_clusters", "lv_occ_frontier_rank",
    "lv_occ_frontier_info", "lv_occ_frontier_clear",
    "lv_default_ray_params", "lv_occ_raycast", "lv_occ_view_gain",
    "lv_default_elevation_params", "lv_elev_build", "lv_elev_fetch", "lv_elev_query", "lv_elev_info", "lv_elev_clear",
    "lv_occ_distance_build_cells",
    "lv_default_rollout_params", "lv_occ_rollout",
    "lv_default_mcl_params", "lv_occ_mcl_weigh",
    "lv_default_mcl_resample_params", "lv_occ_mcl_filter_set", "lv_occ_mcl_filter_move", "lv_occ_mcl_filter_weigh", "lv_occ_mcl_filter_resample",
    "lv_occ_mcl_filter_get", "lv_occ_mcl_filter_info", "lv_occ_mcl_filter_clear",
    "lv_default_tsdf_params", "lv_tsdf_configure", "lv_tsdf_integrate", "lv_tsdf_query", "lv_tsdf_fetch", "lv_tsdf_load", "lv_tsdf_clear",
    "lv_tsdf_get_params", "lv_tsdf_mesh_build", "lv_tsdf_mesh_fetch", "lv_tsdf_mesh_info", "lv_tsdf_mesh_clear",
    "lv_default_depth_params", "lv_depth_integrate",
    "lv_default_colour_params", "lv_colour_integrate", "lv_colour_fetch", "lv_colour_load", "lv_colour_query", "lv_colour_clear",
    "lv_colour_info", "lv_mesh_colours",
    "lv_default_surf_ray_params", "lv_surf_raycast", "lv_surf_raycast_views",
    "lv_volume_recentre", "lv_volume_shift_info", "lv_default_occ_mark_params", "lv_occ_mark",
    "lv_default_observation", "lv_observe", "lv_observe_results",
    "lv_default_graph_params", "lv_graph_set", "lv_graph_optimise", "lv_graph_fetch", "lv_graph_chi2", "lv_graph_warp_points",
    "lv_graph_get_info", "lv_graph_clear",
    "lv_default_traj_smooth_params", "lv_default_traj_register_params", "lv_traj_set", "lv_traj_fetch", "lv_traj_get_info", "lv_traj_clear",
    "lv_traj_sample", "lv_traj_smooth", "lv_traj_correct", "lv_traj_register", "lv_traj_register_cloud",
    "lv_default_ndt_params", "lv_default_ndt_align_params", "lv_ndt_build", "lv_ndt_add", "lv_ndt_fetch", "lv_ndt_align", "lv_ndt_info",
    "lv_ndt_clear",
    "lv_default_surf_align_params", "lv_surf_sample", "lv_surf_align",
    "lv_default_occ_surface_params", "lv_occ_from_surface",
    "lv_default_surf_merge_params", "lv_surf_merge",
]

# ctypes signatures of the map queries (include/limovelo_hip.h "Map queries"; tests/test_map_query_abi.py holds them to the header)
QUERY_ARGTYPES = {
    "lv_map_knn": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                   C.POINTER(C.c_int32)],
    "lv_map_radius_search": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                             C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t)],
    "lv_map_box_search": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_size_t,
                          C.POINTER(C.c_size_t)],
}

# ctypes signatures of the multi-hypothesis calls (include/limovelo_hip.h "Multi-hypothesis updates"; tests/test_update_batch_abi.py)
BATCH_ARGTYPES = {
    "lv_iterate_batch": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "lv_update_batch": [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                        C.c_void_p],
}



class View(C.Structure):  # lv_view
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("points", C.c_void_p), ("stride", C.c_size_t), ("n", C.c_size_t)]


class VisibilityParams(C.Structure):  # lv_visibility_params
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("v_min_deg", C.c_float), ("v_max_deg", C.c_float), ("min_range", C.c_float),
                ("max_range", C.c_float), ("margin_abs", C.c_float), ("margin_rel", C.c_float), ("window", C.c_int), ("min_hits", C.c_int),
                ("dry_run", C.c_int)]


# ctypes signatures of the dynamic-point removal (include/limovelo_hip.h "Dynamic-point removal"; tests/test_map_visibility_abi.py)
VISIBILITY_ARGTYPES = {
    "lv_map_remove_dynamic": [C.c_void_p, C.POINTER(View), C.c_size_t, C.POINTER(VisibilityParams), C.POINTER(C.c_uint8),
                              C.POINTER(C.c_size_t)],
}


LV_IMAGE_RGB8, LV_IMAGE_BGR8, LV_IMAGE_MONO8 = 0, 1, 2
IMAGE_CHANNELS = {LV_IMAGE_RGB8: 3, LV_IMAGE_BGR8: 3, LV_IMAGE_MONO8: 1}


class LvCameraView(C.Structure):  # lv_camera_view
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("dist", C.c_float * 5), ("width", C.c_int), ("height", C.c_int), ("format", C.c_int), ("image", C.c_void_p),
                ("row_stride", C.c_size_t)]


class LvPaintParams(C.Structure):  # lv_paint_params
    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("max_norm_radius", C.c_float), ("zbuf_scale", C.c_int),
                ("window", C.c_int), ("margin_abs", C.c_float), ("margin_rel", C.c_float), ("blend", C.c_int)]


# ctypes signatures of the map painting (include/limovelo_hip.h "Map painting"; tests/test_map_paint_abi.py)
PAINT_ARGTYPES = {
    "lv_map_paint": [C.c_void_p, C.POINTER(LvCameraView), C.c_size_t, C.POINTER(LvPaintParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                     C.POINTER(C.c_uint8)],
}


class SurfaceParams(C.Structure):  # lv_surface_params
    _fields_ = [("k", C.c_int), ("max_dist", C.c_float), ("min_neighbours", C.c_int), ("orient", C.c_int), ("viewpoint", C.c_double * 3)]


class OutlierParams(C.Structure):  # lv_outlier_params
    _fields_ = [("mode", C.c_int), ("k", C.c_int), ("max_dist", C.c_float), ("std_mul", C.c_float), ("radius", C.c_float),
                ("min_neighbours", C.c_int), ("dry_run", C.c_int)]


# ctypes signatures of the surface calls (include/limovelo_hip.h "Surface normals and outlier removal"; tests/test_map_surface_abi.py)
SURFACE_ARGTYPES = {
    "lv_map_normals": [C.c_void_p, C.POINTER(SurfaceParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                       C.POINTER(C.c_int32), C.c_size_t],
    "lv_map_remove_outliers": [C.c_void_p, C.POINTER(OutlierParams), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t), C.POINTER(C.c_double)],
}


class ClusterParams(C.Structure):  # lv_cluster_params
    _fields_ = [("radius", C.c_float), ("min_size", C.c_uint32), ("max_size", C.c_uint32), ("dry_run", C.c_int)]


# ctypes signatures of the clustering calls (include/limovelo_hip.h "Map clustering"; tests/test_map_cluster_abi.py)
CLUSTER_ARGTYPES = {
    "lv_map_cluster": [C.c_void_p, C.POINTER(ClusterParams), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_uint32),
                       C.c_size_t, C.POINTER(C.c_size_t)],
    "lv_map_remove_clusters": [C.c_void_p, C.POINTER(ClusterParams), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                               C.POINTER(C.c_size_t)],
}


class PlaneParams(C.Structure):  # lv_plane_params
    _fields_ = [("distance", C.c_float), ("iterations", C.c_uint32), ("max_planes", C.c_uint32), ("min_inliers", C.c_uint32),
                ("seed", C.c_uint64), ("constraint", C.c_int), ("axis", C.c_float * 3), ("max_angle", C.c_float), ("refine", C.c_int)]


class Plane(C.Structure):  # lv_plane (64 bytes)
    _fields_ = [("normal", C.c_float * 3), ("anchor", C.c_float * 3), ("d", C.c_double), ("rms", C.c_double), ("inliers", C.c_uint32),
                ("support", C.c_uint32), ("hypothesis", C.c_uint32), ("candidates", C.c_uint32), ("n_fit", C.c_uint32), ("flags", C.c_uint32)]


# the same record as a numpy dtype (Context.map_planes)
PLANE_DTYPE = np.dtype([("normal", np.float32, 3), ("anchor", np.float32, 3), ("d", np.float64), ("rms", np.float64), ("inliers", np.uint32),
                        ("support", np.uint32), ("hypothesis", np.uint32), ("candidates", np.uint32), ("n_fit", np.uint32),
                        ("flags", np.uint32)])
PLANE_MAX_PLANES = 32
PLANE_CHUNK, PLANE_TILE = 256, 1024   # the scoring kernel's hypotheses / candidates per workgroup (PL_CHUNK, PL_TILE of lv_planes.hpp)

# ctypes signatures of the plane segmentation (include/limovelo_hip.h "Plane segmentation"; tests/test_planes_abi.py)
PLANE_ARGTYPES = {
    "lv_map_planes": [C.c_void_p, C.POINTER(PlaneParams), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(Plane),
                      C.c_size_t, C.POINTER(C.c_size_t)],
}


class PlaceParams(C.Structure):  # lv_place_params
    _fields_ = [("n_rings", C.c_int), ("n_sectors", C.c_int), ("rmin", C.c_float), ("rmax", C.c_float), ("z_offset", C.c_float)]


# ctypes signatures of the place recognition (include/limovelo_hip.h "Place recognition"; tests/test_place_abi.py)
PLACE_ARGTYPES = {
    "lv_place_configure": [C.c_void_p, C.POINTER(PlaceParams)],
    "lv_place_describe": [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)],
    "lv_place_add_scan": [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)],
    "lv_place_add_map": [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_uint32)],
    "lv_place_query": [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                       C.POINTER(C.c_size_t)],
    "lv_place_clear": [C.c_void_p],
    "lv_place_fetch": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t],
    "lv_place_load": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t],
}


class GraphPose(C.Structure):  # lv_graph_pose (56 bytes)
    _fields_ = [("t", C.c_double * 3), ("q", C.c_double * 4)]


class GraphEdge(C.Structure):  # lv_graph_edge (240 bytes)
    _fields_ = [("i", C.c_uint32), ("j", C.c_uint32), ("t", C.c_double * 3), ("q", C.c_double * 4), ("info", C.c_double * 21),
                ("huber", C.c_double)]


class GraphPrior(C.Structure):  # lv_graph_prior (264 bytes)
    _fields_ = [("i", C.c_uint32), ("reserved", C.c_uint32), ("t", C.c_double * 3), ("q", C.c_double * 4), ("lever", C.c_double * 3),
                ("info", C.c_double * 21), ("huber", C.c_double)]


class GraphParams(C.Structure):  # lv_graph_params
    _fields_ = [("max_iterations", C.c_int32), ("pcg_max_iterations", C.c_int32), ("pcg_tol", C.c_double), ("step_tol", C.c_double),
                ("lambda_init", C.c_double), ("lambda_min", C.c_double), ("lambda_max", C.c_double)]


class GraphInfo(C.Structure):  # lv_graph_info
    _fields_ = [("set", C.c_int32), ("status", C.c_int32), ("n", C.c_uint32), ("n_edges", C.c_uint32), ("n_priors", C.c_uint32),
                ("n_fixed", C.c_uint32), ("longest_list", C.c_uint32), ("accepted", C.c_uint32), ("rejected", C.c_uint32),
                ("pcg_iterations", C.c_uint32), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("last_step", C.c_double),
                ("lambda_", C.c_double)]

    def as_dict(self):
        return {("lambda" if f == "lambda_" else f): getattr(self, f) for f, _ in self._fields_}


GRAPH_CONVERGED, GRAPH_MAX_ITERATIONS = 0, 1
# numpy views of the records (the same bytes as GraphPose, GraphEdge, GraphPrior)
GRAPH_POSE_DTYPE = np.dtype([("t", "f8", 3), ("q", "f8", 4)])
GRAPH_EDGE_DTYPE = np.dtype([("i", "u4"), ("j", "u4"), ("t", "f8", 3), ("q", "f8", 4), ("info", "f8", 21), ("huber", "f8")])
GRAPH_PRIOR_DTYPE = np.dtype([("i", "u4"), ("reserved", "u4"), ("t", "f8", 3), ("q", "f8", 4), ("lever", "f8", 3), ("info", "f8", 21),
                              ("huber", "f8")])

# ctypes signatures of the pose graph (include/limovelo_hip.h "Pose graph"; tests/test_graph_abi.py)
GRAPH_ARGTYPES = {
    "lv_graph_set": [C.c_void_p, C.POINTER(GraphPose), C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(GraphEdge), C.c_size_t,
                     C.POINTER(GraphPrior), C.c_size_t],
    "lv_graph_optimise": [C.c_void_p, C.POINTER(GraphParams), C.POINTER(GraphInfo)],
    "lv_graph_fetch": [C.c_void_p, C.POINTER(GraphPose), C.c_size_t],
    "lv_graph_chi2": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "lv_graph_warp_points": [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_float)],
    "lv_graph_get_info": [C.c_void_p, C.POINTER(GraphInfo)],
    "lv_graph_clear": [C.c_void_p],
}


class TrajKnot(C.Structure):  # lv_traj_knot (64 bytes)
    _fields_ = [("time", C.c_double), ("t", C.c_double * 3), ("q", C.c_double * 4)]


class TrajSmoothParams(C.Structure):  # lv_traj_smooth_params (24 bytes)
    _fields_ = [("sigma", C.c_double), ("half_window", C.c_int32), ("iterations", C.c_int32), ("pin_ends", C.c_int32)]


class TrajRegisterParams(C.Structure):  # lv_traj_register_params (72 bytes)
    _fields_ = [("extrapolate", C.c_int32), ("frame", C.c_int32), ("ext_t", C.c_double * 3), ("ext_q", C.c_double * 4),
                ("frame_time", C.c_double)]


class TrajInfo(C.Structure):  # lv_traj_info (64 bytes)
    _fields_ = [("set", C.c_int32), ("n", C.c_uint32), ("t_first", C.c_double), ("t_last", C.c_double), ("smooth_iterations", C.c_uint32),
                ("corrections", C.c_uint32), ("last_register", C.c_uint64 * 4)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["last_register"] = [int(v) for v in self.last_register]
        return d


TRAJ_MAX_KNOTS = 1 << 20
TRAJ_INSIDE, TRAJ_BEFORE, TRAJ_AFTER, TRAJ_NONFINITE = 0, 1, 2, 3
TRAJ_CLAMP, TRAJ_REFUSE = 0, 1
TRAJ_WORLD, TRAJ_FRAME_AT = 0, 1
TRAJ_TILE = 256   # knots a workgroup of the register kernel stages (TRAJ_TILE of lv_traj.hpp)
TRAJ_KNOT_DTYPE = np.dtype([("time", "f8"), ("t", "f8", 3), ("q", "f8", 4)])   # the same bytes as TrajKnot

# ctypes signatures of the trajectory (include/limovelo_hip.h "Trajectory"; tests/test_traj_abi.py)
TRAJ_ARGTYPES = {
    "lv_traj_set": [C.c_void_p, C.POINTER(TrajKnot), C.c_size_t],
    "lv_traj_fetch": [C.c_void_p, C.POINTER(TrajKnot), C.c_size_t],
    "lv_traj_get_info": [C.c_void_p, C.POINTER(TrajInfo)],
    "lv_traj_clear": [C.c_void_p],
    "lv_traj_sample": [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_int, C.POINTER(GraphPose), C.POINTER(C.c_uint8)],
    "lv_traj_smooth": [C.c_void_p, C.POINTER(TrajSmoothParams), C.POINTER(C.c_uint8)],
    "lv_traj_correct": [C.c_void_p, C.POINTER(TrajKnot), C.c_size_t],
    "lv_traj_register": [C.c_void_p, C.POINTER(TrajRegisterParams), C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_float),
                         C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)],
    "lv_traj_register_cloud": [C.c_void_p, C.POINTER(TrajRegisterParams), C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                               C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)],
}


class NdtParams(C.Structure):  # lv_ndt_params (40 bytes)
    _fields_ = [("origin", C.c_float * 3), ("resolution", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("min_points", C.c_int32), ("reg", C.c_double)]


class NdtAlignParams(C.Structure):  # lv_ndt_align_params (48 bytes)
    _fields_ = [("search", C.c_int32), ("max_iterations", C.c_int32), ("d2", C.c_double), ("step_tol", C.c_double),
                ("lambda_init", C.c_double), ("lambda_min", C.c_double), ("lambda_max", C.c_double)]


class NdtResult(C.Structure):  # lv_ndt_result (264 bytes)
    _fields_ = [("pose", GraphPose), ("score", C.c_double), ("info", C.c_double * 21), ("last_step", C.c_double), ("lambda_", C.c_double),
                ("n_in", C.c_uint32), ("status", C.c_int32), ("accepted", C.c_uint32), ("rejected", C.c_uint32)]


class NdtTargetInfo(C.Structure):  # lv_ndt_target_info (80 bytes)
    _fields_ = [("built", C.c_int32), ("from_map", C.c_int32), ("n_used", C.c_uint64), ("n_ignored", C.c_uint64), ("used_voxels", C.c_uint64),
                ("sparse_voxels", C.c_uint64), ("params", NdtParams)]


NDT_CONVERGED, NDT_MAX_ITERATIONS, NDT_NO_OVERLAP = 0, 1, 2
NDT_CHUNK = 512   # LV_NDT_CHUNK: source points per workgroup of the evaluation
NDT_COUNT, NDT_S1, NDT_S2, NDT_MEAN, NDT_COV, NDT_ICOV = range(6)
# name, element type and elements per voxel of lv_ndt_fetch's layers
NDT_LAYERS = (("count", np.uint32, 1), ("S1", np.int64, 3), ("S2", np.int64, 6), ("mean", np.float64, 3), ("cov", np.float64, 6),
              ("icov", np.float64, 6))
# the same bytes as NdtResult
NDT_RESULT_DTYPE = np.dtype([("t", "f8", 3), ("q", "f8", 4), ("score", "f8"), ("info", "f8", 21), ("last_step", "f8"), ("lambda", "f8"),
                             ("n_in", "u4"), ("status", "i4"), ("accepted", "u4"), ("rejected", "u4")])

# ctypes signatures of the NDT registration (include/limovelo_hip.h "NDT registration"; tests/test_ndt_abi.py)
NDT_ARGTYPES = {
    "lv_ndt_build": [C.c_void_p, C.POINTER(NdtParams), C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)],
    "lv_ndt_add": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)],
    "lv_ndt_fetch": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "lv_ndt_align": [C.c_void_p, C.POINTER(NdtAlignParams), C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(GraphPose), C.c_size_t,
                     C.POINTER(NdtResult), C.POINTER(C.c_int32)],
    "lv_ndt_info": [C.c_void_p, C.POINTER(NdtTargetInfo)],
    "lv_ndt_clear": [C.c_void_p],
}


class SurfAlignParams(C.Structure):  # lv_surf_align_params (64 bytes)
    _fields_ = [("min_weight", C.c_int32), ("max_iterations", C.c_int32), ("min_points", C.c_uint32), ("reserved", C.c_int32),
                ("max_dist", C.c_double), ("huber", C.c_double), ("step_tol", C.c_double), ("lambda_init", C.c_double),
                ("lambda_min", C.c_double), ("lambda_max", C.c_double)]


class SurfAlignResult(C.Structure):  # lv_surf_align_result (264 bytes): lv_ndt_result with cost for score
    _fields_ = [("pose", GraphPose), ("cost", C.c_double), ("info", C.c_double * 21), ("last_step", C.c_double), ("lambda_", C.c_double),
                ("n_in", C.c_uint32), ("status", C.c_int32), ("accepted", C.c_uint32), ("rejected", C.c_uint32)]


SURF_SAMPLE_OUTSIDE, SURF_SAMPLE_UNKNOWN, SURF_SAMPLE_KNOWN = 0, 1, 2
SURF_ALIGN_CONVERGED, SURF_ALIGN_MAX_ITERATIONS, SURF_ALIGN_NO_OVERLAP = 0, 1, 2
SURF_ALIGN_CHUNK = 512   # LV_SURF_ALIGN_CHUNK: source points per workgroup of the evaluation
# the same bytes as SurfAlignResult
SURF_ALIGN_RESULT_DTYPE = np.dtype([("t", "f8", 3), ("q", "f8", 4), ("cost", "f8"), ("info", "f8", 21), ("last_step", "f8"), ("lambda", "f8"),
                                    ("n_in", "u4"), ("status", "i4"), ("accepted", "u4"), ("rejected", "u4")])

# ctypes signatures of the surface registration (include/limovelo_hip.h "Surface registration"; tests/test_surf_align_abi.py)
SURF_ALIGN_ARGTYPES = {
    "lv_surf_sample": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_uint8)],
    "lv_surf_align": [C.c_void_p, C.POINTER(SurfAlignParams), C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(GraphPose), C.c_size_t,
                      C.POINTER(SurfAlignResult), C.POINTER(C.c_int32)],
}


LV_MERGE_TRILINEAR, LV_MERGE_NEAREST = 0, 1


class SurfSubmap(C.Structure):  # lv_surf_submap (48 bytes)
    _fields_ = [("origin", C.c_float * 3), ("resolution", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("trunc_cells", C.c_int),
                ("S", C.POINTER(C.c_int32)), ("W", C.POINTER(C.c_int32))]


class SurfMergeParams(C.Structure):  # lv_surf_merge_params (16 bytes)
    _fields_ = [("min_weight", C.c_int32), ("interp", C.c_int32), ("reserved", C.c_int32 * 2)]


# ctypes signatures of the submap merge (include/limovelo_hip.h "Submap merging"; tests/test_surf_merge_abi.py)
SURF_MERGE_ARGTYPES = {
    "lv_surf_merge": [C.c_void_p, C.POINTER(SurfSubmap), C.POINTER(GraphPose), C.POINTER(SurfMergeParams), C.POINTER(C.c_uint64)],
}


class OccupancyParams(C.Structure):  # lv_occupancy_params
    _fields_ = [("origin", C.c_float * 3), ("resolution", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("min_range", C.c_float), ("max_range", C.c_float), ("l_hit", C.c_float), ("l_miss", C.c_float), ("l_min", C.c_float),
                ("l_max", C.c_float), ("l_occ", C.c_float), ("l_free", C.c_float)]


# ctypes signatures of the occupancy grid (include/limovelo_hip.h "Occupancy grid"; tests/test_occupancy_abi.py)
OCCUPANCY_ARGTYPES = {
    "lv_occ_configure": [C.c_void_p, C.POINTER(OccupancyParams)],
    "lv_occ_integrate": [C.c_void_p, C.POINTER(View), C.c_size_t, C.POINTER(C.c_uint64)],
    "lv_occ_query": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_float)],
    "lv_occ_project": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int8), C.c_size_t],
    "lv_occ_fetch": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t],
    "lv_occ_load": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t],
    "lv_occ_clear": [C.c_void_p],
    "lv_occ_get_params": [C.c_void_p, C.POINTER(OccupancyParams)],
}

LV_OCC_FAR = 2147483647


class DistanceParams(C.Structure):  # lv_distance_params
    _fields_ = [("planar", C.c_int), ("k_lo", C.c_int), ("k_hi", C.c_int), ("unknown_is_obstacle", C.c_int), ("signed_field", C.c_int),
                ("max_cells", C.c_int)]


class DistanceInfo(C.Structure):  # lv_distance_info
    _fields_ = [("built", C.c_int), ("planar", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("stale", C.c_int),
                ("params", DistanceParams)]


# ctypes signatures of the distance field (include/limovelo_hip.h "Distance field"; tests/test_occ_distance_abi.py)
DISTANCE_ARGTYPES = {
    "lv_occ_distance_build": [C.c_void_p, C.POINTER(DistanceParams), C.POINTER(C.c_uint64)],
    "lv_occ_distance_fetch": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_size_t],
    "lv_occ_distance_query": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "lv_occ_distance_info": [C.c_void_p, C.POINTER(DistanceInfo)],
    "lv_occ_distance_clear": [C.c_void_p],
}

LV_PLAN_UNREACHED = 0xFFFFFFFF


class PlanParams(C.Structure):  # lv_plan_params
    _fields_ = [("connectivity", C.c_int), ("min_clear_s2", C.c_int)]


class PlanInfo(C.Structure):  # lv_plan_info
    _fields_ = [("built", C.c_int), ("planar", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("stale", C.c_int),
                ("rounds", C.c_int), ("params", PlanParams)]


# ctypes signatures of the planner (include/limovelo_hip.h "Planner"; tests/test_occ_plan_abi.py)
PLAN_ARGTYPES = {
    "lv_occ_plan_build": [C.c_void_p, C.POINTER(PlanParams), C.POINTER(C.c_uint8), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                          C.POINTER(C.c_uint64)],
    "lv_occ_plan_fetch": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t],
    "lv_occ_plan_paths": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                          C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)],
    "lv_occ_plan_info": [C.c_void_p, C.POINTER(PlanInfo)],
    "lv_occ_plan_clear": [C.c_void_p],
}

LV_LATTICE_REACH, LV_LATTICE_MAX_SWEEP, LV_LATTICE_UNREACHED = 8, 10, 0xFFFFFFFF


class LatticePrim(C.Structure):  # lv_lattice_prim (32 bytes)
    _fields_ = [("di", C.c_int8), ("dj", C.c_int8), ("h_to", C.c_uint8), ("n_sweep", C.c_uint8), ("length", C.c_uint16), ("reserved", C.c_uint16),
                ("penalty", C.c_uint32), ("sweep", (C.c_int8 * 2) * LV_LATTICE_MAX_SWEEP)]


# the same record as a numpy dtype (Context.occ_lattice_build, limo_velo_amd.lattice)
LATTICE_PRIM_DTYPE = np.dtype([("di", np.int8), ("dj", np.int8), ("h_to", np.uint8), ("n_sweep", np.uint8), ("length", np.uint16),
                               ("reserved", np.uint16), ("penalty", np.uint32), ("sweep", np.int8, (LV_LATTICE_MAX_SWEEP, 2))])
assert LATTICE_PRIM_DTYPE.itemsize == C.sizeof(LatticePrim) == 32
# a goal or start record: a world point and a heading bin (-1: any)
LATTICE_POSE_DTYPE = np.dtype([("xyz", np.float32, 3), ("h", np.int32)])


class LatticeParams(C.Structure):  # lv_lattice_params
    _fields_ = [("H", C.c_int), ("P", C.c_int)]


class LatticeInfo(C.Structure):  # lv_lattice_info
    _fields_ = [("built", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("H", C.c_int), ("P", C.c_int), ("stale", C.c_int), ("rounds", C.c_int),
                ("tile", C.c_int), ("reach", C.c_int), ("params", LatticeParams)]


# ctypes signatures of the lattice planner (include/limovelo_hip.h "Lattice planner")
LATTICE_ARGTYPES = {
    "lv_occ_lattice_build": [C.c_void_p, C.POINTER(LatticeParams), C.POINTER(LatticePrim), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                             C.POINTER(C.c_uint64)],
    "lv_occ_lattice_fetch": [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t],
    "lv_occ_lattice_paths": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                             C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)],
    "lv_occ_lattice_info": [C.c_void_p, C.POINTER(LatticeInfo)],
    "lv_occ_lattice_clear": [C.c_void_p],
}

LV_FRONTIER_NONE = -1


class FrontierParams(C.Structure):  # lv_frontier_params
    _fields_ = [("planar", C.c_int), ("k_lo", C.c_int), ("k_hi", C.c_int), ("connectivity", C.c_int), ("min_size", C.c_int)]


class FrontierInfo(C.Structure):  # lv_frontier_info
    _fields_ = [("built", C.c_int), ("planar", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("stale", C.c_int),
                ("n_clusters", C.c_int), ("params", FrontierParams)]


class FrontierCluster(C.Structure):  # lv_frontier_cluster (72 bytes)
    _fields_ = [("size", C.c_int32), ("first", C.c_int32), ("rep", C.c_int32), ("centre", C.c_int32 * 3), ("lo", C.c_int32 * 3),
                ("hi", C.c_int32 * 3), ("sum", C.c_uint64 * 3)]


# the same record as a numpy dtype (Context.occ_frontier_clusters)
FRONTIER_CLUSTER_DTYPE = np.dtype([("size", np.int32), ("first", np.int32), ("rep", np.int32), ("centre", np.int32, 3), ("lo", np.int32, 3),
                                   ("hi", np.int32, 3), ("sum", np.uint64, 3)])

# ctypes signatures of the frontiers (include/limovelo_hip.h "Frontiers"; tests/test_occ_frontier_abi.py)
FRONTIER_ARGTYPES = {
    "lv_occ_frontier_build": [C.c_void_p, C.POINTER(FrontierParams), C.POINTER(C.c_uint64)],
    "lv_occ_frontier_fetch": [C.c_void_p, C.POINTER(C.c_int32), C.c_size_t],
    "lv_occ_frontier_clusters": [C.c_void_p, C.POINTER(FrontierCluster), C.c_size_t, C.POINTER(C.c_size_t)],
    "lv_occ_frontier_rank": [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_size_t],
    "lv_occ_frontier_info": [C.c_void_p, C.POINTER(FrontierInfo)],
    "lv_occ_frontier_clear": [C.c_void_p],
}

LV_RAY_IGNORED, LV_RAY_CLEAR, LV_RAY_STOPPED = 0, 1, 2


class RayParams(C.Structure):  # lv_ray_params
    _fields_ = [("stop_unknown", C.c_int)]


class RayResult(C.Structure):  # lv_ray_result (32 bytes)
    _fields_ = [("status", C.c_int32), ("cell", C.c_int32), ("steps", C.c_int32), ("axis", C.c_int32), ("n_free", C.c_int32),
                ("n_unknown", C.c_int32), ("num", C.c_int32), ("den", C.c_int32)]


# the same record as a numpy dtype (Context.occ_raycast)
RAY_RESULT_DTYPE = np.dtype([(f, np.int32) for f, _ in RayResult._fields_])

# ctypes signatures of the ray casting (include/limovelo_hip.h "Ray casting"; tests/test_occ_ray_abi.py)
RAY_ARGTYPES = {
    "lv_occ_raycast": [C.c_void_p, C.POINTER(RayParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(RayResult)],
    "lv_occ_view_gain": [C.c_void_p, C.POINTER(View), C.c_size_t, C.POINTER(C.c_uint64)],
}

LV_ELEV_NONE = 2147483647
(LV_ELEV_LO, LV_ELEV_TOP, LV_ELEV_SPAN, LV_ELEV_STEP, LV_ELEV_SLOPE2, LV_ELEV_COUNT, LV_ELEV_BAND_COUNT, LV_ELEV_CLASS,
 LV_ELEV_HEIGHT) = range(9)
# name and numpy type of every layer of lv_elev_fetch, by its number
ELEV_LAYERS = (("lo", np.int32), ("top", np.int32), ("span", np.int32), ("step", np.int32), ("slope2", np.int32), ("count", np.uint32),
               ("band_count", np.uint32), ("cls", np.int8), ("height", np.float32))


class ElevationParams(C.Structure):  # lv_elevation_params
    _fields_ = [("origin", C.c_float * 3), ("resolution", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("min_points", C.c_int),
                ("head", C.c_int), ("max_span", C.c_int), ("max_step", C.c_int), ("max_slope2", C.c_int)]


class ElevationInfo(C.Structure):  # lv_elevation_info
    _fields_ = [("built", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("from_map", C.c_int), ("n_points", C.c_uint64),
                ("params", ElevationParams)]


# ctypes signatures of the elevation map (include/limovelo_hip.h "Elevation map"; tests/test_elevation_abi.py)
ELEVATION_ARGTYPES = {
    "lv_elev_build": [C.c_void_p, C.POINTER(ElevationParams), C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)],
    "lv_elev_fetch": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "lv_elev_query": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_int8)],
    "lv_elev_info": [C.c_void_p, C.POINTER(ElevationInfo)],
    "lv_elev_clear": [C.c_void_p],
    "lv_occ_distance_build_cells": [C.c_void_p, C.POINTER(DistanceParams), C.POINTER(C.c_int8), C.c_size_t, C.POINTER(C.c_uint64)],
}

LV_ROLLOUT_CLEAR, LV_ROLLOUT_STOPPED = 1, 2


class RolloutParams(C.Structure):  # lv_rollout_params
    _fields_ = [("T", C.c_int), ("Tc", C.c_int), ("dt", C.c_float), ("fp_clear_s2", C.c_int), ("w_cost", C.c_uint32), ("w_goal", C.c_uint32),
                ("w_stop", C.c_uint32), ("min_steps", C.c_int), ("goal_mode", C.c_int)]


class RolloutResult(C.Structure):  # lv_rollout_result (32 bytes)
    _fields_ = [("status", C.c_int32), ("steps", C.c_int32), ("why", C.c_int32), ("cell_end", C.c_int32), ("p_end", C.c_uint32),
                ("p_min", C.c_uint32), ("s_min", C.c_int32), ("cost_sum", C.c_uint32)]


# the same record as a numpy dtype (Context.occ_rollout)
ROLLOUT_RESULT_DTYPE = np.dtype([(f, np.uint32 if t is C.c_uint32 else np.int32) for f, t in RolloutResult._fields_])

# ctypes signatures of the rollouts (include/limovelo_hip.h "Rollouts"; tests/test_occ_rollout_abi.py)
ROLLOUT_ARGTYPES = {
    "lv_occ_rollout": [C.c_void_p, C.POINTER(RolloutParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float),
                       C.c_size_t, C.POINTER(RolloutResult), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)],
}


class MclParams(C.Structure):  # lv_mcl_params
    _fields_ = [("out_cost", C.c_uint32), ("min_inside", C.c_int)]


MCL_NO_SCORE = 2 ** 64 - 1

# ctypes signatures of the localisation (include/limovelo_hip.h "Localisation"; tests/test_occ_mcl_abi.py)
MCL_ARGTYPES = {
    "lv_occ_mcl_weigh": [C.c_void_p, C.POINTER(MclParams), C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.c_size_t,
                         C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)],
}


class MclResampleParams(C.Structure):  # lv_mcl_resample_params
    _fields_ = [("shift", C.c_int), ("mode", C.c_int), ("below_num", C.c_uint32), ("below_den", C.c_uint32)]


class MclFilterStats(C.Structure):  # lv_mcl_filter_stats
    _fields_ = [("W", C.c_uint64), ("sum_w2", C.c_uint64), ("s_min", C.c_int64), ("S", C.c_int64 * 5), ("n_eligible", C.c_uint32),
                ("n_clamped", C.c_uint32), ("resampled", C.c_int), ("epoch", C.c_uint32), ("since_resample", C.c_uint32),
                ("origin", C.c_float * 3), ("resolution", C.c_float)]


class MclFilterInfo(C.Structure):  # lv_mcl_filter_info
    _fields_ = [("K", C.c_uint64), ("seed", C.c_uint64), ("set", C.c_int), ("epoch", C.c_uint32), ("since_resample", C.c_uint32)]


# ctypes signatures of the resident localisation filter (include/limovelo_hip.h "Resident localisation filter";
# tests/test_occ_mcl_filter_abi.py)
MCL_FILTER_ARGTYPES = {
    "lv_occ_mcl_filter_set": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_uint64],
    "lv_occ_mcl_filter_move": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "lv_occ_mcl_filter_weigh": [C.c_void_p, C.POINTER(MclParams), C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t,
                                C.POINTER(C.c_int64)],
    "lv_occ_mcl_filter_resample": [C.c_void_p, C.POINTER(MclResampleParams), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(MclFilterStats),
                                   C.POINTER(C.c_uint32)],
    "lv_occ_mcl_filter_get": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t],
    "lv_occ_mcl_filter_info": [C.c_void_p, C.POINTER(MclFilterInfo)],
    "lv_occ_mcl_filter_clear": [C.c_void_p],
}


OBS_POSITION, OBS_VELOCITY_WORLD, OBS_VELOCITY_BODY, OBS_ATTITUDE = 1, 2, 3, 4   # LV_OBS_*
OBSERVE_BATCH = 8   # LV_OBSERVE_BATCH


class Observation(C.Structure):  # lv_observation
    _fields_ = [("kind", C.c_int), ("mask", C.c_int), ("z", C.c_double * 4), ("R", C.c_double * 9), ("lever", C.c_double * 3),
                ("gate", C.c_double)]


class ObserveResult(C.Structure):  # lv_observe_result
    _fields_ = [("status", C.c_int), ("rows", C.c_int), ("nis", C.c_double), ("y", C.c_double * 3)]


# ctypes signatures of the aiding observations (include/limovelo_hip.h "Aiding observations"; tests/test_observe_abi.py)
OBSERVE_ARGTYPES = {
    "lv_observe": [C.c_void_p, C.POINTER(Observation), C.c_size_t, C.POINTER(ObserveResult)],
    "lv_observe_results": [C.c_void_p, C.POINTER(ObserveResult), C.c_size_t, C.POINTER(C.c_size_t)],
}


def default_observation(kind: int, **kw) -> Observation:
    o = Observation()
    load_library().lv_default_observation(C.byref(o), int(kind))
    for k, v in kw.items():
        if k in ("z", "R", "lever"):
            a = np.asarray(v, np.float64).ravel()
            arr = getattr(o, k)
            assert a.size <= len(arr), (k, a.size)
            for i, t in enumerate(a):
                arr[i] = float(t)
        else:
            setattr(o, k, v)
    return o


class TsdfParams(C.Structure):  # lv_tsdf_params
    _fields_ = [("origin", C.c_float * 3), ("resolution", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("min_range", C.c_float), ("max_range", C.c_float), ("trunc_cells", C.c_int), ("max_weight", C.c_int), ("carve", C.c_int)]


class MeshInfo(C.Structure):  # lv_mesh_info
    _fields_ = [("built", C.c_int), ("stale", C.c_int), ("min_weight", C.c_int), ("reserved", C.c_int), ("vertices", C.c_uint64),
                ("triangles", C.c_uint64), ("active_cells", C.c_uint64), ("refused_edges", C.c_uint64)]


# ctypes signatures of the TSDF and its mesh (include/limovelo_hip.h "TSDF and mesh"; tests/test_tsdf_abi.py)
TSDF_ARGTYPES = {
    "lv_tsdf_configure": [C.c_void_p, C.POINTER(TsdfParams)],
    "lv_tsdf_integrate": [C.c_void_p, C.POINTER(View), C.c_size_t, C.POINTER(C.c_uint64)],
    "lv_tsdf_query": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_int32)],
    "lv_tsdf_fetch": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_size_t],
    "lv_tsdf_load": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t],
    "lv_tsdf_clear": [C.c_void_p],
    "lv_tsdf_get_params": [C.c_void_p, C.POINTER(TsdfParams)],
    "lv_tsdf_mesh_build": [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)],
    "lv_tsdf_mesh_fetch": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t],
    "lv_tsdf_mesh_info": [C.c_void_p, C.POINTER(MeshInfo)],
    "lv_tsdf_mesh_clear": [C.c_void_p],
}


LV_DEPTH_U16, LV_DEPTH_F32 = 0, 1
DEPTH_DTYPES = {LV_DEPTH_U16: np.dtype(np.uint16), LV_DEPTH_F32: np.dtype(np.float32)}


class DepthView(C.Structure):  # lv_depth_view
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("dist", C.c_float * 5), ("width", C.c_int), ("height", C.c_int), ("format", C.c_int), ("depth_scale", C.c_float),
                ("depth", C.c_void_p), ("row_stride", C.c_size_t)]


class DepthParams(C.Structure):  # lv_depth_params
    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("max_norm_radius", C.c_float), ("carve", C.c_int), ("reserved", C.c_int)]


# ctypes signatures of the depth fusion (include/limovelo_hip.h "Depth fusion"; tests/test_depth_abi.py)
DEPTH_ARGTYPES = {
    "lv_depth_integrate": [C.c_void_p, C.POINTER(DepthView), C.c_size_t, C.POINTER(DepthParams), C.POINTER(C.c_uint64)],
}


def depth_view(frame):
    """(DepthView, depth array it points into) from a frame dict: R [3, 3] and t [3] camera -> world, fx, fy, cx, cy, depth ([h, w]
    uint16: LV_DEPTH_U16, or float32: LV_DEPTH_F32, metres; rows may be strided), optional depth_scale (metres per unit of a
    uint16 image, default 0.001) and dist (k1, k2, p1, p2, k3)."""
    img = np.asarray(frame["depth"])
    if img.ndim != 2 or img.dtype not in (np.uint16, np.float32):
        raise ValueError("depth must be a 2-D uint16 or float32 array")
    if img.strides[1] != img.itemsize or img.strides[0] < img.shape[1] * img.itemsize:
        img = np.ascontiguousarray(img)
    v = DepthView()
    v.R[:] = [float(x) for x in np.asarray(frame["R"], np.float32).ravel()]
    v.t[:] = [float(x) for x in np.asarray(frame["t"], np.float32).ravel()]
    v.fx, v.fy, v.cx, v.cy = (float(frame[k]) for k in ("fx", "fy", "cx", "cy"))
    dist = frame.get("dist")
    v.dist[:] = [float(x) for x in np.asarray(np.zeros(5) if dist is None else dist, np.float32).ravel()]
    v.height, v.width = int(img.shape[0]), int(img.shape[1])
    v.format = LV_DEPTH_U16 if img.dtype == np.uint16 else LV_DEPTH_F32
    v.depth_scale = float(frame.get("depth_scale", 0.001))
    v.depth = img.ctypes.data
    v.row_stride = int(img.strides[0])
    return v, img


class ColourParams(C.Structure):  # lv_colour_params
    _fields_ = [("view", LvPaintParams), ("band", C.c_int), ("min_weight", C.c_int), ("max_weight", C.c_int), ("reserved", C.c_int)]


class ColourInfo(C.Structure):  # struct lv_colour_info
    _fields_ = [("present", C.c_int), ("reserved", C.c_int), ("voxels", C.c_uint64), ("coloured", C.c_uint64)]


# ctypes signatures of the colour layer (include/limovelo_hip.h "Colour layer"; tests/test_colour_abi.py)
COLOUR_ARGTYPES = {
    "lv_colour_integrate": [C.c_void_p, C.POINTER(LvCameraView), C.c_size_t, C.POINTER(ColourParams), C.POINTER(C.c_uint64)],
    "lv_colour_fetch": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_size_t],
    "lv_colour_load": [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t],
    "lv_colour_query": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8)],
    "lv_colour_clear": [C.c_void_p],
    "lv_colour_info": [C.c_void_p, C.POINTER(ColourInfo)],
    "lv_mesh_colours": [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t],
}

LV_SURF_IGNORED, LV_SURF_CLEAR, LV_SURF_HIT, LV_SURF_BLOCKED = 0, 1, 2, 3


class TsdfRayParams(C.Structure):  # lv_tsdf_ray_params
    _fields_ = [("min_weight", C.c_int), ("reserved", C.c_int)]


class TsdfRayResult(C.Structure):  # lv_tsdf_ray_result (32 bytes)
    _fields_ = [("status", C.c_int32), ("cell", C.c_int32), ("steps", C.c_int32), ("axis", C.c_int32), ("depth", C.c_int32),
                ("t", C.c_int32), ("n_known", C.c_int32), ("n_unknown", C.c_int32)]


# the same record as a numpy dtype (Context.tsdf_raycast)
TSDF_RAY_RESULT_DTYPE = np.dtype([(f, np.int32) for f, _ in TsdfRayResult._fields_])

# ctypes signatures of the surface ray casting (include/limovelo_hip.h "Surface ray casting"; tests/test_tsdf_ray_abi.py)
TSDF_RAY_ARGTYPES = {
    "lv_surf_raycast": [C.c_void_p, C.POINTER(TsdfRayParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                        C.POINTER(TsdfRayResult), C.POINTER(C.c_float), C.POINTER(C.c_uint8)],
    "lv_surf_raycast_views": [C.c_void_p, C.POINTER(TsdfRayParams), C.POINTER(View), C.c_size_t, C.POINTER(TsdfRayResult), C.POINTER(C.c_float),
                              C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint64)],
}


LV_VOLUME_OCC, LV_VOLUME_SURFACE = 0, 1
VOLUME_SHIFT_LIMIT = 1 << 20


class VolumeShifts(C.Structure):  # lv_volume_shifts
    _fields_ = [("grid", C.c_int32 * 3), ("surface", C.c_int32 * 3), ("field", C.c_int32 * 3), ("plan", C.c_int32 * 3),
                ("frontier", C.c_int32 * 3)]


class OccMarkParams(C.Structure):  # lv_occ_mark_params
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("min_points", C.c_int), ("only_unknown", C.c_int), ("l_mark", C.c_float)]


# ctypes signatures of the rolling volumes (include/limovelo_hip.h "Rolling volumes"; tests/test_volume_recentre_abi.py)
VOLUME_ARGTYPES = {
    "lv_volume_recentre": [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)],
    "lv_volume_shift_info": [C.c_void_p, C.POINTER(VolumeShifts)],
    "lv_occ_mark": [C.c_void_p, C.POINTER(OccMarkParams), C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)],
}


LV_OCC_SURFACE_FILL, LV_OCC_SURFACE_OVERWRITE, LV_OCC_SURFACE_REPLACE, LV_OCC_SURFACE_ACCUMULATE = 0, 1, 2, 3


class OccSurfaceParams(C.Structure):  # lv_occ_surface_params
    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3), ("min_weight", C.c_int), ("band", C.c_int), ("reach", C.c_int), ("mode", C.c_int),
                ("l_solid", C.c_float), ("l_open", C.c_float)]


# ctypes signatures of the way from the surface to the grid (include/limovelo_hip.h "Occupancy from the surface"; tests/test_surf_occ_abi.py)
OCC_SURFACE_ARGTYPES = {
    "lv_occ_from_surface": [C.c_void_p, C.POINTER(OccSurfaceParams), C.POINTER(C.c_uint64)],
}


def camera_view(frame):
    """(LvCameraView, image array it points into) from a frame dict: R [3, 3] and t [3] camera -> world, fx, fy, cx, cy, image
    ([h, w, 3] or [h, w] uint8; rows may be strided), optional format (LV_IMAGE_*; default RGB8, MONO8 for a 2-D image) and dist
    (k1, k2, p1, p2, k3)."""
    img = np.asarray(frame["image"])
    if img.dtype != np.uint8:
        raise ValueError("image must be uint8")
    fmt = int(frame.get("format", LV_IMAGE_MONO8 if img.ndim == 2 else LV_IMAGE_RGB8))
    ch = IMAGE_CHANNELS.get(fmt)
    if ch is None or img.ndim != (2 if ch == 1 else 3) or (ch == 3 and img.shape[2] != 3):
        raise ValueError(f"image of shape {img.shape} does not match format {fmt}")
    if not (img.strides[-1] == 1 and (ch == 1 or img.strides[1] == 3)):
        img = np.ascontiguousarray(img)
    v = LvCameraView()
    v.R[:] = [float(x) for x in np.asarray(frame["R"], np.float32).ravel()]
    v.t[:] = [float(x) for x in np.asarray(frame["t"], np.float32).ravel()]
    v.fx, v.fy, v.cx, v.cy = (float(frame[k]) for k in ("fx", "fy", "cx", "cy"))
    v.dist[:] = [float(x) for x in np.asarray(frame.get("dist", np.zeros(5)), np.float32).ravel()]
    v.height, v.width = int(img.shape[0]), int(img.shape[1])
    v.format = fmt
    v.image = img.ctypes.data
    v.row_stride = int(img.strides[0])
    return v, img


def camera_pose(state, R_IC, t_IC):
    """(R [3, 3] f32, t [3] f32): the camera -> world pose of an lv_state (26 f64) and the camera -> IMU extrinsic (R_IC, t_IC):
    R = R_WI R_IC, t = R_WI t_IC + p_WI, composed in f64 (the IMU rotation from the state's quaternion qx, qy, qz, qw), rounded
    to f32 once."""
    x = np.asarray(state, np.float64).ravel()
    qx, qy, qz, qw = x[3:7]
    R_WI = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                     [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                     [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    R_IC = np.asarray(R_IC, np.float64).reshape(3, 3)
    t_IC = np.asarray(t_IC, np.float64).ravel()
    return (R_WI @ R_IC).astype(np.float32), (R_WI @ t_IC + x[0:3]).astype(np.float32)


def sensor_pose(state):
    """(R [3, 3] f32, t [3] f32): the sensor -> world pose Xt2 * Xt2.I_Rt_L() of an lv_state (26 f64), formed as lv_map_add_scan
    forms it on the device (lv_device.hpp compute_pose_consts: rotations from the quaternions in f64, rounded to f32, composed in
    f32 with each sum taken as p0 + (p1 + p2))."""
    x = np.asarray(state, np.float64).ravel()

    def rot(q):
        qx, qy, qz, qw = q
        tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
        twx, twy, twz = tx * qw, ty * qw, tz * qw
        txx, txy, txz = tx * qx, ty * qx, tz * qx
        tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
        return np.array([1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx,
                         txz - twy, tyz + twx, 1.0 - (txx + tyy)]).astype(np.float32)

    def dot3(a0, b0, a1, b1, a2, b2):
        return np.float32(a0 * b0) + np.float32(np.float32(a1 * b1) + np.float32(a2 * b2))

    XR, LR = rot(x[3:7]), rot(x[7:11])
    Xt, Lt = x[0:3].astype(np.float32), x[11:14].astype(np.float32)
    R = np.empty(9, np.float32)
    t = np.empty(3, np.float32)
    for i in range(3):
        for j in range(3):
            R[i * 3 + j] = dot3(XR[i * 3], LR[j], XR[i * 3 + 1], LR[3 + j], XR[i * 3 + 2], LR[6 + j])
        t[i] = np.float32(dot3(XR[i * 3], Lt[0], XR[i * 3 + 1], Lt[1], XR[i * 3 + 2], Lt[2]) + Xt[i])
    return R.reshape(3, 3), t


def pseudo_measurement(sums: dict, estimate_extrinsics: bool):
    """lv_pseudo_measurement: (h_x [rows, 12], h [rows]) with h_x^T h_x = H^T H and h_x^T h = H^T h — the Eigen-free half of
    IKFoM::h_share_model for an unmodified esekf loop (host arithmetic: no context, no device)."""
    rec = Sums()
    HTH = np.ascontiguousarray(sums["HTH"], np.float64).ravel()
    for i in range(144):
        rec.HTH[i] = HTH[i]
    for i in range(12):
        rec.HTh[i] = float(sums["HTh"][i])
    rec.sum_h2 = float(sums.get("sum_h2", 0.0))
    rec.n_valid = int(sums.get("n_valid", 1))
    hx = np.zeros((12, 12))
    h = np.zeros(12)
    rows = C.c_int(0)
    lib = load_library()
    lib.lv_pseudo_measurement.argtypes = [C.POINTER(Sums), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    if lib.lv_pseudo_measurement(C.byref(rec), int(bool(estimate_extrinsics)), hx.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                                 C.byref(rows)) != LV_OK:
        raise RuntimeError(lib.lv_last_error().decode())
    return hx[: rows.value].copy(), h[: rows.value].copy()


def pass_geometry(n_scan: int, n_cus: int = 256):
    """(searching workgroups, steps per round, rounds, dedicated bookkeeper) of pass_kernel — host logic only."""
    out = (C.c_int * 4)()
    lib = load_library()
    lib.lv_pass_geometry.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_int)]
    if lib.lv_pass_geometry(n_scan, n_cus, out) != LV_OK:
        raise RuntimeError(lib.lv_last_error().decode())
    return tuple(int(v) for v in out)


class CloudFormat(C.Structure):  # lv_cloud_format
    _fields_ = [("point_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32),
                ("off_time", C.c_uint32), ("time_type", C.c_int), ("off_intensity", C.c_uint32), ("intensity_type", C.c_int),
                ("off_range", C.c_uint32), ("range_type", C.c_int), ("relative_time", C.c_int)]


class IngestParams(C.Structure):  # lv_ingest_params
    _fields_ = [("header_stamp_usec", C.c_uint64), ("stamp_beginning", C.c_int), ("offset_beginning", C.c_int),
                ("full_rotation_time", C.c_double), ("downsample_rate", C.c_int), ("min_dist", C.c_float)]


POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("pad_", "f4"), ("time", "f8"), ("intensity", "f4"), ("range", "f4")])
LIDAR_VELODYNE, LIDAR_HESAI, LIDAR_OUSTER, LIDAR_CUSTOM = 0, 1, 2, 3
SCAN_ROUTE_NONE, SCAN_ROUTE_SMALL, SCAN_ROUTE_LARGE, SCAN_ROUTE_GENERAL = 0, 1, 2, 3   # LV_SCAN_ROUTE_*


class Params(C.Structure):
    _fields_ = [
        ("MAX_NUM_ITERS", C.c_int),
        ("NUM_MATCH_POINTS", C.c_int),
        ("MAX_DIST_PLANE", C.c_double),
        ("PLANES_THRESHOLD", C.c_float),
        ("estimate_extrinsics", C.c_int),
        ("LiDAR_noise", C.c_double),
        ("LIMITS", C.c_double * NS),
        ("degeneracy_threshold", C.c_double),
        ("voxel_size", C.c_float),
        ("lanes_per_query", C.c_int),
        ("degeneracy_mode", C.c_int),
        ("print_degeneracy_values", C.c_int),
    ]


class Sums(C.Structure):
    _fields_ = [("HTH", C.c_double * 144), ("HTh", C.c_double * 12), ("sum_h2", C.c_double), ("n_valid", C.c_int64)]

    def as_dict(self):
        return dict(HTH=np.array(self.HTH).reshape(12, 12), HTh=np.array(self.HTh), sum_h2=float(self.sum_h2),
                    n_valid=int(self.n_valid))


class Timing(C.Structure):
    _fields_ = [("last_update_ms", C.c_float), ("last_reduce_ms", C.c_float), ("last_solve_ms", C.c_float),
                ("last_passes", C.c_int), ("fallback_queries", C.c_int), ("pass_match_ms", C.c_float * 8),
                ("pass_solve_ms", C.c_float * 8), ("mailbox_resyncs", C.c_int), ("pass_collective_ms", C.c_float * 8)]


# lv_motion_state (include/limovelo_hip.h): the f32 State members State::propagate_f reads, 184 bytes
MOTION_DTYPE = np.dtype([("R", "f4", 9), ("pos", "f4", 3), ("vel", "f4", 3), ("bw", "f4", 3), ("ba", "f4", 3), ("g", "f4", 3),
                         ("RLI", "f4", 9), ("tLI", "f4", 3), ("a", "f4", 3), ("w", "f4", 3), ("pad_", "f4", 2), ("time", "f8")])
assert MOTION_DTYPE.itemsize == 184


def motion_state(time=0.0, R=None, pos=(0, 0, 0), vel=(0, 0, 0), a=(0, 0, 9.807), w=(0, 0, 0), RLI=None, tLI=(0, 0, 0),
                 g=(0, 0, -9.807), bw=(0, 0, 0), ba=(0, 0, 0)) -> np.ndarray:
    """One lv_motion_state record (a numpy array of length 1)."""
    s = np.zeros(1, MOTION_DTYPE)
    s["R"] = np.eye(3, dtype=np.float32).ravel() if R is None else np.asarray(R, np.float32).ravel()
    s["RLI"] = np.eye(3, dtype=np.float32).ravel() if RLI is None else np.asarray(RLI, np.float32).ravel()
    for k, v in (("pos", pos), ("vel", vel), ("a", a), ("w", w), ("tLI", tLI), ("g", g), ("bw", bw), ("ba", ba)):
        s[k] = np.asarray(v, np.float32)
    s["time"] = time
    return s


class MapStats(C.Structure):  # lv_map_stats
    _fields_ = [("living", C.c_uint64), ("ids", C.c_uint64), ("capacity", C.c_uint64), ("pool_used", C.c_uint64 * 4),
                ("pool_cap", C.c_uint64 * 4), ("slots_used", C.c_uint64 * 4), ("slots_cap", C.c_uint64 * 4),
                ("tombstones", C.c_uint64), ("dropped", C.c_uint64), ("relinearisations", C.c_uint64),
                ("incremental_adds", C.c_uint64), ("bytes", C.c_uint64)]


class LvError(RuntimeError):
    pass


_lib = None


def load_library() -> C.CDLL:
    """dlopen liblimovelo_hip.so.  Raises (never falls back) if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LvError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        lib.lv_last_error.restype = C.c_char_p
        lib.lv_version.restype = C.c_char_p
        lib.lv_scan_size.restype = C.c_size_t
        lib.lv_scan_size.argtypes = [C.c_void_p]
        lib.lv_scan_route.restype = C.c_int
        lib.lv_scan_route.argtypes = [C.c_void_p]
        lib.lv_map_size.restype = C.c_size_t
        lib.lv_cloud_size.restype = C.c_size_t
        lib.lv_cloud_size.argtypes = [C.c_void_p]
        lib.lv_map_size.argtypes = [C.c_void_p]
        lib.lv_get_stream.restype = C.c_void_p
        lib.lv_get_stream.argtypes = [C.c_void_p]
        lib.lv_sums_device_ptr.restype = C.c_void_p
        lib.lv_sums_device_ptr.argtypes = [C.c_void_p]
        lib.lv_destroy.restype = None
        lib.lv_destroy.argtypes = [C.c_void_p]
        lib.lv_default_params.restype = None
        lib.lv_default_visibility_params.restype = None
        lib.lv_default_visibility_params.argtypes = [C.POINTER(VisibilityParams)]
        lib.lv_default_paint_params.restype = None
        lib.lv_default_paint_params.argtypes = [C.POINTER(LvPaintParams)]
        lib.lv_default_surface_params.restype = None
        lib.lv_default_surface_params.argtypes = [C.POINTER(SurfaceParams)]
        lib.lv_default_outlier_params.restype = None
        lib.lv_default_outlier_params.argtypes = [C.POINTER(OutlierParams)]
        lib.lv_default_cluster_params.restype = None
        lib.lv_default_cluster_params.argtypes = [C.POINTER(ClusterParams)]
        lib.lv_default_plane_params.restype = None
        lib.lv_default_plane_params.argtypes = [C.POINTER(PlaneParams)]
        lib.lv_default_place_params.restype = None
        lib.lv_default_place_params.argtypes = [C.POINTER(PlaceParams)]
        lib.lv_place_count.restype = C.c_size_t
        lib.lv_place_count.argtypes = [C.c_void_p]
        lib.lv_default_occupancy_params.restype = None
        lib.lv_default_occupancy_params.argtypes = [C.POINTER(OccupancyParams)]
        lib.lv_default_distance_params.restype = None
        lib.lv_default_distance_params.argtypes = [C.POINTER(DistanceParams)]
        lib.lv_default_plan_params.restype = None
        lib.lv_default_plan_params.argtypes = [C.POINTER(PlanParams)]
        lib.lv_default_lattice_params.restype = None
        lib.lv_default_lattice_params.argtypes = [C.POINTER(LatticeParams)]
        lib.lv_default_frontier_params.restype = None
        lib.lv_default_frontier_params.argtypes = [C.POINTER(FrontierParams)]
        lib.lv_default_ray_params.restype = None
        lib.lv_default_ray_params.argtypes = [C.POINTER(RayParams)]
        lib.lv_default_elevation_params.restype = None
        lib.lv_default_elevation_params.argtypes = [C.POINTER(ElevationParams)]
        lib.lv_default_rollout_params.restype = None
        lib.lv_default_rollout_params.argtypes = [C.POINTER(RolloutParams)]
        lib.lv_default_mcl_params.restype = None
        lib.lv_default_mcl_params.argtypes = [C.POINTER(MclParams)]
        lib.lv_default_mcl_resample_params.restype = None
        lib.lv_default_mcl_resample_params.argtypes = [C.POINTER(MclResampleParams)]
        lib.lv_default_tsdf_params.restype = None
        lib.lv_default_tsdf_params.argtypes = [C.POINTER(TsdfParams)]
        lib.lv_default_depth_params.restype = None
        lib.lv_default_depth_params.argtypes = [C.POINTER(DepthParams)]
        lib.lv_default_colour_params.restype = None
        lib.lv_default_colour_params.argtypes = [C.POINTER(ColourParams)]
        lib.lv_default_surf_ray_params.restype = None
        lib.lv_default_surf_ray_params.argtypes = [C.POINTER(TsdfRayParams)]
        lib.lv_default_occ_mark_params.restype = None
        lib.lv_default_occ_mark_params.argtypes = [C.POINTER(OccMarkParams)]
        lib.lv_default_observation.restype = None
        lib.lv_default_observation.argtypes = [C.POINTER(Observation), C.c_int]
        lib.lv_default_graph_params.restype = None
        lib.lv_default_graph_params.argtypes = [C.POINTER(GraphParams)]
        lib.lv_default_traj_smooth_params.restype = None
        lib.lv_default_traj_smooth_params.argtypes = [C.POINTER(TrajSmoothParams)]
        lib.lv_default_traj_register_params.restype = None
        lib.lv_default_traj_register_params.argtypes = [C.POINTER(TrajRegisterParams)]
        lib.lv_default_ndt_params.restype = None
        lib.lv_default_ndt_params.argtypes = [C.POINTER(NdtParams)]
        lib.lv_default_ndt_align_params.restype = None
        lib.lv_default_ndt_align_params.argtypes = [C.POINTER(NdtAlignParams)]
        lib.lv_default_surf_align_params.restype = None
        lib.lv_default_surf_align_params.argtypes = [C.POINTER(SurfAlignParams)]
        lib.lv_default_surf_merge_params.restype = None
        lib.lv_default_surf_merge_params.argtypes = [C.POINTER(SurfMergeParams)]
        lib.lv_default_occ_surface_params.restype = None
        lib.lv_default_occ_surface_params.argtypes = [C.POINTER(OccSurfaceParams)]
        for name, argtypes in {**QUERY_ARGTYPES, **BATCH_ARGTYPES, **VISIBILITY_ARGTYPES, **PAINT_ARGTYPES, **PLACE_ARGTYPES, **SURFACE_ARGTYPES,
                               **CLUSTER_ARGTYPES, **PLANE_ARGTYPES, **OCCUPANCY_ARGTYPES, **DISTANCE_ARGTYPES, **PLAN_ARGTYPES, **LATTICE_ARGTYPES,
                               **FRONTIER_ARGTYPES,
                               **RAY_ARGTYPES, **ELEVATION_ARGTYPES, **ROLLOUT_ARGTYPES, **MCL_ARGTYPES, **MCL_FILTER_ARGTYPES, **TSDF_ARGTYPES, **DEPTH_ARGTYPES, **COLOUR_ARGTYPES, **TSDF_RAY_ARGTYPES, **VOLUME_ARGTYPES,
                               **OBSERVE_ARGTYPES, **GRAPH_ARGTYPES, **TRAJ_ARGTYPES, **NDT_ARGTYPES, **SURF_ALIGN_ARGTYPES,
                               **OCC_SURFACE_ARGTYPES, **SURF_MERGE_ARGTYPES}.items():
            getattr(lib, name).argtypes = argtypes
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


def default_params(**kw) -> Params:
    p = Params()
    load_library().lv_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "LIMITS":
            for i in range(NS):
                p.LIMITS[i] = float(v[i])
        else:
            setattr(p, k, v)
    return p


def default_visibility_params(**kw) -> VisibilityParams:
    p = VisibilityParams()
    load_library().lv_default_visibility_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_paint_params(**kw) -> LvPaintParams:
    p = LvPaintParams()
    load_library().lv_default_paint_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_surface_params(**kw) -> SurfaceParams:
    p = SurfaceParams()
    load_library().lv_default_surface_params(C.byref(p))
    for k, v in kw.items():
        if k == "viewpoint":
            p.viewpoint[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_outlier_params(**kw) -> OutlierParams:
    p = OutlierParams()
    load_library().lv_default_outlier_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_cluster_params(**kw) -> ClusterParams:
    p = ClusterParams()
    load_library().lv_default_cluster_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_plane_params(**kw) -> PlaneParams:
    p = PlaneParams()
    load_library().lv_default_plane_params(C.byref(p))
    for k, v in kw.items():
        if k == "axis":
            p.axis[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_place_params(**kw) -> PlaceParams:
    p = PlaceParams()
    load_library().lv_default_place_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_traj_smooth_params(**kw) -> TrajSmoothParams:
    p = TrajSmoothParams()
    load_library().lv_default_traj_smooth_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_traj_register_params(extrapolate=None, frame=None, ext_t=None, ext_q=None, frame_time=None) -> TrajRegisterParams:
    p = TrajRegisterParams()
    load_library().lv_default_traj_register_params(C.byref(p))
    if extrapolate is not None:
        p.extrapolate = int(extrapolate)
    if frame is not None:
        p.frame = int(frame)
    if ext_t is not None:
        p.ext_t[:] = [float(v) for v in ext_t]
    if ext_q is not None:
        p.ext_q[:] = [float(v) for v in ext_q]
    if frame_time is not None:
        p.frame_time = float(frame_time)
    return p


def traj_knots(times, poses) -> np.ndarray:
    """TRAJ_KNOT_DTYPE records from times [n] and poses [n, 7] (t, q = x y z w)."""
    x = np.asarray(poses, np.float64).reshape(-1, 7)
    k = np.zeros(len(x), TRAJ_KNOT_DTYPE)
    k["time"], k["t"], k["q"] = np.asarray(times, np.float64).reshape(-1), x[:, :3], x[:, 3:]
    return k


def default_graph_params(**kw) -> GraphParams:
    p = GraphParams()
    load_library().lv_default_graph_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_ndt_params(**kw) -> NdtParams:
    p = NdtParams()
    load_library().lv_default_ndt_params(C.byref(p))
    for k, v in kw.items():
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_ndt_align_params(**kw) -> NdtAlignParams:
    p = NdtAlignParams()
    load_library().lv_default_ndt_align_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_surf_merge_params(**kw) -> SurfMergeParams:
    p = SurfMergeParams()
    load_library().lv_default_surf_merge_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def surf_submap(origin, resolution, trunc_cells, S, W):
    """(SurfSubmap, the int32 arrays it points into) from a volume as Context.tsdf_fetch gives it: S and W [nz, ny, nx]."""
    a = np.ascontiguousarray(S, np.int32)
    b = np.ascontiguousarray(W, np.int32)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError("surf_submap: S and W of one [nz, ny, nx] shape")
    m = SurfSubmap()
    m.origin[:] = [float(v) for v in origin]
    m.resolution = float(resolution)
    m.nz, m.ny, m.nx = (int(v) for v in a.shape)
    m.trunc_cells = int(trunc_cells)
    m.S = a.ctypes.data_as(C.POINTER(C.c_int32))
    m.W = b.ctypes.data_as(C.POINTER(C.c_int32))
    return m, (a, b)


def default_surf_align_params(**kw) -> SurfAlignParams:
    p = SurfAlignParams()
    load_library().lv_default_surf_align_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_occupancy_params(**kw) -> OccupancyParams:
    p = OccupancyParams()
    load_library().lv_default_occupancy_params(C.byref(p))
    for k, v in kw.items():
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_distance_params(**kw) -> DistanceParams:
    p = DistanceParams()
    load_library().lv_default_distance_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_plan_params(**kw) -> PlanParams:
    p = PlanParams()
    load_library().lv_default_plan_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_lattice_params(**kw) -> LatticeParams:
    p = LatticeParams()
    load_library().lv_default_lattice_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def lattice_poses(poses) -> np.ndarray:
    """Goal or start records (LATTICE_POSE_DTYPE) from records, or from rows (x, y, z, h): h the heading bin, -1 for any."""
    a = np.asarray(poses)
    if a.dtype == LATTICE_POSE_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.asarray(a, np.float64).reshape(-1, 4)
    out = np.zeros(len(a), LATTICE_POSE_DTYPE)
    out["xyz"] = a[:, :3].astype(np.float32)
    out["h"] = a[:, 3].astype(np.int32)
    return out


def default_frontier_params(**kw) -> FrontierParams:
    p = FrontierParams()
    load_library().lv_default_frontier_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_ray_params(**kw) -> RayParams:
    p = RayParams()
    load_library().lv_default_ray_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_elevation_params(**kw) -> ElevationParams:
    p = ElevationParams()
    load_library().lv_default_elevation_params(C.byref(p))
    for k, v in kw.items():
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_rollout_params(**kw) -> RolloutParams:
    p = RolloutParams()
    load_library().lv_default_rollout_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_mcl_params(**kw) -> MclParams:
    p = MclParams()
    load_library().lv_default_mcl_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_mcl_resample_params(**kw) -> MclResampleParams:
    p = MclResampleParams()
    load_library().lv_default_mcl_resample_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_tsdf_params(**kw) -> TsdfParams:
    p = TsdfParams()
    load_library().lv_default_tsdf_params(C.byref(p))
    for k, v in kw.items():
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_depth_params(**kw) -> DepthParams:
    p = DepthParams()
    load_library().lv_default_depth_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_colour_params(**kw) -> ColourParams:
    """lv_default_colour_params; a keyword that names a field of lv_paint_params (zbuf_scale, window, margin_abs, ...) sets it in
    the embedded `view`."""
    p = ColourParams()
    load_library().lv_default_colour_params(C.byref(p))
    own = {f for f, _ in ColourParams._fields_}
    for k, v in kw.items():
        setattr(p if k in own else p.view, k, v)
    return p


def default_tsdf_ray_params(**kw) -> TsdfRayParams:
    p = TsdfRayParams()
    load_library().lv_default_surf_ray_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_occ_mark_params(**kw) -> OccMarkParams:
    p = OccMarkParams()
    load_library().lv_default_occ_mark_params(C.byref(p))
    for k, v in kw.items():
        if k in ("lo", "hi"):
            getattr(p, k)[:] = [int(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def default_occ_surface_params(**kw) -> OccSurfaceParams:
    p = OccSurfaceParams()
    load_library().lv_default_occ_surface_params(C.byref(p))
    for k, v in kw.items():
        if k in ("lo", "hi"):
            getattr(p, k)[:] = [int(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def view_array(views):
    """(lv_view array, the point arrays it refers to) from views = [(R [3, 3], t [3], points [n, 3] sensor frame)]."""
    keep = []
    arr = (View * max(len(views), 1))()
    for i, (R, t, pts) in enumerate(views):
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3)) if len(pts) else (None, 12, 0)
        keep.append(a)
        arr[i].R[:] = [float(v) for v in np.asarray(R, np.float32).ravel()]
        arr[i].t[:] = [float(v) for v in np.asarray(t, np.float32).ravel()]
        arr[i].points = a.ctypes.data if a is not None else None
        arr[i].stride = stride
        arr[i].n = n
    return arr, keep


def _points(a):
    """Accepts [N,3] float32 (stride 12) or a structured/2-D array with a custom byte stride."""
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] < 3 or not a.flags["C_CONTIGUOUS"]:
        a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.strides[0], a.shape[0]


class Context:
    def __init__(self, params: Params | None = None, device: int = 0):
        self.lib = load_library()
        self.params = params or default_params()
        self.h = C.c_void_p()
        self._check(self.lib.lv_create(C.byref(self.params), int(device), C.byref(self.h)))
        # pre-bound buffers for the hot call (keeps the Python overhead of update() at a few microseconds)
        self._xb = np.zeros(26)
        self._Pb = np.zeros((NS, NS))
        self._passes = C.c_int(0)
        self._xp = self._xb.ctypes.data_as(C.c_void_p)
        self._Pp = self._Pb.ctypes.data_as(C.c_void_p)
        self._passes_ref = C.byref(self._passes)

    def _check(self, rc):
        if rc != LV_OK:
            raise LvError(f"limovelo_hip error {rc}: {self.lib.lv_last_error().decode()}")

    def close(self):
        if self.h:
            self.lib.lv_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- Mapper side
    def map_build(self, pts):
        a, stride, n = _points(pts)
        self._check(self.lib.lv_map_build(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n)))

    def map_add(self, pts, downsample=False):
        a, stride, n = _points(pts)
        self._check(self.lib.lv_map_add(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                        int(bool(downsample))))

    def map_add_scan(self, downsample=True):
        """The mapping step on the device: current scan -> world with the device-held state -> insert."""
        self._check(self.lib.lv_map_add_scan(self.h, int(bool(downsample))))

    def map_evict_box(self, lo, hi, keep_inside=True) -> int:
        lo = np.ascontiguousarray(lo, np.float32)
        hi = np.ascontiguousarray(hi, np.float32)
        n = C.c_size_t(0)
        self._check(self.lib.lv_map_evict_box(self.h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), int(bool(keep_inside)),
                                              C.byref(n)))
        return int(n.value)

    def map_evict_oldest(self, n_oldest: int) -> int:
        n = C.c_size_t(0)
        self._check(self.lib.lv_map_evict_oldest(self.h, C.c_size_t(n_oldest), C.byref(n)))
        return int(n.value)

    def map_relinearise_async(self):
        self._check(self.lib.lv_map_relinearise_async(self.h))

    def map_reserve_rebuild(self):
        """lv_map_reserve_rebuild: the second store of the background rebuild allocated (and touched) now, at set-up time."""
        self._check(self.lib.lv_map_reserve_rebuild(self.h))

    def map_rebuild_status(self, wait=False) -> dict:
        out = (C.c_uint64 * 4)()
        self._check(self.lib.lv_map_rebuild_status(self.h, C.c_int(int(wait)), out))
        return dict(state=int(out[0]), started=int(out[1]), adopted=int(out[2]), journal=int(out[3]))

    def map_relinearise(self):
        self._check(self.lib.lv_map_relinearise(self.h))

    def map_stats(self) -> dict:
        st = MapStats()
        self._check(self.lib.lv_map_get_stats(self.h, C.byref(st)))
        return {k: (list(getattr(st, k)) if k in ("pool_used", "pool_cap", "slots_used", "slots_cap") else int(getattr(st, k)))
                for k, _ in MapStats._fields_}

    def map_size(self) -> int:
        return int(self.lib.lv_map_size(self.h))

    def map_fetch(self) -> np.ndarray:
        n = self.map_size()
        out = np.empty((n, 3), np.float32)
        self._check(self.lib.lv_map_fetch(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out

    # --- map queries (ikd-Tree Nearest_Search / Radius_Search / Box_Search)
    def map_knn(self, q, k, max_dist=np.inf):
        """(idx [n, k] uint32, d2 [n, k] float32, found [n] int32): the k nearest living points of every query, ascending
        (d2, index); unfilled slots 0xFFFFFFFF / +inf.  Indices are ranks among the living (map_fetch order)."""
        a, stride, n = _points(q)
        kk = max(int(k), 1)   # (an out-of-range k still goes to the library, which refuses it)
        idx = np.empty((n, kk), np.uint32)
        d2 = np.empty((n, kk), np.float32)
        found = np.empty(n, np.int32)
        self._check(self.lib.lv_map_knn(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n), int(k), C.c_float(max_dist),
                                        idx.ctypes.data_as(C.POINTER(C.c_uint32)), d2.ctypes.data_as(C.POINTER(C.c_float)),
                                        found.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx, d2, found

    def map_radius_count(self, q, radius):
        """(offsets [n + 1] uint64, total): the count-only form of lv_map_radius_search."""
        a, stride, n = _points(q)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_size_t(0)
        self._check(self.lib.lv_map_radius_search(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n), C.c_float(radius),
                                                  off.ctypes.data_as(C.POINTER(C.c_size_t)), None, None, C.c_size_t(0), C.byref(total)))
        return off, int(total.value)

    def map_radius(self, q, radius):
        """(offsets [n + 1], idx [total] uint32, d2 [total] float32), CSR: query i's points are idx[offsets[i]:offsets[i + 1]],
        ascending index.  Counts first, then fills."""
        a, stride, n = _points(q)
        off, total = self.map_radius_count(a, radius)
        idx = np.empty(total, np.uint32)
        d2 = np.empty(total, np.float32)
        t = C.c_size_t(0)
        self._check(self.lib.lv_map_radius_search(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n), C.c_float(radius),
                                                  off.ctypes.data_as(C.POINTER(C.c_size_t)), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  d2.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(total), C.byref(t)))
        return off, idx, d2

    def map_box(self, lo, hi):
        """(idx [n] uint32, xyz [n, 3] float32): the living points inside [lo, hi] (faces inclusive), ascending index."""
        lo = np.ascontiguousarray(lo, np.float32)
        hi = np.ascontiguousarray(hi, np.float32)
        fp = C.POINTER(C.c_float)
        cnt = C.c_size_t(0)
        self._check(self.lib.lv_map_box_search(self.h, lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), None, None, C.c_size_t(0), C.byref(cnt)))
        n = int(cnt.value)
        idx = np.empty(n, np.uint32)
        xyz = np.empty((n, 3), np.float32)
        self._check(self.lib.lv_map_box_search(self.h, lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               xyz.ctypes.data_as(fp), C.c_size_t(n), C.byref(cnt)))
        return idx[: int(cnt.value)], xyz[: int(cnt.value)]

    # --- Localizator side
    # --- dynamic-point removal
    def map_remove_dynamic(self, views, params: VisibilityParams | None = None, dry_run=False):
        """(n_removed, hits [map_size] uint8): lv_map_remove_dynamic over views = [(R [3, 3], t [3], points [n, 3] sensor frame)],
        R, t the sensor -> world pose (sensor_pose); hits in map order as the map stood before the removal."""
        p = VisibilityParams.from_buffer_copy(params) if params is not None else default_visibility_params()
        p.dry_run = int(bool(dry_run) or bool(p.dry_run))
        keep = []
        arr = (View * max(len(views), 1))()
        for i, (R, t, pts) in enumerate(views):
            a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3)) if len(pts) else (None, 12, 0)
            keep.append(a)
            arr[i].R[:] = [float(v) for v in np.asarray(R, np.float32).ravel()]
            arr[i].t[:] = [float(v) for v in np.asarray(t, np.float32).ravel()]
            arr[i].points = a.ctypes.data if a is not None else None
            arr[i].stride = stride
            arr[i].n = n
        hits = np.zeros(self.map_size(), np.uint8)
        nr = C.c_size_t(0)
        self._check(self.lib.lv_map_remove_dynamic(self.h, arr, C.c_size_t(len(views)), C.byref(p),
                                                   hits.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nr)))
        return int(nr.value), hits

    # --- surface normals and outlier removal
    def map_normals(self, params: SurfaceParams | None = None):
        """dict(normals [m, 3] f32, curvature [m] f32, mean_dist [m] f32, n_used [m] int32) in map order: lv_map_normals."""
        p = params if params is not None else default_surface_params()
        m = self.map_size()
        out = dict(normals=np.zeros((m, 3), np.float32), curvature=np.zeros(m, np.float32), mean_dist=np.zeros(m, np.float32),
                   n_used=np.zeros(m, np.int32))
        fp = C.POINTER(C.c_float)
        self._check(self.lib.lv_map_normals(self.h, C.byref(p), out["normals"].ctypes.data_as(fp), out["curvature"].ctypes.data_as(fp),
                                            out["mean_dist"].ctypes.data_as(fp), out["n_used"].ctypes.data_as(C.POINTER(C.c_int32)),
                                            C.c_size_t(m)))
        return out

    def map_remove_outliers(self, params: OutlierParams | None = None, dry_run=False):
        """(n_removed, flags [map_size] uint8, stats [3] = mu, sigma, threshold): lv_map_remove_outliers; flags in map order as the
        map stood before the removal."""
        p = OutlierParams.from_buffer_copy(params) if params is not None else default_outlier_params()
        p.dry_run = int(bool(dry_run) or bool(p.dry_run))
        flags = np.zeros(self.map_size(), np.uint8)
        stats = np.zeros(3)
        nr = C.c_size_t(0)
        self._check(self.lib.lv_map_remove_outliers(self.h, C.byref(p), flags.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nr),
                                                    stats.ctypes.data_as(C.POINTER(C.c_double))))
        return int(nr.value), flags, stats

    # --- map clustering
    def _point_bytes(self, a, what):
        """mask / seeds: one byte per living point in map order (None stays None)."""
        if a is None:
            return None, None
        a = np.ascontiguousarray(np.asarray(a).reshape(-1) != 0, np.uint8)
        if len(a) != self.map_size():
            raise ValueError(f"{what}: {len(a)} entries for a map of {self.map_size()} points")
        return a, a.ctypes.data_as(C.POINTER(C.c_uint8))

    def map_cluster(self, params: ClusterParams | None = None, mask=None) -> dict:
        """dict(labels [m] int32 in map order (-1: in no reported cluster), sizes [C] uint32 in label order, n_clusters = C):
        lv_map_cluster; mask: None or [m] in map order, 0 = excluded."""
        p = params if params is not None else default_cluster_params()
        m = self.map_size()
        keep, mp = self._point_bytes(mask, "mask")
        labels = np.full(m, -1, np.int32)
        sizes = np.zeros(m, np.uint32)   # (C <= m)
        C_ = C.c_size_t(0)
        self._check(self.lib.lv_map_cluster(self.h, C.byref(p), mp, labels.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(m),
                                            sizes.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(m), C.byref(C_)))
        n = int(C_.value)
        return dict(labels=labels, sizes=sizes[:n].copy(), n_clusters=n)

    def map_remove_clusters(self, params: ClusterParams | None = None, mask=None, seeds=None, dry_run=False) -> dict:
        """dict(flags [m] uint8 in map order as the map stood before the removal, n_removed): lv_map_remove_clusters; seeds None:
        components below min_size leave; seeds [m]: the components within [min_size, max_size] that hold a seeded point leave."""
        p = ClusterParams.from_buffer_copy(params) if params is not None else default_cluster_params()
        p.dry_run = int(bool(dry_run) or bool(p.dry_run))
        keep_m, mp = self._point_bytes(mask, "mask")
        keep_s, sp = self._point_bytes(seeds, "seeds")
        flags = np.zeros(self.map_size(), np.uint8)
        nr = C.c_size_t(0)
        self._check(self.lib.lv_map_remove_clusters(self.h, C.byref(p), mp, sp, flags.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nr)))
        return dict(flags=flags, n_removed=int(nr.value))

    # --- plane segmentation
    def map_planes(self, params: PlaneParams | None = None, mask=None) -> dict:
        """dict(labels [m] int32 in map order (the plane's index in extraction order, -1: on no plane), planes [P] records
        (PLANE_DTYPE) in extraction order, n_planes = P): lv_map_planes; mask: None or [m] in map order, 0 = excluded."""
        p = params if params is not None else default_plane_params()
        m = self.map_size()
        keep, mp = self._point_bytes(mask, "mask")
        labels = np.full(m, -1, np.int32)
        planes = np.zeros(PLANE_MAX_PLANES, PLANE_DTYPE)
        P = C.c_size_t(0)
        self._check(self.lib.lv_map_planes(self.h, C.byref(p), mp, labels.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(m),
                                           planes.ctypes.data_as(C.POINTER(Plane)), C.c_size_t(PLANE_MAX_PLANES), C.byref(P)))
        n = int(P.value)
        return dict(labels=labels, planes=planes[:n].copy(), n_planes=n)

    # --- map painting
    def map_paint(self, views, params: LvPaintParams | None = None):
        """(rgb [m, 3] f32, depth [m] f32, n_seen [m] uint8) in map order: lv_map_paint over views = [frame dict (camera_view)]."""
        p = params if params is not None else default_paint_params()
        arr = (LvCameraView * max(len(views), 1))()
        keep = []
        for i, f in enumerate(views):
            arr[i], img = camera_view(f)
            keep.append(img)
        m = self.map_size()
        rgb = np.zeros((m, 3), np.float32)
        depth = np.full(m, np.inf, np.float32)
        seen = np.zeros(m, np.uint8)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.lv_map_paint(self.h, arr, C.c_size_t(len(views)), C.byref(p), rgb.ctypes.data_as(fp), depth.ctypes.data_as(fp),
                                          seen.ctypes.data_as(C.POINTER(C.c_uint8))))
        return rgb, depth, seen

    # --- occupancy grid (include/limovelo_hip.h "Occupancy grid")
    def occ_configure(self, params: OccupancyParams | None = None):
        """lv_occ_configure: allocates the grid (default: lv_default_occupancy_params), every voxel unknown."""
        p = params if params is not None else default_occupancy_params()
        self._check(self.lib.lv_occ_configure(self.h, C.byref(p)))

    def occ_params(self) -> OccupancyParams:
        p = OccupancyParams()
        self._check(self.lib.lv_occ_get_params(self.h, C.byref(p)))
        return p

    def occ_integrate(self, views) -> np.ndarray:
        """lv_occ_integrate over views = [(R [3, 3], t [3], points [n, 3] sensor frame)] (1..32 of them, the tuples of
        map_remove_dynamic); returns stats [4] uint64: rays used, rays cut, voxel updates free, voxel updates hit."""
        arr, keep = view_array(views)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_integrate(self.h, arr, C.c_size_t(len(views)), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def occ_query(self, pts) -> np.ndarray:
        """[n] f32: the log-odds of the voxel each world point falls in, NaN outside the grid / unknown."""
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3))
        out = np.full(n, np.nan, np.float32)
        self._check(self.lib.lv_occ_query(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                          out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def occ_project(self, k_lo: int, k_hi: int) -> np.ndarray:
        """[ny, nx] int8 (100 occupied, 0 free, -1 unknown) over the layers k_lo..k_hi: lv_occ_project."""
        p = self.occ_params()
        out = np.full((p.ny, p.nx), -1, np.int8)
        self._check(self.lib.lv_occ_project(self.h, int(k_lo), int(k_hi), out.ctypes.data_as(C.POINTER(C.c_int8)), C.c_size_t(out.size)))
        return out

    def occ_fetch(self) -> np.ndarray:
        """[nz, ny, nx] f32 log-odds, NaN = never observed."""
        p = self.occ_params()
        out = np.zeros((p.nz, p.ny, p.nx), np.float32)
        self._check(self.lib.lv_occ_fetch(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size)))
        return out

    def occ_load(self, logodds):
        a = np.ascontiguousarray(logodds, np.float32)
        self._check(self.lib.lv_occ_load(self.h, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(a.size)))

    def occ_clear(self):
        self._check(self.lib.lv_occ_clear(self.h))

    # --- distance field (include/limovelo_hip.h "Distance field")
    def occ_distance_build(self, params: DistanceParams | None = None) -> np.ndarray:
        """lv_occ_distance_build (default: 3-D, unknown = free, unsigned, untruncated); returns stats [4] uint64: obstacles, voxels
        with a finite value, the largest finite d2_out, the largest finite d2_in."""
        p = params if params is not None else default_distance_params()
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_distance_build(self.h, C.byref(p), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def occ_distance_info(self) -> DistanceInfo:
        out = DistanceInfo()
        self._check(self.lib.lv_occ_distance_info(self.h, C.byref(out)))
        return out

    def occ_distance_fetch(self, s2=True, metres=True):
        """(s2 int32, metres f32), each [nz, ny, nx] ([ny, nx] of a planar field) or None where not asked for."""
        i = self.occ_distance_info()
        if not i.built:   # (the library's own refusal)
            self._check(self.lib.lv_occ_distance_fetch(self.h, None, (C.c_float * 1)(), C.c_size_t(0)))
        shape = (i.ny, i.nx) if i.planar else (i.nz, i.ny, i.nx)
        a = np.zeros(shape, np.int32) if s2 else None
        m = np.zeros(shape, np.float32) if metres else None
        self._check(self.lib.lv_occ_distance_fetch(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)) if s2 else None,
                                                   m.ctypes.data_as(C.POINTER(C.c_float)) if metres else None,
                                                   C.c_size_t(int(np.prod(shape)))))
        return a, m

    def occ_distance_query(self, pts, want_grad=True):
        """(dist [n] f32 metres, grad [n, 3] f32 or None) at the voxel of each world point; dist NaN outside the grid."""
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3))
        dist = np.full(n, np.nan, np.float32)
        grad = np.zeros((n, 3), np.float32) if want_grad else None
        self._check(self.lib.lv_occ_distance_query(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                                   dist.ctypes.data_as(C.POINTER(C.c_float)),
                                                   grad.ctypes.data_as(C.POINTER(C.c_float)) if want_grad else None))
        return dist, grad

    def occ_distance_clear(self):
        self._check(self.lib.lv_occ_distance_clear(self.h))

    # --- planner (include/limovelo_hip.h "Planner")
    def occ_plan_build(self, goals, cost_table, params: PlanParams | None = None) -> np.ndarray:
        """lv_occ_plan_build over the distance field last built: goals [n, 3] world points, cost_table uint8 [n_cost] (every entry
        1..255; entry t is the cost of a cell isqrt(s2) = t cells from the nearest obstacle), params default 8-connected with
        min_clear_s2 1.  Returns stats [4] uint64: goals used, traversable cells, reached cells, the largest finite P."""
        p = params if params is not None else default_plan_params()
        a, stride, n = _points(np.asarray(goals, np.float32).reshape(-1, 3))
        table = np.ascontiguousarray(cost_table, np.uint8).reshape(-1)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_plan_build(self.h, C.byref(p), table.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(table.size),
                                               a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                               stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def occ_plan_info(self) -> PlanInfo:
        out = PlanInfo()
        self._check(self.lib.lv_occ_plan_info(self.h, C.byref(out)))
        return out

    def occ_plan_fetch(self, potential=True, cell_cost=True):
        """(potential uint32, cell_cost uint8), each [nz, ny, nx] ([ny, nx] of a planar plan) or None where not asked for."""
        i = self.occ_plan_info()
        if not i.built:   # (the library's own refusal)
            self._check(self.lib.lv_occ_plan_fetch(self.h, (C.c_uint32 * 1)(), None, C.c_size_t(0)))
        shape = (i.ny, i.nx) if i.planar else (i.nz, i.ny, i.nx)
        pot = np.zeros(shape, np.uint32) if potential else None
        cc = np.zeros(shape, np.uint8) if cell_cost else None
        self._check(self.lib.lv_occ_plan_fetch(self.h, pot.ctypes.data_as(C.POINTER(C.c_uint32)) if potential else None,
                                               cc.ctypes.data_as(C.POINTER(C.c_uint8)) if cell_cost else None,
                                               C.c_size_t(int(np.prod(shape)))))
        return pot, cc

    def occ_plan_paths(self, starts):
        """(status [n] int32, cost [n] uint32, offsets [n + 1] uint64, cells [total] int32), CSR: start i's path is
        cells[offsets[i]:offsets[i + 1]], linear cell indices from the start cell to a goal cell.  Counts first, then fills."""
        a, stride, n = _points(np.asarray(starts, np.float32).reshape(-1, 3))
        status = np.full(n, 2, np.int32)
        cost = np.full(n, LV_PLAN_UNREACHED, np.uint32)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_size_t(0)
        args = (self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n), status.ctypes.data_as(C.POINTER(C.c_int32)),
                cost.ctypes.data_as(C.POINTER(C.c_uint32)), off.ctypes.data_as(C.POINTER(C.c_size_t)))
        self._check(self.lib.lv_occ_plan_paths(*args, None, C.c_size_t(0), C.byref(total)))
        cells = np.empty(int(total.value), np.int32)
        if cells.size:
            self._check(self.lib.lv_occ_plan_paths(*args, cells.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(cells.size), C.byref(total)))
        return status, cost, off, cells

    def occ_plan_clear(self):
        self._check(self.lib.lv_occ_plan_clear(self.h))

    # --- lattice planner (include/limovelo_hip.h "Lattice planner")
    def occ_lattice_build(self, goals, prims, params: LatticeParams | None = None) -> np.ndarray:
        """lv_occ_lattice_build over the planar plan last built: goals as lattice_poses takes them, prims the table as
        LATTICE_PRIM_DTYPE records of shape [H, P] (params default: the table's shape).  Returns stats [4] uint64: goals used,
        traversable states, reached states, the largest finite V."""
        t = np.ascontiguousarray(prims, LATTICE_PRIM_DTYPE)
        p = params if params is not None else default_lattice_params(H=t.shape[0], P=t.shape[1] if t.ndim > 1 else 1)
        g = lattice_poses(goals)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_lattice_build(self.h, C.byref(p), t.ctypes.data_as(C.POINTER(LatticePrim)), C.c_size_t(t.size),
                                                  g.ctypes.data_as(C.c_void_p), C.c_size_t(LATTICE_POSE_DTYPE.itemsize), C.c_size_t(len(g)),
                                                  stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def occ_lattice_info(self) -> LatticeInfo:
        out = LatticeInfo()
        self._check(self.lib.lv_occ_lattice_info(self.h, C.byref(out)))
        return out

    def occ_lattice_fetch(self) -> np.ndarray:
        """V, uint32 [H, ny, nx]."""
        i = self.occ_lattice_info()
        if not i.built:   # (the library's own refusal)
            self._check(self.lib.lv_occ_lattice_fetch(self.h, (C.c_uint32 * 1)(), C.c_size_t(0)))
        V = np.zeros((i.H, i.ny, i.nx), np.uint32)
        self._check(self.lib.lv_occ_lattice_fetch(self.h, V.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(V.size)))
        return V

    def occ_lattice_paths(self, starts):
        """(status [n] int32, cost [n] uint32, offsets [n + 1] uint64, states [total] int32, prims [total] uint8), CSR: start i's
        path is states[offsets[i]:offsets[i + 1]], linear state indices from the start state to a goal state; prims the primitive
        taken out of each state, 255 at a path's last.  Counts first, then fills."""
        a = lattice_poses(starts)
        n = len(a)
        status = np.full(n, 2, np.int32)
        cost = np.full(n, LV_LATTICE_UNREACHED, np.uint32)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_size_t(0)
        args = (self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(LATTICE_POSE_DTYPE.itemsize), C.c_size_t(n), status.ctypes.data_as(C.POINTER(C.c_int32)),
                cost.ctypes.data_as(C.POINTER(C.c_uint32)), off.ctypes.data_as(C.POINTER(C.c_size_t)))
        self._check(self.lib.lv_occ_lattice_paths(*args, None, None, C.c_size_t(0), C.byref(total)))
        states = np.empty(int(total.value), np.int32)
        taken = np.empty(int(total.value), np.uint8)
        if states.size:
            self._check(self.lib.lv_occ_lattice_paths(*args, states.ctypes.data_as(C.POINTER(C.c_int32)), taken.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                      C.c_size_t(states.size), C.byref(total)))
        return status, cost, off, states, taken

    def occ_lattice_clear(self):
        self._check(self.lib.lv_occ_lattice_clear(self.h))

    # --- frontiers (include/limovelo_hip.h "Frontiers")
    def occ_frontier_build(self, params: FrontierParams | None = None) -> np.ndarray:
        """lv_occ_frontier_build (default: 3-D, 26-connected, min_size 1); returns stats [4] uint64: FREE cells, UNKNOWN cells,
        frontier cells, clusters reported."""
        p = params if params is not None else default_frontier_params()
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_frontier_build(self.h, C.byref(p), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def occ_frontier_info(self) -> FrontierInfo:
        out = FrontierInfo()
        self._check(self.lib.lv_occ_frontier_info(self.h, C.byref(out)))
        return out

    def occ_frontier_fetch(self) -> np.ndarray:
        """The labels, int32 [nz, ny, nx] ([ny, nx] of a planar result): the cluster's number on its members, -1 elsewhere."""
        i = self.occ_frontier_info()
        if not i.built:   # (the library's own refusal)
            self._check(self.lib.lv_occ_frontier_fetch(self.h, (C.c_int32 * 1)(), C.c_size_t(0)))
        out = np.full((i.ny, i.nx) if i.planar else (i.nz, i.ny, i.nx), LV_FRONTIER_NONE, np.int32)
        self._check(self.lib.lv_occ_frontier_fetch(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(out.size)))
        return out

    def occ_frontier_clusters(self) -> np.ndarray:
        """The clusters in label order as a structured array (FRONTIER_CLUSTER_DTYPE).  Counts first, then fills."""
        n = C.c_size_t(0)
        self._check(self.lib.lv_occ_frontier_clusters(self.h, None, C.c_size_t(0), C.byref(n)))
        out = np.zeros(int(n.value), FRONTIER_CLUSTER_DTYPE)
        if out.size:
            self._check(self.lib.lv_occ_frontier_clusters(self.h, out.ctypes.data_as(C.POINTER(FrontierCluster)), C.c_size_t(out.size), C.byref(n)))
        return out

    def occ_frontier_rank(self, reach: int = 0):
        """(best_p uint32 [C], best_cell int32 [C]) over the plan last built: per cluster the least potential within Chebyshev
        distance `reach` of a member and the cell that has it (LV_PLAN_UNREACHED and -1 where nothing is reached)."""
        n = int(self.occ_frontier_info().n_clusters)
        p = np.full(max(n, 1), LV_PLAN_UNREACHED, np.uint32)
        cell = np.full(max(n, 1), -1, np.int32)
        self._check(self.lib.lv_occ_frontier_rank(self.h, int(reach), p.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  cell.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(n)))
        return p[:n], cell[:n]

    def occ_frontier_clear(self):
        self._check(self.lib.lv_occ_frontier_clear(self.h))

    # --- ray casting (include/limovelo_hip.h "Ray casting")
    def occ_raycast(self, frm, to, params: RayParams | None = None) -> np.ndarray:
        """lv_occ_raycast of the rays frm[i] -> to[i] ([n, 3] world points each; default: stop at occupied cells only); returns a
        structured array [n] of RAY_RESULT_DTYPE."""
        p = params if params is not None else default_ray_params()
        a, sa, n = _points(np.asarray(frm, np.float32).reshape(-1, 3))
        b, sb, nb = _points(np.asarray(to, np.float32).reshape(-1, 3))
        if n != nb:
            raise ValueError("occ_raycast: as many `to` points as `from` points")
        out = np.zeros(n, RAY_RESULT_DTYPE)
        self._check(self.lib.lv_occ_raycast(self.h, C.byref(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(sa), b.ctypes.data_as(C.c_void_p),
                                            C.c_size_t(sb), C.c_size_t(n), out.ctypes.data_as(C.POINTER(RayResult))))
        return out

    # --- elevation map (include/limovelo_hip.h "Elevation map")
    def elev_build(self, params: ElevationParams | None = None, points=None) -> np.ndarray:
        """lv_elev_build from points [n, 3] (None: the living points of the device map); returns stats [4] uint64: points used,
        overhang points, known cells, lethal cells."""
        p = params if params is not None else default_elevation_params()
        stats = np.zeros(4, np.uint64)
        if points is None:
            a, stride, n = None, 0, 0
        else:
            a, stride, n = _points(np.asarray(points, np.float32).reshape(-1, 3))
            if n == 0:   # (no points, but still "caller points": a pointer that is not NULL)
                a, stride = np.zeros((1, 3), np.float32), 12
        self._check(self.lib.lv_elev_build(self.h, C.byref(p), None if a is None else C.c_void_p(a.ctypes.data), C.c_size_t(stride), C.c_size_t(n),
                                           stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def elev_info(self) -> ElevationInfo:
        out = ElevationInfo()
        self._check(self.lib.lv_elev_info(self.h, C.byref(out)))
        return out

    def elev_fetch(self, layer: int) -> np.ndarray:
        """[ny, nx] of the layer's type (ELEV_LAYERS): lv_elev_fetch."""
        i = self.elev_info()
        dtype = ELEV_LAYERS[layer][1] if 0 <= int(layer) < len(ELEV_LAYERS) else np.int32
        out = np.zeros((i.ny, i.nx) if i.built else (1, 1), dtype)
        self._check(self.lib.lv_elev_fetch(self.h, int(layer), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)))
        return out

    def elev_query(self, pts):
        """(height [n] f32 metres, cls [n] int8) of the cell each world point's x, y fall in; NaN and -1 outside the grid."""
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3))
        h = np.full(n, np.nan, np.float32)
        k = np.full(n, -1, np.int8)
        self._check(self.lib.lv_elev_query(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                           h.ctypes.data_as(C.POINTER(C.c_float)), k.ctypes.data_as(C.POINTER(C.c_int8))))
        return h, k

    def elev_clear(self):
        self._check(self.lib.lv_elev_clear(self.h))

    def occ_distance_build_cells(self, cells, params: DistanceParams | None = None) -> np.ndarray:
        """lv_occ_distance_build_cells over cells (int8, [ny, nx] of the occupancy grid: 100 an obstacle, negative unknown); default
        parameters: planar = 1.  Returns lv_occ_distance_build's stats."""
        p = params if params is not None else default_distance_params(planar=1)
        a = np.ascontiguousarray(cells, np.int8)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_distance_build_cells(self.h, C.byref(p), a.ctypes.data_as(C.POINTER(C.c_int8)), C.c_size_t(a.size),
                                                         stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    # --- rollouts (include/limovelo_hip.h "Rollouts")
    def occ_rollout(self, start, controls, params: RolloutParams | None = None, footprint=None, want=("results", "best")) -> dict:
        """lv_occ_rollout of the control sequences controls [K, Tc, 2] (v, w) from the pose start (x, y, th); params.Tc is set from
        the array.  footprint: [n_fp, 2] body-frame points or None.  want: which of "results" ([K] ROLLOUT_RESULT_DTYPE), "poses"
        ([K, T + 1, 3] f32), "score" ([K] uint64) and "best" ([2] int64: index, score; -1, -1 if none) to fetch; returns them in a
        dict."""
        src = params if params is not None else default_rollout_params()
        p = RolloutParams.from_buffer_copy(src)
        u = np.ascontiguousarray(controls, np.float32)
        if u.ndim != 3 or u.shape[2] != 2:
            raise ValueError("occ_rollout: controls [K, Tc, 2]")
        K = u.shape[0]
        if K:
            p.Tc = u.shape[1]
        s0 = np.ascontiguousarray(start, np.float32).reshape(3)
        fp = np.zeros((0, 2), np.float32) if footprint is None else np.ascontiguousarray(footprint, np.float32).reshape(-1, 2)
        out = {}
        if "results" in want:
            out["results"] = np.zeros(K, ROLLOUT_RESULT_DTYPE)
        if "poses" in want:
            out["poses"] = np.zeros((K, p.T + 1, 3), np.float32)
        if "score" in want:
            out["score"] = np.zeros(K, np.uint64)
        if "best" in want:
            out["best"] = np.zeros(2, np.int64)

        def ptr(name, t):
            return out[name].ctypes.data_as(C.POINTER(t)) if name in out else None

        fptr = C.POINTER(C.c_float)
        self._check(self.lib.lv_occ_rollout(self.h, C.byref(p), s0.ctypes.data_as(fptr), u.ctypes.data_as(fptr) if K else None, C.c_size_t(K),
                                            fp.ctypes.data_as(fptr) if len(fp) else None, C.c_size_t(len(fp)), ptr("results", RolloutResult),
                                            ptr("poses", C.c_float), ptr("score", C.c_uint64), ptr("best", C.c_int64)))
        return out

    # --- localisation (include/limovelo_hip.h "Localisation")
    def occ_mcl_weigh(self, poses, beams, table, params: MclParams | None = None, want=("score", "n_in", "best")) -> dict:
        """lv_occ_mcl_weigh of the poses [K, 4] (x, y, z, th) under the scan end points beams [B, 3] (body frame) and the cost
        table [n_table] uint32 by squared voxel distance.  want: which of "score" ([K] uint64, MCL_NO_SCORE where not eligible),
        "n_in" ([K] uint32) and "best" ([2] int64: index, score; -1, -1 if none) to fetch; returns them in a dict."""
        p = params if params is not None else default_mcl_params()
        x = np.ascontiguousarray(poses, np.float32)
        e = np.ascontiguousarray(beams, np.float32)
        t = np.ascontiguousarray(table, np.uint32)
        if x.ndim != 2 or x.shape[1] != 4:
            raise ValueError("occ_mcl_weigh: poses [K, 4]")
        if e.ndim != 2 or e.shape[1] != 3:
            raise ValueError("occ_mcl_weigh: beams [B, 3]")
        if t.ndim != 1:
            raise ValueError("occ_mcl_weigh: table [n_table]")
        K = x.shape[0]
        out = {}
        if "score" in want:
            out["score"] = np.zeros(K, np.uint64)
        if "n_in" in want:
            out["n_in"] = np.zeros(K, np.uint32)
        if "best" in want:
            out["best"] = np.zeros(2, np.int64)

        def ptr(name, ct):
            return out[name].ctypes.data_as(C.POINTER(ct)) if name in out else None

        fptr = C.POINTER(C.c_float)
        self._check(self.lib.lv_occ_mcl_weigh(self.h, C.byref(p), x.ctypes.data_as(fptr) if K else None, C.c_size_t(K),
                                              e.ctypes.data_as(fptr) if len(e) else None, C.c_size_t(len(e)),
                                              t.ctypes.data_as(C.POINTER(C.c_uint32)) if len(t) else None, C.c_size_t(len(t)),
                                              ptr("score", C.c_uint64), ptr("n_in", C.c_uint32), ptr("best", C.c_int64)))
        return out

    # --- resident localisation filter (include/limovelo_hip.h "Resident localisation filter")
    def occ_mcl_filter_set(self, poses, seed: int = 0) -> None:
        """lv_occ_mcl_filter_set: the particles [K, 4] (x, y, z, th) go to the device; acc, n_in and the epoch are 0."""
        x = np.ascontiguousarray(poses, np.float32)
        if x.ndim != 2 or x.shape[1] != 4:
            raise ValueError("occ_mcl_filter_set: poses [K, 4]")
        self._check(self.lib.lv_occ_mcl_filter_set(self.h, x.ctypes.data_as(C.POINTER(C.c_float)) if len(x) else None, C.c_size_t(len(x)),
                                                   C.c_uint64(int(seed))))

    def occ_mcl_filter_move(self, delta, sigma) -> None:
        """lv_occ_mcl_filter_move by delta = (rot1, trans, rot2) with the standard deviations sigma (mcl.motion_sigmas)."""
        d = np.ascontiguousarray(delta, np.float32).reshape(3)
        s = np.ascontiguousarray(sigma, np.float32).reshape(3)
        fptr = C.POINTER(C.c_float)
        self._check(self.lib.lv_occ_mcl_filter_move(self.h, d.ctypes.data_as(fptr), s.ctypes.data_as(fptr)))

    def occ_mcl_filter_weigh(self, beams, table, params: MclParams | None = None, want_best: bool = True):
        """lv_occ_mcl_filter_weigh of the resident particles under the beams [B, 3] and the cost table: best [2] int64 (index, score;
        -1, -1 if none) of this scan, or None when it is not asked for (the call then does not wait for the device)."""
        p = params if params is not None else default_mcl_params()
        e = np.ascontiguousarray(beams, np.float32)
        t = np.ascontiguousarray(table, np.uint32)
        if e.ndim != 2 or e.shape[1] != 3:
            raise ValueError("occ_mcl_filter_weigh: beams [B, 3]")
        if t.ndim != 1:
            raise ValueError("occ_mcl_filter_weigh: table [n_table]")
        best = np.zeros(2, np.int64) if want_best else None
        self._check(self.lib.lv_occ_mcl_filter_weigh(self.h, C.byref(p), e.ctypes.data_as(C.POINTER(C.c_float)) if len(e) else None, C.c_size_t(len(e)),
                                                     t.ctypes.data_as(C.POINTER(C.c_uint32)) if len(t) else None, C.c_size_t(len(t)),
                                                     best.ctypes.data_as(C.POINTER(C.c_int64)) if want_best else None))
        return best

    def occ_mcl_filter_resample(self, wtable, params: MclResampleParams | None = None, want_ancestors: bool = False):
        """lv_occ_mcl_filter_resample with the weight table [n_w] uint32: (MclFilterStats, ancestors [K] uint32 or None: asked for
        and resampled)."""
        p = params if params is not None else default_mcl_resample_params()
        t = np.ascontiguousarray(wtable, np.uint32)
        if t.ndim != 1:
            raise ValueError("occ_mcl_filter_resample: wtable [n_w]")
        stats = MclFilterStats()
        anc = np.zeros(int(self.occ_mcl_filter_info().K), np.uint32) if want_ancestors else None
        self._check(self.lib.lv_occ_mcl_filter_resample(self.h, C.byref(p), t.ctypes.data_as(C.POINTER(C.c_uint32)) if len(t) else None,
                                                        C.c_size_t(len(t)), C.byref(stats),
                                                        anc.ctypes.data_as(C.POINTER(C.c_uint32)) if anc is not None and len(anc) else None))
        return stats, (anc if anc is not None and stats.resampled else None)

    def occ_mcl_filter_get(self, want=("poses", "acc", "n_in")) -> dict:
        """lv_occ_mcl_filter_get: those of poses [K, 4] f32, acc [K] uint64 and n_in [K] uint32 that `want` names."""
        K = int(self.occ_mcl_filter_info().K)
        out = {}
        if "poses" in want:
            out["poses"] = np.zeros((K, 4), np.float32)
        if "acc" in want:
            out["acc"] = np.zeros(K, np.uint64)
        if "n_in" in want:
            out["n_in"] = np.zeros(K, np.uint32)

        def ptr(name, ct):
            return out[name].ctypes.data_as(C.POINTER(ct)) if name in out else None

        self._check(self.lib.lv_occ_mcl_filter_get(self.h, ptr("poses", C.c_float), ptr("acc", C.c_uint64), ptr("n_in", C.c_uint32), C.c_size_t(max(K, 1))))
        return out

    def occ_mcl_filter_info(self) -> MclFilterInfo:
        info = MclFilterInfo()
        self._check(self.lib.lv_occ_mcl_filter_info(self.h, C.byref(info)))
        return info

    def occ_mcl_filter_clear(self) -> None:
        self._check(self.lib.lv_occ_mcl_filter_clear(self.h))

    def occ_view_gain(self, views) -> np.ndarray:
        """lv_occ_view_gain over views = [(R [3, 3], t [3], pattern end points [n, 3] sensor frame)] (1..32 of them); returns
        [n_views, 4] uint64: rays used, rays stopped, distinct unknown cells seen, distinct free cells seen."""
        arr, keep = view_array(views)
        gain = np.zeros((len(views), 4), np.uint64)
        self._check(self.lib.lv_occ_view_gain(self.h, arr, C.c_size_t(len(views)), gain.ctypes.data_as(C.POINTER(C.c_uint64))))
        return gain

    # --- TSDF and mesh (include/limovelo_hip.h "TSDF and mesh")
    def tsdf_configure(self, params: TsdfParams | None = None):
        """lv_tsdf_configure: allocates the volume (default: lv_default_tsdf_params), every voxel unobserved."""
        p = params if params is not None else default_tsdf_params()
        self._check(self.lib.lv_tsdf_configure(self.h, C.byref(p)))

    def tsdf_params(self) -> TsdfParams:
        p = TsdfParams()
        self._check(self.lib.lv_tsdf_get_params(self.h, C.byref(p)))
        return p

    def tsdf_integrate(self, views) -> np.ndarray:
        """lv_tsdf_integrate over views = [(R [3, 3], t [3], points [n, 3] sensor frame)] (1..32 of them, one call); returns stats
        [4] uint64: rays used, rays cut, contributions, voxels touched."""
        arr, keep = view_array(views)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_tsdf_integrate(self.h, arr, C.c_size_t(len(views)), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def tsdf_query(self, pts):
        """(metres [n] f32, weight [n] int32) of the voxel each world point falls in; NaN and 0 outside the grid."""
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3))
        m = np.full(n, np.nan, np.float32)
        w = np.zeros(n, np.int32)
        self._check(self.lib.lv_tsdf_query(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                           m.ctypes.data_as(C.POINTER(C.c_float)), w.ctypes.data_as(C.POINTER(C.c_int32))))
        return m, w

    def tsdf_fetch(self, S=True, W=True, metres=False) -> dict:
        """dict of the wanted arrays, [nz, ny, nx] each: S and W int32, metres f32 (NaN where W = 0)."""
        p = self.tsdf_params()
        shape = (p.nz, p.ny, p.nx)
        out = {}
        if S:
            out["S"] = np.zeros(shape, np.int32)
        if W:
            out["W"] = np.zeros(shape, np.int32)
        if metres:
            out["metres"] = np.zeros(shape, np.float32)

        def ptr(name, ct):
            return out[name].ctypes.data_as(C.POINTER(ct)) if name in out else None

        self._check(self.lib.lv_tsdf_fetch(self.h, ptr("S", C.c_int32), ptr("W", C.c_int32), ptr("metres", C.c_float),
                                           C.c_size_t(p.nx * p.ny * p.nz)))
        return out

    def tsdf_load(self, S, W):
        a = np.ascontiguousarray(S, np.int32)
        b = np.ascontiguousarray(W, np.int32)
        if a.size != b.size:
            raise ValueError("tsdf_load: S and W of one size")
        self._check(self.lib.lv_tsdf_load(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(a.size)))

    def tsdf_clear(self):
        self._check(self.lib.lv_tsdf_clear(self.h))

    def tsdf_mesh_build(self, min_weight: int = 1) -> np.ndarray:
        """lv_tsdf_mesh_build; returns counts [4] uint64: vertices, triangles, active cells, edges refused for a missing cell."""
        counts = np.zeros(4, np.uint64)
        self._check(self.lib.lv_tsdf_mesh_build(self.h, int(min_weight), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        return counts

    def tsdf_mesh_info(self) -> MeshInfo:
        out = MeshInfo()
        self._check(self.lib.lv_tsdf_mesh_info(self.h, C.byref(out)))
        return out

    def tsdf_mesh_fetch(self, xyz=True, sub=True, tri=True) -> dict:
        """dict of the wanted arrays of the mesh last built: xyz [V, 3] f32 metres, sub [V, 3] int32 sub-units, tri [F, 3] uint32."""
        i = self.tsdf_mesh_info()
        if not i.built:
            raise LvError("limovelo_hip error -4: no mesh: call lv_tsdf_mesh_build first")   # (LV_ESTATE, as the library answers)
        nv, nt = int(i.vertices), int(i.triangles)
        out = {}
        if xyz:
            out["xyz"] = np.zeros((nv, 3), np.float32)
        if sub:
            out["sub"] = np.zeros((nv, 3), np.int32)
        if tri:
            out["tri"] = np.zeros((nt, 3), np.uint32)

        def ptr(name, ct):
            return out[name].ctypes.data_as(C.POINTER(ct)) if name in out else None

        self._check(self.lib.lv_tsdf_mesh_fetch(self.h, ptr("xyz", C.c_float), ptr("sub", C.c_int32), ptr("tri", C.c_uint32), C.c_size_t(nv),
                                                C.c_size_t(nt)))
        return out

    def tsdf_mesh_clear(self):
        self._check(self.lib.lv_tsdf_mesh_clear(self.h))

    # --- depth fusion (include/limovelo_hip.h "Depth fusion")
    def tsdf_integrate_depth(self, frames, params: DepthParams | None = None) -> np.ndarray:
        """lv_depth_integrate over frames = [frame dict (depth_view)] (1..32, one call); returns stats [4] uint64: (voxel, view) pairs
        projected, those with a valid depth, contributions, voxels touched."""
        p = params if params is not None else default_depth_params()
        arr = (DepthView * max(len(frames), 1))()
        keep = []
        for i, f in enumerate(frames):
            arr[i], img = depth_view(f)
            keep.append(img)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_depth_integrate(self.h, arr, C.c_size_t(len(frames)), C.byref(p), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    # --- colour layer (include/limovelo_hip.h "Colour layer")
    def colour_integrate(self, views, params: ColourParams | None = None) -> np.ndarray:
        """lv_colour_integrate over views = [frame dict (camera_view)] (1..32, one call); returns stats [4] uint64: candidates,
        (voxel, view) pairs projected, pairs seen, voxels coloured by the call."""
        p = params if params is not None else default_colour_params()
        arr = (LvCameraView * max(len(views), 1))()
        keep = []
        for i, f in enumerate(views):
            arr[i], img = camera_view(f)
            keep.append(img)
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_colour_integrate(self.h, arr, C.c_size_t(len(views)), C.byref(p), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def colour_fetch(self, sums=True, rgba=False) -> dict:
        """dict of the wanted arrays: sums [nz, ny, nx, 4] uint32 (C[0..2], Wc), rgba [nz, ny, nx, 4] uint8 (the voxel colours)."""
        p = self.tsdf_params()
        out = {}
        if sums:
            out["sums"] = np.zeros((p.nz, p.ny, p.nx, 4), np.uint32)
        if rgba:
            out["rgba"] = np.zeros((p.nz, p.ny, p.nx, 4), np.uint8)
        self._check(self.lib.lv_colour_fetch(self.h, out["sums"].ctypes.data_as(C.POINTER(C.c_uint32)) if sums else None,
                                             out["rgba"].ctypes.data_as(C.POINTER(C.c_uint8)) if rgba else None, C.c_size_t(p.nx * p.ny * p.nz)))
        return out

    def colour_load(self, sums):
        a = np.ascontiguousarray(sums, np.uint32)
        if a.size % 4:
            raise ValueError("colour_load: four values per voxel")
        self._check(self.lib.lv_colour_load(self.h, a.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(a.size // 4)))

    def colour_query(self, pts) -> np.ndarray:
        """rgba [n, 4] uint8 of the voxel each world point falls in; 0, 0, 0, 0 outside the grid and where never coloured."""
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3))
        out = np.zeros((n, 4), np.uint8)
        self._check(self.lib.lv_colour_query(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n),
                                             out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def colour_clear(self):
        self._check(self.lib.lv_colour_clear(self.h))

    def colour_info(self) -> ColourInfo:
        out = ColourInfo()
        self._check(self.lib.lv_colour_info(self.h, C.byref(out)))
        return out

    def mesh_colours(self) -> np.ndarray:
        """rgba [V, 4] uint8 of the mesh last built, in vertex order (LvError where it carries none)."""
        i = self.tsdf_mesh_info()
        nv = int(i.vertices) if i.built else 0
        out = np.zeros((max(nv, 1), 4), np.uint8)
        self._check(self.lib.lv_mesh_colours(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(nv)))
        return out[:nv]

    # --- surface ray casting (include/limovelo_hip.h "Surface ray casting")
    def tsdf_raycast(self, frm, to, params: TsdfRayParams | None = None, normals=False, colours=False):
        """lv_surf_raycast of the rays frm[i] -> to[i] ([n, 3] world points each; default min_weight 1); returns (results [n] of
        TSDF_RAY_RESULT_DTYPE, normals [n, 3] f32 or None, rgba [n, 4] uint8 or None)."""
        p = params if params is not None else default_tsdf_ray_params()
        a, sa, n = _points(np.asarray(frm, np.float32).reshape(-1, 3))
        b, sb, nb = _points(np.asarray(to, np.float32).reshape(-1, 3))
        if n != nb:
            raise ValueError("tsdf_raycast: as many `to` points as `from` points")
        out = np.zeros(n, TSDF_RAY_RESULT_DTYPE)
        nrm = np.zeros((n, 3), np.float32) if normals else None
        col = np.zeros((n, 4), np.uint8) if colours else None
        self._check(self.lib.lv_surf_raycast(self.h, C.byref(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(sa), b.ctypes.data_as(C.c_void_p),
                                             C.c_size_t(sb), C.c_size_t(n), out.ctypes.data_as(C.POINTER(TsdfRayResult)),
                                             nrm.ctypes.data_as(C.POINTER(C.c_float)) if normals else None,
                                             col.ctypes.data_as(C.POINTER(C.c_uint8)) if colours else None))
        return out, nrm, col

    def tsdf_raycast_views(self, views, params: TsdfRayParams | None = None, normals=False, colours=False):
        """lv_surf_raycast_views over views = [(R [3, 3], t [3], pattern end points [n, 3] sensor frame)] (1..32); returns (results,
        normals or None, rgba or None over every return of every view in order, stats [4] uint64: rays used, HIT, BLOCKED, CLEAR)."""
        p = params if params is not None else default_tsdf_ray_params()
        arr, keep = view_array(views)
        n = sum(int(arr[i].n) for i in range(len(views)))
        out = np.zeros(max(n, 1), TSDF_RAY_RESULT_DTYPE)
        nrm = np.zeros((max(n, 1), 3), np.float32) if normals else None
        col = np.zeros((max(n, 1), 4), np.uint8) if colours else None
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_surf_raycast_views(self.h, C.byref(p), arr, C.c_size_t(len(views)), out.ctypes.data_as(C.POINTER(TsdfRayResult)),
                                                   nrm.ctypes.data_as(C.POINTER(C.c_float)) if normals else None,
                                                   col.ctypes.data_as(C.POINTER(C.c_uint8)) if colours else None, C.c_size_t(n),
                                                   stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:n], (nrm[:n] if normals else None), (col[:n] if colours else None), stats

    # --- rolling volumes (include/limovelo_hip.h "Rolling volumes")
    def volume_recentre(self, volume: int, shift) -> np.ndarray:
        """lv_volume_recentre of LV_VOLUME_OCC or LV_VOLUME_SURFACE by shift (3 whole voxels); returns stats [4] uint64: voxels kept,
        exposed, that held evidence and left the volume, 0."""
        d = (C.c_int32 * 3)(*[int(v) for v in shift])
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_volume_recentre(self.h, int(volume), d, stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def volume_shift_info(self) -> VolumeShifts:
        out = VolumeShifts()
        self._check(self.lib.lv_volume_shift_info(self.h, C.byref(out)))
        return out

    def occ_mark(self, params: OccMarkParams | None = None, points=None) -> np.ndarray:
        """lv_occ_mark from points [n, 3] (None: the living points of the device map); returns stats [4] uint64: points used,
        voxels holding >= min_points, voxels marked, voxels left alone because they were observed."""
        p = params if params is not None else default_occ_mark_params()
        stats = np.zeros(4, np.uint64)
        if points is None:
            a, stride, n = None, 0, 0
        else:
            a, stride, n = _points(np.asarray(points, np.float32).reshape(-1, 3))
            if n == 0:   # (no points, but still "caller points": a pointer that is not NULL)
                a, stride = np.zeros((1, 3), np.float32), 12
        self._check(self.lib.lv_occ_mark(self.h, C.byref(p), None if a is None else C.c_void_p(a.ctypes.data), C.c_size_t(stride), C.c_size_t(n),
                                         stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def occ_from_surface(self, params: OccSurfaceParams | None = None) -> np.ndarray:
        """lv_occ_from_surface ("Occupancy from the surface"): the occupancy grid's box filled from the TSDF volume; returns stats
        [4] uint64: voxels classed OCCUPIED, classed FREE, voxels whose bits changed, voxels outside the volume."""
        p = params if params is not None else default_occ_surface_params()
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_occ_from_surface(self.h, C.byref(p), stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    # --- place recognition (include/limovelo_hip.h "Place recognition")
    def place_configure(self, params: PlaceParams | None = None):
        """lv_place_configure: sets the parameters (default: lv_default_place_params) and clears the database."""
        p = params if params is not None else default_place_params()
        self._check(self.lib.lv_place_configure(self.h, C.byref(p)))
        self._place_prm = p

    def place_params(self) -> PlaceParams:
        """The parameters of the last place_configure (the defaults before one)."""
        return getattr(self, "_place_prm", None) or default_place_params()

    def _place_bins(self):
        p = self.place_params()
        return int(p.n_rings), int(p.n_sectors)

    def place_describe(self, state) -> np.ndarray:
        """[n_rings, n_sectors] f32: the descriptor of the current scan at state (26 f64), not stored."""
        r, s = self._place_bins()
        x = np.ascontiguousarray(state, np.float64)
        out = np.zeros((r, s), np.float32)
        self._check(self.lib.lv_place_describe(self.h, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def place_add_scan(self, state) -> int:
        x = np.ascontiguousarray(state, np.float64)
        i = C.c_uint32(0)
        self._check(self.lib.lv_place_add_scan(self.h, x.ctypes.data_as(C.c_void_p), C.byref(i)))
        return int(i.value)

    def place_add_map(self, centres) -> int:
        """Places built from the device map at centres [n, 3] (f64); returns the first id."""
        c = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1, 3))
        i = C.c_uint32(0)
        self._check(self.lib.lv_place_add_map(self.h, c.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(len(c)), C.byref(i)))
        return int(i.value)

    def place_query(self, state, k: int):
        """(ids [n] uint32, shifts [n] int32, dist [n] f32) of the k places nearest to the current scan at state, n = min(k, count)."""
        x = np.ascontiguousarray(state, np.float64)
        ids = np.zeros(max(int(k), 1), np.uint32)
        sh = np.zeros(max(int(k), 1), np.int32)
        d = np.zeros(max(int(k), 1), np.float32)
        n = C.c_size_t(0)
        self._check(self.lib.lv_place_query(self.h, x.ctypes.data_as(C.c_void_p), int(k), ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            sh.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        m = int(n.value)
        return ids[:m].copy(), sh[:m].copy(), d[:m].copy()

    def place_count(self) -> int:
        return int(self.lib.lv_place_count(self.h))

    def place_clear(self):
        self._check(self.lib.lv_place_clear(self.h))

    def place_fetch(self):
        """(desc [n, n_rings, n_sectors] f32, centres [n, 3] f64) of every place, in id order."""
        r, s = self._place_bins()
        n = self.place_count()
        desc = np.zeros((n, r, s), np.float32)
        cen = np.zeros((n, 3), np.float64)
        self._check(self.lib.lv_place_fetch(self.h, desc.ctypes.data_as(C.POINTER(C.c_float)), cen.ctypes.data_as(C.POINTER(C.c_double)),
                                            C.c_size_t(n)))
        return desc, cen

    def place_centres(self) -> np.ndarray:
        """[n, 3] f64: every place's centre, in id order (lv_place_fetch without the descriptors)."""
        n = self.place_count()
        cen = np.zeros((n, 3), np.float64)
        self._check(self.lib.lv_place_fetch(self.h, None, cen.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(n)))
        return cen

    def place_load(self, desc, centres):
        """Appends places: desc [n, n_rings, n_sectors] (or [n, n_rings * n_sectors]) f32, centres [n, 3] f64."""
        c = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(desc, np.float32).reshape(len(c), -1))
        self._check(self.lib.lv_place_load(self.h, d.ctypes.data_as(C.POINTER(C.c_float)), c.ctypes.data_as(C.POINTER(C.c_double)),
                                           C.c_size_t(len(c))))

    # --- pose graph (include/limovelo_hip.h "Pose graph")
    def graph_set(self, poses, fixed=None, edges=None, priors=None):
        """lv_graph_set: poses [n, 7] f64 (t, q = x y z w), fixed [n] bool or None, edges GRAPH_EDGE_DTYPE, priors GRAPH_PRIOR_DTYPE."""
        x = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 7))
        f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, bool).astype(np.uint8))
        e = np.ascontiguousarray(np.zeros(0, GRAPH_EDGE_DTYPE) if edges is None else np.asarray(edges, GRAPH_EDGE_DTYPE).reshape(-1))
        p = np.ascontiguousarray(np.zeros(0, GRAPH_PRIOR_DTYPE) if priors is None else np.asarray(priors, GRAPH_PRIOR_DTYPE).reshape(-1))
        self._check(self.lib.lv_graph_set(self.h, x.ctypes.data_as(C.POINTER(GraphPose)), C.c_size_t(len(x)),
                                          None if f is None else f.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          e.ctypes.data_as(C.POINTER(GraphEdge)) if len(e) else None, C.c_size_t(len(e)),
                                          p.ctypes.data_as(C.POINTER(GraphPrior)) if len(p) else None, C.c_size_t(len(p))))

    def graph_optimise(self, params: GraphParams | None = None, **kw) -> dict:
        """lv_graph_optimise with the given parameters (default: lv_default_graph_params changed by kw); the info record as a dict."""
        p = params if params is not None else default_graph_params(**kw)
        info = GraphInfo()
        self._check(self.lib.lv_graph_optimise(self.h, C.byref(p), C.byref(info)))
        return info.as_dict()

    def graph_info(self) -> dict:
        info = GraphInfo()
        self._check(self.lib.lv_graph_get_info(self.h, C.byref(info)))
        return info.as_dict()

    def graph_fetch(self) -> np.ndarray:
        """[n, 7] f64: the current poses."""
        out = np.zeros((self.graph_info()["n"], 7))
        self._check(self.lib.lv_graph_fetch(self.h, out.ctypes.data_as(C.POINTER(GraphPose)), C.c_size_t(len(out))))
        return out

    def graph_chi2(self):
        """(edge_s [n_edges], prior_s [n_priors]) f64: r^T info r of every factor at the current poses."""
        i = self.graph_info()
        es, ps = np.zeros(i["n_edges"]), np.zeros(i["n_priors"])
        self._check(self.lib.lv_graph_chi2(self.h, es.ctypes.data_as(C.POINTER(C.c_double)), ps.ctypes.data_as(C.POINTER(C.c_double))))
        return es, ps

    def graph_warp_points(self, pts, keys) -> np.ndarray:
        """[n, 3] f32: pts moved by the correction of their key's node (lv_graph_warp_points)."""
        a, stride, n = _points(pts)
        k = np.ascontiguousarray(keys, np.uint32)
        if len(k) != n:
            raise ValueError("one key per point")
        out = np.zeros((n, 3), np.float32)
        self._check(self.lib.lv_graph_warp_points(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), k.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  C.c_size_t(n), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def graph_clear(self):
        self._check(self.lib.lv_graph_clear(self.h))

    # --- trajectory (include/limovelo_hip.h "Trajectory"; limo_velo_amd.offline has the helpers)
    @staticmethod
    def _traj_knots(knots):
        k = np.ascontiguousarray(np.asarray(knots, TRAJ_KNOT_DTYPE).reshape(-1))
        return k, k.ctypes.data_as(C.POINTER(TrajKnot))

    def traj_set(self, knots):
        """lv_traj_set: knots as TRAJ_KNOT_DTYPE records (capi.traj_knots builds them from times and poses)."""
        k, p = self._traj_knots(knots)
        self._check(self.lib.lv_traj_set(self.h, p, C.c_size_t(len(k))))

    def traj_info(self) -> dict:
        info = TrajInfo()
        self._check(self.lib.lv_traj_get_info(self.h, C.byref(info)))
        return info.as_dict()

    def traj_fetch(self) -> np.ndarray:
        """The current knots (TRAJ_KNOT_DTYPE)."""
        out = np.zeros(max(self.traj_info()["n"], 1), TRAJ_KNOT_DTYPE)
        self._check(self.lib.lv_traj_fetch(self.h, out.ctypes.data_as(C.POINTER(TrajKnot)), C.c_size_t(len(out))))
        return out[:self.traj_info()["n"]]

    def traj_clear(self):
        self._check(self.lib.lv_traj_clear(self.h))

    def traj_sample(self, times, extrapolate=TRAJ_CLAMP):
        """(poses [n, 7] f64, status [n] u8) of the trajectory at times [n] f64."""
        t = np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1))
        out, st = np.zeros((len(t), 7)), np.zeros(len(t), np.uint8)
        self._check(self.lib.lv_traj_sample(self.h, t.ctypes.data_as(C.POINTER(C.c_double)), C.c_size_t(len(t)), int(extrapolate),
                                            out.ctypes.data_as(C.POINTER(GraphPose)), st.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out, st

    def traj_smooth(self, params: TrajSmoothParams | None = None, fixed=None, **kw):
        """lv_traj_smooth with the given parameters (default: lv_default_traj_smooth_params changed by kw); fixed [n] bool or None."""
        p = params if params is not None else default_traj_smooth_params(**kw)
        f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, bool).astype(np.uint8))
        if f is not None and len(f) != self.traj_info()["n"]:
            raise ValueError("one flag per knot")
        self._check(self.lib.lv_traj_smooth(self.h, C.byref(p), None if f is None else f.ctypes.data_as(C.POINTER(C.c_uint8))))

    def traj_correct(self, corrections):
        """lv_traj_correct: corrections D_k at keyframe times as TRAJ_KNOT_DTYPE records (offline.corrections builds them)."""
        k, p = self._traj_knots(corrections)
        self._check(self.lib.lv_traj_correct(self.h, p, C.c_size_t(len(k))))

    def traj_register(self, points, params: TrajRegisterParams | None = None, time_offset=None, want_points=True, want_status=True):
        """lv_traj_register.  points: a structured array with x, y, z f32 at offset 0 and an f64 field "time" (POINT_DTYPE, what
        cloud_fetch returns), or (bytes-like, stride, time_offset, n).  Returns (out [n, 3] f32 or None, status [n] u8 or None,
        stats [4])."""
        if isinstance(points, tuple):
            raw, stride, toff, n = points
            buf = np.frombuffer(raw, np.uint8)
        else:
            a = np.ascontiguousarray(points)
            stride, n = a.dtype.itemsize, len(a)
            toff = a.dtype.fields["time"][1] if time_offset is None else int(time_offset)
            buf = a.view(np.uint8).reshape(-1)
        p = params if params is not None else default_traj_register_params()
        out = np.zeros((n, 3), np.float32) if want_points else None
        st = np.zeros(n, np.uint8) if want_status else None
        stats = (C.c_uint64 * 4)()
        self._check(self.lib.lv_traj_register(self.h, C.byref(p), buf.ctypes.data_as(C.c_void_p) if n else None, C.c_size_t(stride),
                                              C.c_size_t(toff), C.c_size_t(n),
                                              out.ctypes.data_as(C.POINTER(C.c_float)) if want_points else None,
                                              st.ctypes.data_as(C.POINTER(C.c_uint8)) if want_status else None, stats))
        return out, st, [int(v) for v in stats]

    def traj_register_cloud(self, t1: float, t2: float, params: TrajRegisterParams | None = None):
        """lv_traj_register_cloud over the device LiDAR buffer's window [t1, t2]: (out [n, 3] f32, status [n] u8, stats [4])."""
        p = params if params is not None else default_traj_register_params()
        n = C.c_size_t(0)
        stats = (C.c_uint64 * 4)()
        self._check(self.lib.lv_traj_register_cloud(self.h, C.byref(p), C.c_double(t1), C.c_double(t2), None, None, C.c_size_t(0), C.byref(n), stats))
        cnt = int(n.value)
        out, st = np.zeros((max(cnt, 1), 3), np.float32), np.zeros(max(cnt, 1), np.uint8)
        self._check(self.lib.lv_traj_register_cloud(self.h, C.byref(p), C.c_double(t1), C.c_double(t2), out.ctypes.data_as(C.POINTER(C.c_float)),
                                                    st.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(len(st)), C.byref(n), stats))
        return out[:n.value], st[:n.value], [int(v) for v in stats]

    # --- NDT registration (include/limovelo_hip.h "NDT registration"; limo_velo_amd.ndt has the helpers)
    def _ndt_points(self, points):
        if points is None:
            return None, 0, 0
        a, stride, n = _points(np.asarray(points, np.float32).reshape(-1, 3))
        if n == 0:   # (no points, but still "caller points": a pointer that is not NULL)
            a, stride = np.zeros((1, 3), np.float32), 12
        return a, stride, n

    def ndt_build(self, params: NdtParams | None = None, points=None) -> np.ndarray:
        """lv_ndt_build from points [n, 3] (None: the living points of the device map); stats [4] uint64: points used, points
        ignored, used voxels, occupied voxels below min_points."""
        p = params if params is not None else default_ndt_params()
        stats = np.zeros(4, np.uint64)
        a, stride, n = self._ndt_points(points)
        self._check(self.lib.lv_ndt_build(self.h, C.byref(p), None if a is None else C.c_void_p(a.ctypes.data), C.c_size_t(stride), C.c_size_t(n),
                                          stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def ndt_add(self, points=None) -> np.ndarray:
        """lv_ndt_add: further points into the target; stats as ndt_build (the points of this call, the voxels of the whole)."""
        stats = np.zeros(4, np.uint64)
        a, stride, n = self._ndt_points(points)
        self._check(self.lib.lv_ndt_add(self.h, None if a is None else C.c_void_p(a.ctypes.data), C.c_size_t(stride), C.c_size_t(n),
                                        stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def ndt_info(self) -> NdtTargetInfo:
        out = NdtTargetInfo()
        self._check(self.lib.lv_ndt_info(self.h, C.byref(out)))
        return out

    def ndt_fetch(self, layer: int) -> np.ndarray:
        """[nz, ny, nx] (COUNT) or [nz, ny, nx, 3 or 6] of the layer's type (NDT_LAYERS): lv_ndt_fetch."""
        i = self.ndt_info()
        _, dtype, width = NDT_LAYERS[layer] if 0 <= int(layer) < len(NDT_LAYERS) else ("", np.int64, 1)
        shape = (i.params.nz, i.params.ny, i.params.nx) if i.built else (1, 1, 1)
        out = np.zeros(shape + ((width,) if width > 1 else ()), dtype)
        self._check(self.lib.lv_ndt_fetch(self.h, int(layer), out.ctypes.data_as(C.c_void_p), C.c_size_t(int(np.prod(shape)))))
        return out

    def ndt_align(self, source, guesses, params: NdtAlignParams | None = None, **kw):
        """lv_ndt_align of source [n, 3] from guesses [K, 7] f64 (t, q = x y z w): (results, best) with results an array of
        NDT_RESULT_DTYPE [K] and best = (index, n_in) or (-1, -1)."""
        p = params if params is not None else default_ndt_align_params(**kw)
        a, stride, n = _points(np.asarray(source, np.float32).reshape(-1, 3))
        g = np.ascontiguousarray(np.asarray(guesses, np.float64).reshape(-1, 7))
        res = np.zeros(len(g), NDT_RESULT_DTYPE)
        best = np.zeros(2, np.int32)
        self._check(self.lib.lv_ndt_align(self.h, C.byref(p), a.ctypes.data_as(C.c_void_p) if n else None, C.c_size_t(stride), C.c_size_t(n),
                                          g.ctypes.data_as(C.POINTER(GraphPose)) if len(g) else None, C.c_size_t(len(g)),
                                          res.ctypes.data_as(C.POINTER(NdtResult)) if len(g) else None, best.ctypes.data_as(C.POINTER(C.c_int32))))
        return res, (int(best[0]), int(best[1]))

    def ndt_clear(self):
        self._check(self.lib.lv_ndt_clear(self.h))

    # --- Surface registration (include/limovelo_hip.h "Surface registration"; limo_velo_amd.mesh has the helpers)
    def surf_sample(self, pts, min_weight: int = 1):
        """lv_surf_sample at world points [n, 3]: (d [n] f64 metres, n [n, 3] f64 the gradient, status [n] uint8 of SURF_SAMPLE_*);
        d and n are zeros where the point is not KNOWN."""
        a, stride, n = _points(np.asarray(pts, np.float32).reshape(-1, 3))
        out = np.zeros((n, 4), np.float64)
        status = np.zeros(n, np.uint8)
        self._check(self.lib.lv_surf_sample(self.h, int(min_weight), a.ctypes.data_as(C.c_void_p) if n else None, C.c_size_t(stride), C.c_size_t(n),
                                            out.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out[:, 0].copy(), out[:, 1:].copy(), status

    def surf_align(self, source, guesses, params: SurfAlignParams | None = None, **kw):
        """lv_surf_align of source [n, 3] (sensor frame) from guesses [K, 7] f64 (t, q = x y z w, sensor -> world): (results, best)
        with results an array of SURF_ALIGN_RESULT_DTYPE [K] and best = (index, n_in) or (-1, -1)."""
        p = params if params is not None else default_surf_align_params(**kw)
        a, stride, n = _points(np.asarray(source, np.float32).reshape(-1, 3))
        g = np.ascontiguousarray(np.asarray(guesses, np.float64).reshape(-1, 7))
        res = np.zeros(len(g), SURF_ALIGN_RESULT_DTYPE)
        best = np.zeros(2, np.int32)
        self._check(self.lib.lv_surf_align(self.h, C.byref(p), a.ctypes.data_as(C.c_void_p) if n else None, C.c_size_t(stride), C.c_size_t(n),
                                           g.ctypes.data_as(C.POINTER(GraphPose)) if len(g) else None, C.c_size_t(len(g)),
                                           res.ctypes.data_as(C.POINTER(SurfAlignResult)) if len(g) else None,
                                           best.ctypes.data_as(C.POINTER(C.c_int32))))
        return res, (int(best[0]), int(best[1]))

    # --- Submap merging (include/limovelo_hip.h "Submap merging"; limo_velo_amd.mesh has the helpers)
    def surf_merge(self, submap: SurfSubmap, pose, params: SurfMergeParams | None = None) -> np.ndarray:
        """lv_surf_merge of a SurfSubmap (surf_submap()) at pose [7] f64 (t, q = x y z w, submap -> world); params None: the
        defaults.  Returns stats [4] uint64: voxels not OUTSIDE, voxels that contribute, the sum of dW, voxels DROPPED."""
        g = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(7))
        stats = np.zeros(4, np.uint64)
        self._check(self.lib.lv_surf_merge(self.h, C.byref(submap), g.ctypes.data_as(C.POINTER(GraphPose)),
                                           C.byref(params) if params is not None else None, stats.ctypes.data_as(C.POINTER(C.c_uint64))))
        return stats

    def scan_set(self, pts):
        a, stride, n = _points(pts)
        self._n = n
        self._check(self.lib.lv_scan_set(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n)))

    def scan_deskew(self, xyz, times, states, Xt2, downsample_prec=0.5):
        """xyz [N,3] f32, times [N] f64, states / Xt2: numpy records with the lv_motion_state layout (184 B)."""
        n = len(xyz)
        rec = np.zeros(n, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("pad", "f4"), ("time", "f8"), ("intensity", "f4"), ("range", "f4")])
        xyz = np.asarray(xyz, np.float32)
        rec["x"], rec["y"], rec["z"], rec["time"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], np.asarray(times, np.float64)
        st = np.ascontiguousarray(states)
        x2 = np.ascontiguousarray(Xt2)
        assert st.dtype.itemsize == 184 and x2.dtype.itemsize == 184
        self._check(self.lib.lv_scan_deskew(self.h, rec.ctypes.data_as(C.c_void_p), C.c_size_t(32), C.c_size_t(16), C.c_size_t(n),
                                            st.ctypes.data_as(C.c_void_p), C.c_size_t(len(st)), x2.ctypes.data_as(C.c_void_p),
                                            C.c_float(downsample_prec)))
        self._n = self.scan_size()

    def scan_downsample(self, xyz, downsample_prec=0.5):
        a, stride, n = _points(xyz)
        self._check(self.lib.lv_scan_downsample(self.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(stride), C.c_size_t(n), C.c_float(downsample_prec)))
        self._n = self.scan_size()

    # --- row f-4: LiDAR wire formats
    def cloud_format_preset(self, lidar_type: int) -> CloudFormat:
        f = CloudFormat()
        self._check(self.lib.lv_cloud_format_preset(int(lidar_type), C.byref(f)))
        return f

    def cloud_ingest(self, raw: bytes, n: int, fmt: CloudFormat, prm: IngestParams) -> int:
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)
        kept = C.c_size_t(0)
        self._check(self.lib.lv_cloud_ingest(self.h, buf, C.c_size_t(n), C.byref(fmt), C.byref(prm), C.byref(kept)))
        return int(kept.value)

    def cloud_size(self) -> int:
        return int(self.lib.lv_cloud_size(self.h))

    def cloud_fetch(self, t1: float, t2: float) -> np.ndarray:
        cap = max(self.cloud_size(), 1)
        out = np.zeros(cap, POINT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.lv_cloud_fetch(self.h, C.c_double(t1), C.c_double(t2), out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(n)))
        return out[: n.value].copy()

    def cloud_reserve(self, max_points_per_message: int, point_step: int, buffer_points: int):
        self._check(self.lib.lv_cloud_reserve(self.h, C.c_size_t(max_points_per_message), C.c_size_t(point_step), C.c_size_t(buffer_points)))

    def reserve_stream(self, max_window_points: int, max_scan_points: int):
        self._check(self.lib.lv_reserve_stream(self.h, C.c_size_t(max_window_points), C.c_size_t(max_scan_points)))

    def cloud_clear(self, t: float):
        self._check(self.lib.lv_cloud_clear(self.h, C.c_double(t)))

    def scan_deskew_window(self, t1, t2, states, Xt2, downsample_prec=0.5) -> int:
        st = np.ascontiguousarray(states)
        x2 = np.ascontiguousarray(Xt2)
        assert st.dtype.itemsize == 184 and x2.dtype.itemsize == 184
        nw = C.c_size_t(0)
        self._check(self.lib.lv_scan_deskew_window(self.h, C.c_double(t1), C.c_double(t2), st.ctypes.data_as(C.c_void_p), C.c_size_t(len(st)),
                                                   x2.ctypes.data_as(C.c_void_p), C.c_float(downsample_prec), C.byref(nw)))
        self._n = self.scan_size()
        return int(nw.value)

    def scan_size(self) -> int:
        return int(self.lib.lv_scan_size(self.h))

    def scan_route(self) -> int:
        """SCAN_ROUTE_*: the chain that produced the current scan (a decline followed by the general chain: general)."""
        return int(self.lib.lv_scan_route(self.h))

    def scan_fetch(self) -> np.ndarray:
        n = self.scan_size()
        out = np.empty((n, 3), np.float32)
        self._check(self.lib.lv_scan_fetch(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out

    def iterate(self, state) -> dict:
        s = np.ascontiguousarray(state, np.float64)
        out = Sums()
        self._check(self.lib.lv_iterate(self.h, s.ctypes.data_as(C.c_void_p), C.byref(out)))
        return out.as_dict()

    def iterate_batch(self, states) -> list:
        """lv_iterate_batch: one measurement pass per state ([m, 26]) against the current scan -> m sums dicts."""
        xs = np.ascontiguousarray(np.asarray(states, np.float64).reshape(-1, 26))
        m = len(xs)
        out = (Sums * max(m, 1))()
        self._check(self.lib.lv_iterate_batch(self.h, xs.ctypes.data_as(C.c_void_p), C.c_size_t(m), out))
        return [out[i].as_dict() for i in range(m)]

    def update_batch(self, states, P, want_P=False):
        """lv_update_batch: m independent iterated updates from states ([m, 26]) with the shared prior covariance P ->
        (xs [m, 26], Ps [m, 23, 23] or None, passes [m], the sums of each hypothesis' last pass as m dicts)."""
        xs = np.ascontiguousarray(np.asarray(states, np.float64).reshape(-1, 26)).copy()
        m = len(xs)
        Pm = np.ascontiguousarray(P, np.float64).reshape(NS * NS)
        Ps = np.zeros((m, NS, NS)) if want_P else None
        passes = np.zeros(m, np.int32)
        last = (Sums * max(m, 1))()
        self._check(self.lib.lv_update_batch(self.h, xs.ctypes.data_as(C.c_void_p), C.c_size_t(m), Pm.ctypes.data_as(C.POINTER(C.c_double)),
                                             Ps.ctypes.data_as(C.POINTER(C.c_double)) if want_P else None,
                                             passes.ctypes.data_as(C.POINTER(C.c_int)), last))
        return xs, Ps, passes, [last[i].as_dict() for i in range(m)]

    def update(self, state, P, want_trace=True):
        if not want_trace:
            self._xb[:] = state
            self._Pb[:] = np.asarray(P).reshape(NS, NS)
            rc = self.lib.lv_update(self.h, self._xp, self._Pp, self._passes_ref, None, None)
            if rc != LV_OK:
                self._check(rc)
            return self._xb.copy(), self._Pb.copy(), self._passes.value, None, []
        x = np.ascontiguousarray(state, np.float64).copy()
        Pm = np.ascontiguousarray(P, np.float64).copy().reshape(NS, NS)
        npass = self.params.MAX_NUM_ITERS + 1
        passes = C.c_int(0)
        sums = (Sums * npass)()
        trace = np.zeros((npass, 49))
        self._check(self.lib.lv_update(self.h, x.ctypes.data_as(C.c_void_p), Pm.ctypes.data_as(C.c_void_p), C.byref(passes),
                                       sums if want_trace else None,
                                       trace.ctypes.data_as(C.c_void_p) if want_trace else None))
        n = passes.value
        return x, Pm, n, trace[:n], [sums[i].as_dict() for i in range(n)] if want_trace else []

    # --- resident filter (row f-3)
    def filter_set(self, state, P):
        x = np.ascontiguousarray(state, np.float64)
        Pm = np.ascontiguousarray(P, np.float64)
        self._check(self.lib.lv_filter_set(self.h, x.ctypes.data_as(C.c_void_p), Pm.ctypes.data_as(C.c_void_p)))

    def filter_get(self):
        x = np.zeros(26)
        Pm = np.zeros((NS, NS))
        self._check(self.lib.lv_filter_get(self.h, x.ctypes.data_as(C.c_void_p), Pm.ctypes.data_as(C.c_void_p)))
        return x, Pm

    def predict(self, dt, Q, acc, gyro):
        Qm = np.ascontiguousarray(Q, np.float64)
        a = np.ascontiguousarray(acc, np.float64)
        g = np.ascontiguousarray(gyro, np.float64)
        self._check(self.lib.lv_predict(self.h, C.c_double(dt), Qm.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                        g.ctypes.data_as(C.c_void_p)))

    # --- aiding observations (include/limovelo_hip.h "Aiding observations"; limo_velo_amd.aiding builds the records)
    def observe(self, obs_list, wait=False):
        """Applies 1..OBSERVE_BATCH observations (capi.Observation, or one of them) to the resident filter, in order, behind the
        queued predictions.  wait=False only enqueues and returns None; wait=True returns the results as observe_results() does."""
        if isinstance(obs_list, Observation):
            obs_list = [obs_list]
        n = len(obs_list)
        arr = (Observation * max(n, 1))(*obs_list)
        out = (ObserveResult * max(n, 1))() if wait else None
        self._check(self.lib.lv_observe(self.h, arr, n, out))
        return [self._observe_dict(r) for r in out[:n]] if wait else None

    def observe_results(self):
        """The results of the last observe(): a list of dicts {status, rows, nis, y}.  Waits for the stream."""
        out = (ObserveResult * OBSERVE_BATCH)()
        n = C.c_size_t(0)
        self._check(self.lib.lv_observe_results(self.h, out, OBSERVE_BATCH, C.byref(n)))
        return [self._observe_dict(r) for r in out[: n.value]]

    @staticmethod
    def _observe_dict(r):
        return dict(status=int(r.status), rows=int(r.rows), nis=float(r.nis), y=np.array(r.y[:], np.float64))

    def correct(self, want_passes=True) -> int:
        p = C.c_int(0)
        self._check(self.lib.lv_correct(self.h, C.byref(p) if want_passes else None))
        return p.value

    def degeneracy_values(self) -> np.ndarray:
        """[passes, 6] eigenvalues of the pose block of H^T H of the last update (degeneracy_mode >= 1)."""
        eig = np.zeros((16, 6))
        n = C.c_int(0)
        self._check(self.lib.lv_get_degeneracy_values(self.h, eig.ctypes.data_as(C.c_void_p), 16, C.byref(n)))
        return eig[: n.value].copy()

    def update_begin(self, state, P):
        x = np.ascontiguousarray(state, np.float64)
        Pm = np.ascontiguousarray(P, np.float64)
        self._check(self.lib.lv_update_begin(self.h, x.ctypes.data_as(C.c_void_p), Pm.ctypes.data_as(C.c_void_p)))

    def pass_reduce(self):
        self._check(self.lib.lv_pass_reduce(self.h))

    def pass_solve(self):
        self._check(self.lib.lv_pass_solve(self.h))

    def sums_device_ptr(self) -> int:
        return int(self.lib.lv_sums_device_ptr(self.h))

    # --- collective inside the library (row e)
    def comm_unique_id(self, rccl_library: str | None = None) -> bytes:
        buf = C.create_string_buffer(128)
        lib = rccl_library.encode() if rccl_library else None
        self._check(self.lib.lv_comm_unique_id(lib, buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int, rccl_library: str | None = None):
        if len(unique_id) != 128:
            raise ValueError("unique id must be 128 bytes")
        lib = rccl_library.encode() if rccl_library else None
        self._check(self.lib.lv_comm_init(self.h, lib, C.c_char_p(unique_id), int(rank), int(world)))

    def comm_destroy(self):
        self._check(self.lib.lv_comm_destroy(self.h))

    def comm_world(self) -> int:
        return int(self.lib.lv_comm_world(self.h))

    def set_sums_buffer(self, device_ptr: int | None):
        self._check(self.lib.lv_set_sums_buffer(self.h, C.c_void_p(device_ptr or 0)))

    def update_end(self):
        x = np.zeros(26)
        Pm = np.zeros((NS, NS))
        passes = C.c_int(0)
        self._check(self.lib.lv_update_end(self.h, x.ctypes.data_as(C.c_void_p), Pm.ctypes.data_as(C.c_void_p), C.byref(passes)))
        return x, Pm, passes.value

    def set_stream(self, stream_handle: int | None):
        self._check(self.lib.lv_set_stream(self.h, C.c_void_p(stream_handle or 0)))

    def get_stream(self) -> int:
        return int(self.lib.lv_get_stream(self.h) or 0)

    def synchronize(self):
        self._check(self.lib.lv_synchronize(self.h))

    def set_capture(self, on: bool):
        self._check(self.lib.lv_set_capture(self.h, int(on)))

    def set_profiling(self, mode):
        self._check(self.lib.lv_set_profiling(self.h, int(mode)))

    def level_histogram(self) -> list:
        out = (C.c_int * 8)()
        self._check(self.lib.lv_get_level_histogram(self.h, out))
        return list(out)

    def solve_clocks(self) -> np.ndarray:
        out = np.zeros((16, 16), np.int64)
        self._check(self.lib.lv_get_solve_clocks(self.h, out.ctypes.data_as(C.c_void_p), 256))
        return out

    def phase_clocks(self, capacity=4096) -> np.ndarray:
        out = np.zeros((capacity, 8), np.int64)
        nb = C.c_int(0)
        self._check(self.lib.lv_get_phase_clocks(self.h, out.ctypes.data_as(C.c_void_p), capacity, C.byref(nb)))
        return out[:nb.value]

    def timing(self) -> dict:
        t = Timing()
        self._check(self.lib.lv_get_timing(self.h, C.byref(t)))
        out = {k: getattr(t, k) for k, _ in Timing._fields_}
        out["pass_match_ms"] = list(t.pass_match_ms)
        out["pass_solve_ms"] = list(t.pass_solve_ms)
        out["pass_collective_ms"] = list(t.pass_collective_ms)
        return out

    # --- fetches
    def fetch_knn(self):
        n = self._n
        k = self.params.NUM_MATCH_POINTS
        idx = np.empty((n, k), np.uint32)
        d2 = np.empty((n, k), np.float32)
        self._check(self.lib.lv_fetch_knn(self.h, idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p)))
        return idx, d2

    def set_record_dump(self, on=True):
        """pass_kernel (one launch per pass) also stores its hand-over records to memory (for fetch_neighbors)."""
        self._check(self.lib.lv_set_record_dump(self.h, int(on)))

    def comm_set_shard_max(self, n_max: int):
        """The largest shard of the current scan over the ranks (same value on every rank, after every scan_set)."""
        self.lib.lv_comm_set_shard_max.argtypes = [C.c_void_p, C.c_size_t]
        self._check(self.lib.lv_comm_set_shard_max(self.h, int(n_max)))

    def set_comm_fused(self, on=True):
        self._check(self.lib.lv_set_comm_fused(self.h, int(on)))

    GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int)

    def comm_set_host_gather(self, rank: int, world: int, fn):
        """The one-launch-per-pass multi-rank form with the caller's transport (lv_comm_set_host_gather).
        fn(slots: float64 array of world * n, n, rank, world) fills every other rank's slots[r * n:(r + 1) * n] in place
        (this rank's partials are already at [rank * n:(rank + 1) * n]); None removes the transport."""
        self.lib.lv_comm_set_host_gather.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        if fn is None:
            self._check(self.lib.lv_comm_set_host_gather(self.h, 0, 1, None, None))
            self._gather_cb = None
            return

        def tramp(_user, slots, bytes_per_rank, r, w):
            try:
                n = bytes_per_rank // 8
                arr = np.ctypeslib.as_array((C.c_double * (n * w)).from_address(slots))
                fn(arr, n, r, w)
                return 0
            except Exception as e:  # noqa: BLE001 — an exception must not unwind through the C frames
                print(f"[limo_velo_amd] host gather callback failed: {e!r}", flush=True)
                return 1

        cb = self.GATHER_FN(tramp)
        self._check(self.lib.lv_comm_set_host_gather(self.h, int(rank), int(world), C.cast(cb, C.c_void_p), None))
        self._gather_cb = cb   # (keeps the trampoline alive as long as the library may call it)

    def comm_peer_export(self) -> bytes:
        buf = (C.c_ubyte * PEER_HANDLE_BYTES)()
        self._check(self.lib.lv_comm_peer_export(self.h, buf))
        return bytes(buf)

    def comm_peer_init(self, rank: int, world: int, handles):
        blob = b"".join(handles)
        assert len(blob) == PEER_HANDLE_BYTES * world
        self._check(self.lib.lv_comm_peer_init(self.h, int(rank), int(world), blob))

    def set_fused_pass(self, on=True):
        self._check(self.lib.lv_set_fused_pass(self.h, int(on)))

    def set_option(self, name: str, value: int):
        self._check(self.lib.lv_set_option(self.h, name.encode(), int(value)))

    def pass_clocks(self, slots=None):
        """[launch][workgroup slot][32] stamps of the last update's pass_kernel launches, and the number of search
        workgroups n (slot n - 1 of a launch = its bookkeeping workgroup, stamp 10 = books done).  The slot count
        (the library's stride: its workgroup limit + 1) is asked from the library."""
        if slots is None:
            q = C.c_int(0)
            self._check(self.lib.lv_get_pass_clocks(self.h, None, 0, C.byref(q)))
            slots = q.value
        nl = self.params.MAX_NUM_ITERS + 2
        buf = np.zeros((nl, slots, 32), np.int64)
        n = C.c_int(0)
        self._check(self.lib.lv_get_pass_clocks(self.h, buf.ctypes.data_as(C.c_void_p), slots, C.byref(n)))
        return buf, n.value

    def last_update_fused(self) -> bool:
        return bool(self.lib.lv_last_update_fused(self.h))

    def last_passes(self) -> int:
        """Passes of the last update whose results have been fetched (lv_update, or lv_correct + lv_filter_get)."""
        return int(self.lib.lv_last_passes(self.h))

    def fetch_neighbors(self):
        """Neighbour coordinates / squared distances / world points / found counts out of the hand-over records of
        the most recent pass (works for the non-capturing, timed kernels)."""
        n = self._n
        k = self.params.NUM_MATCH_POINTS
        nbr = np.empty((n, k, 3), np.float32)
        d2 = np.empty((n, k), np.float32)
        pw = np.empty((n, 3), np.float32)
        found = np.empty(n, np.int32)
        self._check(self.lib.lv_fetch_neighbors(self.h, nbr.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p),
                                                pw.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p)))
        return nbr, d2, pw, found

    def fetch_matches(self):
        n = self._n
        valid = np.empty(n, np.uint8)
        pw = np.empty((n, 3), np.float32)
        abcd = np.empty((n, 4), np.float32)
        dist = np.empty(n, np.float32)
        self._check(self.lib.lv_fetch_matches(self.h, valid.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p),
                                              abcd.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p)))
        return valid, pw, abcd, dist

    def calculate_H(self, state, p_world, abcd, dist):
        s = np.ascontiguousarray(state, np.float64)
        pw = np.ascontiguousarray(p_world, np.float32)
        ab = np.ascontiguousarray(abcd, np.float32)
        di = np.ascontiguousarray(dist, np.float32)
        n = len(di)
        H = np.zeros((n, 12))
        h = np.zeros(n)
        self._check(self.lib.lv_calculate_H(self.h, s.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p),
                                            ab.ctypes.data_as(C.c_void_p), di.ctypes.data_as(C.c_void_p), C.c_size_t(n),
                                            H.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p)))
        return H, h

    def fetch_rows(self):
        n = self._n
        H = np.empty((n, 12), np.float64)
        h = np.empty(n, np.float64)
        self._check(self.lib.lv_fetch_rows(self.h, H.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p)))
        return H, h
