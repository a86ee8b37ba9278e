"""ctypes loader for libsslam_hip.so (the C-ABI declared in include/sslam.h).

Fails loudly: if the shared library is missing or cannot be loaded an ImportError/OSError is
raised — there is no eager/CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def library_path() -> str:
    return os.path.join(_PKG, "libsslam_hip.so")


def build_library(force: bool = False) -> str:
    """Compile every HIP source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_PKG, "csrc"), "-s"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return library_path()


class OptStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("trials", C.c_int), ("status", C.c_int), ("host_plan_us", C.c_int),
                ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("lambda_", C.c_double),
                ("seconds", C.c_double), ("solver_iterations", C.c_int64)]

    def __repr__(self):
        return (f"OptStats(iterations={self.iterations}, trials={self.trials}, status={self.status}, "
                f"chi2 {self.chi2_before:.6g} -> {self.chi2_after:.6g}, lambda={self.lambda_:.3g}, "
                f"seconds={self.seconds:.4f}, solver_iterations={self.solver_iterations})")


class MapStats(C.Structure):
    """``sslam_map_stats`` (include/sslam.h)"""
    _fields_ = [("n_clouds", C.c_int32), ("n_points", C.c_int32), ("n_used", C.c_int32), ("n_bricks", C.c_int32), ("n_voxels", C.c_int32),
                ("upload_bytes", C.c_int64), ("kernel_ms", C.c_double)]

    def __repr__(self):
        return (f"MapStats(n_clouds={self.n_clouds}, n_points={self.n_points}, n_used={self.n_used}, n_bricks={self.n_bricks}, "
                f"n_voxels={self.n_voxels}, upload_bytes={self.upload_bytes}, kernel_ms={self.kernel_ms:.4f})")


class OccParams(C.Structure):
    """``sslam_occ_params`` (include/sslam.h); ``sslam_occ_default_params`` fills it"""
    _fields_ = [("resolution", C.c_float), ("max_range", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("sensor_origin", C.c_float * 3),
                ("l_hit", C.c_float), ("l_miss", C.c_float), ("l_min", C.c_float), ("l_max", C.c_float), ("l_occ", C.c_float), ("emit", C.c_int32)]


class OccStats(C.Structure):
    """``sslam_occ_stats`` (include/sslam.h)"""
    _fields_ = [("n_clouds", C.c_int32), ("n_points", C.c_int32), ("n_rays", C.c_int32), ("n_truncated", C.c_int32), ("n_clipped_z", C.c_int32),
                ("n_bricks", C.c_int32), ("n_cells", C.c_int32), ("reserved", C.c_int32), ("n_steps", C.c_int64), ("upload_bytes", C.c_int64),
                ("kernel_ms", C.c_double)]

    def __repr__(self):
        return (f"OccStats(n_clouds={self.n_clouds}, n_points={self.n_points}, n_rays={self.n_rays}, n_truncated={self.n_truncated}, "
                f"n_clipped_z={self.n_clipped_z}, n_bricks={self.n_bricks}, n_cells={self.n_cells}, n_steps={self.n_steps}, "
                f"upload_bytes={self.upload_bytes}, kernel_ms={self.kernel_ms:.4f})")


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C semantic_slam_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp, ci, cd, i64 = C.c_void_p, C.c_int, C.c_double, C.c_int64
    dp = C.POINTER(C.c_double)
    sig = {
        "sslam_last_error": (C.c_char_p, []),
        "sslam_device_count": (ci, []),
        "sslam_pinned_alloc": (vp, [C.c_size_t]),
        "sslam_pinned_free": (None, [vp]),
        "sslam_graph_create": (vp, [ci]),
        "sslam_graph_destroy": (None, [vp]),
        "sslam_graph_add_vertex_se3": (ci, [vp, dp, ci]),
        "sslam_graph_add_vertex_point": (ci, [vp, dp]),
        "sslam_graph_add_vertex_plane": (ci, [vp, dp]),
        "sslam_graph_add_edge_se3": (ci, [vp, ci, ci, dp, dp]),
        "sslam_graph_add_edge_se3_point": (ci, [vp, ci, ci, dp, dp]),
        "sslam_graph_add_edge_se3_plane": (ci, [vp, ci, ci, dp, dp]),
        "sslam_graph_add_edge_point_point": (ci, [vp, ci, ci, dp, dp]),
        "sslam_graph_add_edge_se3_prior_xyz": (ci, [vp, ci, dp, dp]),
        "sslam_graph_add_edge_se3_prior_xy": (ci, [vp, ci, dp, dp]),
        "sslam_graph_num_vertices": (ci, [vp]),
        "sslam_graph_num_edges": (ci, [vp]),
        "sslam_graph_get_vertex": (ci, [vp, ci, dp]),
        "sslam_graph_set_vertex": (ci, [vp, ci, dp]),
        "sslam_graph_hessian_index": (ci, [vp, ci]),
        "sslam_graph_set_option": (ci, [vp, C.c_char_p, cd]),
        "sslam_graph_set_edge_robust_kernel": (ci, [vp, ci, ci, cd]),
        "sslam_graph_get_edge_robust_kernel": (ci, [vp, ci, C.POINTER(ci), dp]),
        "sslam_graph_edge_chi2": (ci, [vp, C.POINTER(ci), ci, dp, dp, dp]),
        "sslam_graph_optimize": (ci, [vp, ci, C.POINTER(OptStats)]),
        "sslam_graph_chi2": (ci, [vp, dp]),
        "sslam_graph_marginals": (ci, [vp, C.POINTER(ci), ci, dp]),
        "sslam_graph_marginals_by_hessian_index": (ci, [vp, C.POINTER(ci), ci, dp]),
        "sslam_graph_save_g2o": (ci, [vp, C.c_char_p]),
        "sslam_graph_load_g2o": (ci, [vp, C.c_char_p]),
        "sslam_graph_linearize": (ci, [vp, C.POINTER(ci), C.POINTER(i64), vp, vp, vp, vp]),
        "sslam_graph_solve": (ci, [vp, cd, dp, C.POINTER(i64)]),
        "sslam_graph_oplus": (ci, [vp, dp]),
        "sslam_debug_plan_create": (vp, [C.POINTER(vp), ci]),
        "sslam_debug_plan_destroy": (None, [vp]),
        "sslam_debug_plan_array": (i64, [vp, C.c_char_p, vp, i64]),
        "sslam_debug_voxel_geometry": (ci, [vp, vp, C.c_float, vp, vp]),
        "sslam_batch_create": (vp, [C.POINTER(vp), ci]),
        "sslam_batch_create_streams": (vp, [C.POINTER(vp), ci, ci]),
        "sslam_batch_destroy": (None, [vp]),
        "sslam_batch_upload": (ci, [vp]),
        "sslam_batch_download": (ci, [vp]),
        "sslam_batch_optimize": (ci, [vp, ci, C.POINTER(OptStats)]),
        "sslam_batch_marginals": (ci, [vp, C.POINTER(C.c_int32), ci, dp]),
        "sslam_batch_gate": (ci, [vp, C.POINTER(C.c_int32), dp, dp, ci, dp, dp, dp]),
        "sslam_graph_gate": (ci, [vp, C.POINTER(C.c_int32), dp, dp, ci, dp, dp, dp]),
        "sslam_batch_solve": (i64, [vp, dp, dp, i64, C.POINTER(i64)]),
        "sslam_comm_unique_id": (ci, [C.c_char_p]),
        "sslam_batch_comm_init": (ci, [vp, C.c_char_p, ci, ci]),
        "sslam_batch_set_edge_shard": (ci, [vp, ci, ci]),
        "sslam_batch_linearize_hb": (i64, [vp, dp, i64]),
        "sslam_batch_time_linearize": (ci, [vp, ci, dp]),
        "sslam_batch_time_solver": (ci, [vp, ci, dp, dp]),
        "sslam_batch_linearize_bytes": (i64, [vp]),
        "sslam_batch_info": (ci, [vp, C.c_char_p, dp]),
        "sslam_batch_set_profiling": (ci, [vp, ci]),
        "sslam_batch_kernel_time": (ci, [vp, C.c_char_p, dp, C.POINTER(i64)]),
        "sslam_seg_fitness_scores": (ci, [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, dp]),
        "sslam_seg_register_pairs": (ci, [vp, vp, vp, ci, vp, ci, ci, cd, vp, vp, vp, dp]),
        "sslam_gicp_default_params": (None, [vp]),
        "sslam_seg_cloud_covariances": (ci, [vp, vp, vp, ci, ci, cd, vp, vp, dp]),
        "sslam_seg_register_pairs_gicp": (ci, [vp, vp, vp, ci, vp, ci, vp, vp, ci, cd, vp, vp, vp, dp]),
        "sslam_slam_set_loop_registration": (ci, [vp, ci, vp]),
        "sslam_slam_loop_covariance_passes": (ci, [vp, C.POINTER(i64)]),
        "sslam_inf_default_params": (None, [vp]),
        "sslam_information_from_fitness": (ci, [vp, cd, dp]),
        "sslam_slam_set_fitness_information": (ci, [vp, vp, C.c_float, cd]),
        "sslam_slam_last_fitness": (ci, [vp, vp, vp, ci]),
        "sslam_seg_map_cloud": (ci, [vp, vp, vp, ci, vp, C.c_float, ci, vp, vp, vp, ci, C.POINTER(MapStats)]),
        "sslam_seg_last_map_timing": (ci, [vp, vp]),
        "sslam_slam_set_map_clouds": (ci, [vp, ci, C.c_float]),
        "sslam_slam_map_clouds_kept": (ci, [vp, C.POINTER(C.c_int32)]),
        "sslam_slam_map_cloud": (ci, [vp, C.c_float, ci, vp, vp, vp, ci, vp, vp, ci, C.POINTER(MapStats)]),
        "sslam_occ_default_params": (None, [C.POINTER(OccParams)]),
        "sslam_seg_occupancy_map": (ci, [vp, vp, vp, ci, vp, C.POINTER(OccParams), vp, vp, vp, vp, ci, C.POINTER(OccStats)]),
        "sslam_seg_last_occupancy_timing": (ci, [vp, vp]),
        "sslam_slam_occupancy_map": (ci, [vp, C.POINTER(OccParams), vp, vp, vp, vp, ci, C.POINTER(OccStats)]),
        "sslam_seg_occupancy_map_scans": (ci, [vp, vp, vp, ci, vp, C.POINTER(OccParams), vp, vp, vp, vp, ci, C.POINTER(OccStats)]),
        "sslam_seg_last_occupancy_scan_timing": (ci, [vp, vp]),
        "sslam_seg_last_occupancy_scan_counts": (ci, [vp, vp]),
        "sslam_slam_occupancy_map_scans": (ci, [vp, C.POINTER(OccParams), vp, vp, vp, vp, ci, C.POINTER(OccStats)]),
        "sslam_seg_radius_outlier_removal": (ci, [vp, vp, ci, cd, ci, vp, ci, vp]),
        "sslam_prefilter_default_params": (None, [vp]),
        "sslam_seg_prefilter": (ci, [vp, vp, ci, vp, vp, ci, vp, dp]),
        "sslam_odom_default_params": (None, [vp]),
        "sslam_odom_create": (vp, [vp, vp]),
        "sslam_odom_destroy": (None, [vp]),
        "sslam_odom_reset": (ci, [vp]),
        "sslam_odom_push": (ci, [vp, vp, ci, C.c_int32, C.c_int32, vp, vp]),
        "sslam_odom_keyframe": (ci, [vp, vp, ci, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: loud by design
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib
