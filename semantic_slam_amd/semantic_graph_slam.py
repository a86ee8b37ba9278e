"""Host-side mirror of the reference's orchestrator, ``semantic_graph_slam`` (reference include/ps_graph_slam/semantic_graph_slam.h,
src/ps_graph_slam/semantic_graph_slam.cpp), over the C-ABI ``sslam_slam_*`` of include/sslam.h.

Method names follow the reference (``VIOCallback``, ``run``, ``setPointCloudData``, ``setDetectedObjectInfo``, ``getRobotPose``,
``getMap2OdomTrans``, ``getMappedLandmarks``, ``getKeyframes``, ``saveGraph``); the ROS parameters become ``SlamParams`` fields.
There is no CPU fallback: the tick's frontend pass, optimisation, marginals and data association all run on the GPU.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from ._lib import load_library, MapStats, OccParams, OccStats, OptStats
from .graph_slam import SslamError, _pose7
from .segmentation import DBL_MAX, GicpParams, InfParams, Plane, PointCloudSegmentation, default_inf_params, occupancy_default_params  # noqa: F401


class SlamParams(C.Structure):   # sslam_slam_params
    _fields_ = [("keyframe_delta_trans", C.c_double), ("keyframe_delta_angle", C.c_double), ("keyframe_delta_time", C.c_double),
                ("max_keyframes_per_update", C.c_int), ("update_keyframes_using_detections", C.c_int),
                ("camera_angle_deg", C.c_double), ("add_first_lan", C.c_int), ("first_lan", C.c_double * 3),
                ("use_const_inf_matrix", C.c_int), ("const_stddev_x", C.c_double), ("const_stddev_q", C.c_double),
                ("maha_dist_thres", C.c_double), ("eq_dist_thres", C.c_double), ("land_noise_low", C.c_double),
                ("land_noise_high", C.c_double), ("use_maha_dist", C.c_int), ("use_eq_dist", C.c_int), ("use_rtab_map_odom", C.c_int),
                ("max_iterations", C.c_int), ("reference_quirks", C.c_int), ("device", C.c_int)]


class Landmark(C.Structure):     # sslam_landmark (include/ps_graph_slam/landmark.h:17-33)
    _fields_ = [("id", C.c_int32), ("vertex", C.c_int32), ("class_id", C.c_int32), ("plane_type", C.c_int32), ("is_new", C.c_int32),
                ("pose", C.c_float * 3), ("local_pose", C.c_float * 3), ("covariance", C.c_float * 9), ("normal", C.c_float * 4),
                ("distance", C.c_float)]


class TickStats(C.Structure):    # sslam_tick_stats
    _fields_ = [("keyframes_added", C.c_int), ("landmarks_added", C.c_int), ("landmarks_matched", C.c_int),
                ("landmark_edges_added", C.c_int), ("optimized", C.c_int), ("marginals_ok", C.c_int), ("opt", OptStats),
                ("seconds_frontend", C.c_double), ("seconds_association", C.c_double), ("seconds_optimize", C.c_double),
                ("seconds_marginals", C.c_double)]


class LoopParams(C.Structure):   # sslam_loop_params
    _fields_ = [("distance_thresh", C.c_double), ("accum_distance_thresh", C.c_double), ("distance_from_last_edge_thresh", C.c_double),
                ("fitness_score_max_range", C.c_double), ("fitness_score_thresh", C.c_double), ("max_iterations", C.c_int32),
                ("epsilon", C.c_double), ("max_candidates", C.c_int32), ("voxel_leaf", C.c_float), ("gate_chi2", C.c_double),
                ("robust_kernel", C.c_int32), ("robust_delta", C.c_double), ("inf", InfParams)]


class Loop(C.Structure):         # sslam_loop
    _fields_ = [("new_vertex", C.c_int32), ("cand_vertex", C.c_int32), ("n_candidates", C.c_int32), ("outcome", C.c_int32),
                ("edge_id", C.c_int32), ("used", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("T", C.c_double * 12), ("score", C.c_double), ("d2", C.c_double)]


LOOP_ADDED, LOOP_SCORE, LOOP_GATE, LOOP_NO_MATCH = 0, 1, 2, 3   # SSLAM_LOOP_*
REG_ICP, REG_GICP = 0, 1                                        # SSLAM_REG_*
REG_METHODS = {"ICP": REG_ICP, "GICP": REG_GICP, "FAST_GICP": REG_GICP}   # hdl_graph_slam's registration_method names

_BOUND = False


def _bind(lib):
    global _BOUND
    if _BOUND:
        return
    vp, ci = C.c_void_p, C.c_int
    lib.sslam_slam_default_params.restype = None; lib.sslam_slam_default_params.argtypes = [C.POINTER(SlamParams)]
    lib.sslam_slam_create.restype = vp; lib.sslam_slam_create.argtypes = [C.POINTER(SlamParams), vp]
    lib.sslam_slam_destroy.restype = None; lib.sslam_slam_destroy.argtypes = [vp]
    lib.sslam_slam_set_point_cloud.restype = ci; lib.sslam_slam_set_point_cloud.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci]
    lib.sslam_slam_set_detected_objects.restype = ci; lib.sslam_slam_set_detected_objects.argtypes = [vp, vp, ci]
    lib.sslam_slam_set_segmented_objects.restype = ci; lib.sslam_slam_set_segmented_objects.argtypes = [vp, vp, ci]
    lib.sslam_slam_vio.restype = ci; lib.sslam_slam_vio.argtypes = [vp, C.c_int32, C.c_int32, vp]
    lib.sslam_slam_run.restype = ci; lib.sslam_slam_run.argtypes = [vp, C.POINTER(TickStats)]
    lib.sslam_slam_robot_pose.restype = ci; lib.sslam_slam_robot_pose.argtypes = [vp, vp]
    lib.sslam_slam_map2odom.restype = ci; lib.sslam_slam_map2odom.argtypes = [vp, vp]
    lib.sslam_slam_landmarks.restype = ci; lib.sslam_slam_landmarks.argtypes = [vp, vp, ci]
    lib.sslam_slam_keyframes.restype = ci; lib.sslam_slam_keyframes.argtypes = [vp, vp, vp, ci]
    lib.sslam_slam_graph.restype = vp; lib.sslam_slam_graph.argtypes = [vp]
    lib.sslam_slam_find_matches.restype = ci; lib.sslam_slam_find_matches.argtypes = [vp, vp, ci, vp, vp]
    # sslam_slam_set_fitness_information, sslam_slam_last_fitness, sslam_slam_set_map_clouds, sslam_slam_map_cloud,
    # sslam_slam_occupancy_map: declared in _lib.load_library
    lib.sslam_loop_default_params.restype = None; lib.sslam_loop_default_params.argtypes = [C.POINTER(LoopParams)]
    lib.sslam_slam_set_loop_closure.restype = ci; lib.sslam_slam_set_loop_closure.argtypes = [vp, C.POINTER(LoopParams)]
    lib.sslam_slam_last_loops.restype = ci; lib.sslam_slam_last_loops.argtypes = [vp, vp, ci]
    lib.sslam_slam_last_loop_timing.restype = ci; lib.sslam_slam_last_loop_timing.argtypes = [vp, vp]
    lib.sslam_slam_loop_candidates.restype = ci
    lib.sslam_slam_loop_candidates.argtypes = [vp, vp, ci, vp, ci, C.POINTER(LoopParams), vp, vp, ci]
    _BOUND = True


def default_slam_params(device: int = 0) -> SlamParams:
    lib = load_library(); _bind(lib)
    p = SlamParams()
    lib.sslam_slam_default_params(C.byref(p))
    p.device = device
    return p


def default_loop_params() -> LoopParams:
    """``sslam_loop_default_params``: hdl_graph_slam's LoopDetector defaults, Huber 1.0 on the loop edge, no gate"""
    lib = load_library(); _bind(lib)
    p = LoopParams()
    lib.sslam_loop_default_params(C.byref(p))
    return p


class SemanticGraphSLAM:
    """``semantic_graph_slam`` without ROS: feed it what the node's callbacks receive, call :meth:`run` where the node's loop does."""

    def __init__(self, params: SlamParams | None = None, segmentation: PointCloudSegmentation | None = None, device: int = 0):
        self._lib = load_library(); _bind(self._lib)
        self.params = params if params is not None else default_slam_params(device)
        self._seg = segmentation   # kept alive: the handle is borrowed by the orchestrator
        self._h = self._lib.sslam_slam_create(C.byref(self.params), segmentation._h if segmentation is not None else None)
        if not self._h:
            raise SslamError(-1, self._lib.sslam_last_error().decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.sslam_slam_destroy(h)

    def _check(self, rc):
        if rc < 0:
            raise SslamError(rc, self._lib.sslam_last_error().decode())
        return rc

    # -- callbacks ------------------------------------------------------------------------------------------------------------
    def setPointCloudData(self, point_cloud):
        """semantic_graph_slam.cpp:341-345; ``point_cloud``: object with cloud / width / height / point_step / row_step / offsets"""
        f = point_cloud
        cloud = np.ascontiguousarray(f.cloud, np.uint8)
        self._check(self._lib.sslam_slam_set_point_cloud(self._h, cloud.ctypes.data, f.width, f.height, f.point_step, f.row_step,
                                                         f.offsets[0], f.offsets[1], f.offsets[2]))

    def setDetectedObjectInfo(self, object_info):
        """semantic_graph_slam.cpp:353-357"""
        boxes = PointCloudSegmentation._boxes(object_info)
        self._check(self._lib.sslam_slam_set_detected_objects(self._h, C.cast(boxes, C.c_void_p), len(boxes)))

    def setSegmentedObjects(self, planes):
        """extension: objects already segmented (a list of ``segmentation.Plane`` records) for the next keyframe"""
        arr = (Plane * max(len(planes), 1))(*planes)
        self._check(self._lib.sslam_slam_set_segmented_objects(self._h, C.cast(arr, C.c_void_p), len(planes)))

    def VIOCallback(self, stamp, odom) -> bool:
        """semantic_graph_slam.cpp:234-287.  ``stamp`` = (sec, nsec) or float seconds; ``odom`` = [t, q(x,y,z,w)] or a 4x4 isometry."""
        if isinstance(stamp, (tuple, list)):
            sec, nsec = int(stamp[0]), int(stamp[1])
        else:
            sec = int(np.floor(stamp)); nsec = int(round((stamp - sec) * 1e9))
        tq = _pose7(odom)
        return bool(self._check(self._lib.sslam_slam_vio(self._h, sec, nsec, tq.ctypes.data)))

    # -- the tick -------------------------------------------------------------------------------------------------------------
    def run(self) -> bool:
        """semantic_graph_slam.cpp:58-102; statistics of the tick in ``last_stats``"""
        st = TickStats()
        rc = self._check(self._lib.sslam_slam_run(self._h, C.byref(st)))
        self.last_stats = st
        return bool(rc)

    def set_fitness_information(self, params: InfParams | None = "default", voxel_leaf: float = 0.1, max_range: float | None = None) -> None:
        """``sslam_slam_set_fitness_information``: the odometry edges of the following ticks take the information matrix of the fitness
        score of their keyframes' clouds (InformationMatrixCalculator without ~use_const_inf_matrix).  ``params``: an ``InfParams``, the
        defaults, or None to go back to the constant matrix.  ``max_range`` bounds the SQUARED nearest-neighbour distance (None: no bound)."""
        if isinstance(params, str):
            params = default_inf_params()
        self._check(self._lib.sslam_slam_set_fitness_information(self._h, None if params is None else C.byref(params), C.c_float(voxel_leaf),
                                                                 C.c_double(DBL_MAX if max_range is None else max_range)))

    def last_fitness(self):
        """(scores, used) of the odometry edges the last ``run`` added, in order; -1 / -1 for an edge that took the constant matrix"""
        n = self._check(self._lib.sslam_slam_last_fitness(self._h, None, None, 0))
        score = np.zeros(max(n, 1)); used = np.zeros(max(n, 1), np.int32)
        self._check(self._lib.sslam_slam_last_fitness(self._h, score.ctypes.data, used.ctypes.data, n))
        return score[:n], used[:n]

    def set_loop_closure(self, params: LoopParams | None = "default") -> None:
        """``sslam_slam_set_loop_closure``: the following ticks search loop candidates among the processed keyframes, scan-match them,
        gate the best match and add the loop edge (hdl_graph_slam's LoopDetector::detect).  ``params``: a ``LoopParams``, the defaults, or
        None to turn it off.  Needs the frontend handle given to the constructor."""
        if isinstance(params, str):
            params = default_loop_params()
        self._check(self._lib.sslam_slam_set_loop_closure(self._h, None if params is None else C.byref(params)))

    def set_loop_registration(self, method="ICP", k: int = 20, plane_epsilon: float = 1e-3) -> None:
        """``sslam_slam_set_loop_registration``: the scan matcher of the loop stage, hdl_graph_slam's ``registration_method``.  ``method``:
        "ICP" / ``REG_ICP`` (the default of a handle) or "GICP" / "FAST_GICP" / ``REG_GICP``; with GICP every keyframe's downsampled
        cloud gets its covariances (``k`` neighbours, ``plane_epsilon``) once and the pairs go through ``register_pairs_gicp``."""
        if isinstance(method, str):
            if method not in REG_METHODS:
                raise ValueError(f"registration method {method!r}: one of {sorted(REG_METHODS)}")
            method = REG_METHODS[method]
        gp = GicpParams(int(k), float(plane_epsilon))
        self._check(self._lib.sslam_slam_set_loop_registration(self._h, int(method), C.byref(gp)))

    def loop_covariance_passes(self) -> int:
        """``sslam_slam_loop_covariance_passes``: keyframe clouds whose covariances were computed so far (GICP: one per keyframe with a cloud)"""
        n = C.c_int64(0)
        self._check(self._lib.sslam_slam_loop_covariance_passes(self._h, C.byref(n)))
        return n.value

    def last_loops(self):
        """the ``Loop`` records of the last ``run``: one per new keyframe that reached the selection with at least one candidate"""
        n = self._check(self._lib.sslam_slam_last_loops(self._h, None, 0))
        arr = (Loop * max(n, 1))()
        self._check(self._lib.sslam_slam_last_loops(self._h, C.cast(arr, C.c_void_p), n))
        return [arr[k] for k in range(n)]

    def last_loop_timing(self) -> np.ndarray:
        """wall seconds inside the last ``run``: candidate launch, registration, gate, the whole loop stage"""
        out = np.zeros(4)
        self._check(self._lib.sslam_slam_last_loop_timing(self._h, out.ctypes.data))
        return out

    def set_map_clouds(self, on: bool = True, keyframe_leaf: float = 0.1) -> None:
        """``sslam_slam_set_map_clouds``: the following ticks keep the downsampled cloud (``keyframe_leaf``) of every keyframe on the
        device for :meth:`map_cloud`; ``on=False`` drops what was kept.  Needs the frontend handle given to the constructor."""
        self._check(self._lib.sslam_slam_set_map_clouds(self._h, int(bool(on)), C.c_float(keyframe_leaf)))

    def map_cloud(self, resolution: float, min_points: int = 1):
        """``sslam_slam_map_cloud``: the kept keyframe clouds at their current estimates, one centroid per occupied voxel.  Returns
        (xyz [m, 3] float32, counts [m] int32, cells [m, 3] int32, vertex_ids [c] int32, poses [c, 12] float64, ``MapStats``); the poses
        (R row-major, then t) are what the map was built from."""
        st = MapStats()
        npts = C.c_int32(0)
        nc = self._check(self._lib.sslam_slam_map_clouds_kept(self._h, C.byref(npts)))
        cap = npts.value                                               # a voxel holds at least one point
        xyz = np.zeros((max(cap, 1), 3), np.float32); cnt = np.zeros(max(cap, 1), np.int32); cells = np.zeros((max(cap, 1), 3), np.int32)
        ids = np.zeros(max(nc, 1), np.int32); poses = np.zeros((max(nc, 1), 12))
        m = self._check(self._lib.sslam_slam_map_cloud(self._h, C.c_float(resolution), int(min_points), xyz.ctypes.data, cells.ctypes.data,
                                                       cnt.ctypes.data, cap, ids.ctypes.data, poses.ctypes.data, nc, C.byref(st)))
        nc = min(nc, st.n_clouds)                                      # 0 with map clouds off
        return xyz[:m].copy(), cnt[:m].copy(), cells[:m].copy(), ids[:nc], poses[:nc], st

    def occupancy_map(self, params: OccParams | None = None, max_out: int | None = None):
        """``sslam_slam_occupancy_map``: the kept keyframe clouds (:meth:`set_map_clouds`) at their current estimates, ray-cast into the sparse
        grid.  ``params`` defaults to :func:`occupancy_default_params`.  Returns (cells [m, 3] int32, hits [m] int32, misses [m] int32,
        logodds [m] float32, ``OccStats``); the poses are those :meth:`map_cloud` reports.  Without ``max_out`` a first call counts the
        records and a second one fetches them."""
        return self._occupancy_map(self._lib.sslam_slam_occupancy_map, params, max_out)

    def occupancy_map_scans(self, params: OccParams | None = None, max_out: int | None = None):
        """``sslam_slam_occupancy_map_scans``: the same kept clouds at the same poses through OctoMap's per-scan update -- every keyframe's cloud
        one scan, in keyframe order, a cell updated once per scan and clamped after every update.  Arguments and return values as for
        :meth:`occupancy_map`."""
        return self._occupancy_map(self._lib.sslam_slam_occupancy_map_scans, params, max_out)

    def _occupancy_map(self, entry, params, max_out):
        p = params if params is not None else occupancy_default_params()
        st = OccStats()
        cap = int(max_out) if max_out is not None else self._check(entry(self._h, C.byref(p), None, None, None, None, 0, C.byref(st)))
        cells = np.zeros((max(cap, 1), 3), np.int32); hits = np.zeros(max(cap, 1), np.int32); misses = np.zeros(max(cap, 1), np.int32)
        lo = np.zeros(max(cap, 1), np.float32)
        m = min(cap, self._check(entry(self._h, C.byref(p), cells.ctypes.data, hits.ctypes.data, misses.ctypes.data, lo.ctypes.data, cap, C.byref(st))))
        return cells[:m], hits[:m], misses[:m], lo[:m], st

    def loop_candidates(self, keys, news, params: LoopParams | None = None, cap: int | None = None):
        """``sslam_slam_loop_candidates`` (k_loop_candidates on its own).  ``keys`` / ``news``: [n, 3] float64 rows of x, y, accum_distance of
        the old / new keyframes.  Returns (cand [n_new, cap] int32 with -1 where not filled, count [n_new] int32); ``cap`` defaults to
        max_candidates, or the number of keys when that is 0."""
        p = params if params is not None else default_loop_params()
        k = np.ascontiguousarray(keys, np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(news, np.float64).reshape(-1, 3)
        if cap is None:
            cap = p.max_candidates if p.max_candidates else len(k)
        cand = np.full((len(q), cap), -1, np.int32)
        count = np.zeros(len(q), np.int32)
        self._check(self._lib.sslam_slam_loop_candidates(self._h, k.ctypes.data if len(k) else None, len(k), q.ctypes.data if len(q) else None, len(q),
                                                         C.byref(p), cand.ctypes.data if cand.size else None, count.ctypes.data if len(q) else None, cap))
        return cand, count

    # -- getters --------------------------------------------------------------------------------------------------------------
    def getRobotPose(self) -> np.ndarray:
        out = np.zeros(7)
        self._check(self._lib.sslam_slam_robot_pose(self._h, out.ctypes.data))
        return out

    def getMap2OdomTrans(self) -> np.ndarray:
        out = np.zeros(7)
        self._check(self._lib.sslam_slam_map2odom(self._h, out.ctypes.data))
        return out

    def getMappedLandmarks(self):
        n = self._check(self._lib.sslam_slam_landmarks(self._h, None, 0))
        arr = (Landmark * max(n, 1))()
        self._check(self._lib.sslam_slam_landmarks(self._h, C.cast(arr, C.c_void_p), n))
        return [arr[k] for k in range(n)]

    def getKeyframes(self):
        """(vertex ids, estimates[n, 7]) of the keyframes already in the graph"""
        n = self._check(self._lib.sslam_slam_keyframes(self._h, None, None, 0))
        ids = np.zeros(max(n, 1), np.int32); est = np.zeros((max(n, 1), 7))
        self._check(self._lib.sslam_slam_keyframes(self._h, ids.ctypes.data, est.ctypes.data, n))
        return ids[:n], est[:n]

    def saveGraph(self, path: str):
        g = self._lib.sslam_slam_graph(self._h)
        rc = self._lib.sslam_graph_save_g2o(g, path.encode())
        if rc < 0:
            raise SslamError(rc, self._lib.sslam_last_error().decode())

    def set_graph_option(self, key: str, value: float) -> None:
        """an option of the orchestrator's graph handle (sslam_graph_set_option through sslam_slam_graph): e.g. "speculative_trials" 0 for
        several robots sharing one GPU (ten speculative lanes fill the device; the plain single-launch solve takes a tenth of it)"""
        lib = self._lib
        lib.sslam_graph_set_option.restype = C.c_int
        lib.sslam_graph_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        rc = lib.sslam_graph_set_option(lib.sslam_slam_graph(self._h), key.encode(), float(value))
        if rc < 0:
            raise SslamError(rc, lib.sslam_last_error().decode())

    def num_edges(self) -> int:
        return int(self._lib.sslam_graph_num_edges(self._lib.sslam_slam_graph(self._h)))

    def graph_vertex(self, vid: int, n: int = 3) -> np.ndarray:
        out = np.zeros(7)
        g = self._lib.sslam_slam_graph(self._h)
        rc = self._lib.sslam_graph_get_vertex(g, vid, out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc < 0:
            raise SslamError(rc, self._lib.sslam_last_error().decode())
        return out[:n]

    def find_matches(self, planes, robot_pose):
        """data_association::find_matches on the device (parity hook; no graph vertices are added)"""
        n = len(planes)
        arr = (Plane * max(n, 1))(*planes)
        out = (Landmark * max(n, 1))()
        rp = np.ascontiguousarray(robot_pose, np.float32).reshape(6)
        self._check(self._lib.sslam_slam_find_matches(self._h, C.cast(arr, C.c_void_p), n, rp.ctypes.data, C.cast(out, C.c_void_p)))
        return [out[k] for k in range(n)]
