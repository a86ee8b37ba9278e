"""Host-side mirror of the scan-matching odometry of include/sslam.h (``sslam_odom_*``): hdl_graph_slam's prefiltering_nodelet and
scan_matching_odometry_nodelet.  Every frame is prefiltered and matched against the current keyframe cloud on the device; the pose that
comes back is what ``SemanticGraphSLAM.VIOCallback`` takes, so a run needs no VIO source.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import load_library
from .segmentation import GicpParams, PointCloudSegmentation

DOWNSAMPLE_NONE, DOWNSAMPLE_VOXELGRID = 0, 1                    # SSLAM_DOWNSAMPLE_*
OUTLIER_NONE, OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1, 2     # SSLAM_OUTLIER_*
REG_ICP, REG_GICP = 0, 1                                        # SSLAM_REG_*
_DOWNSAMPLE = {"NONE": DOWNSAMPLE_NONE, "VOXELGRID": DOWNSAMPLE_VOXELGRID}
_OUTLIER = {"NONE": OUTLIER_NONE, "STATISTICAL": OUTLIER_STATISTICAL, "RADIUS": OUTLIER_RADIUS}
_METHOD = {"ICP": REG_ICP, "GICP": REG_GICP, "FAST_GICP": REG_GICP}


class PrefilterParams(C.Structure):
    """``sslam_prefilter_params`` (include/sslam.h); ``sslam_prefilter_default_params`` fills it"""
    _fields_ = [("use_distance_filter", C.c_int32), ("distance_near", C.c_double), ("distance_far", C.c_double), ("downsample", C.c_int32),
                ("leaf", C.c_float), ("outlier", C.c_int32), ("mean_k", C.c_int32), ("stddev_mul", C.c_double), ("radius", C.c_double),
                ("min_neighbors", C.c_int32)]


class OdomParams(C.Structure):
    """``sslam_odom_params`` (include/sslam.h); ``sslam_odom_default_params`` fills it"""
    _fields_ = [("prefilter", PrefilterParams), ("method", C.c_int32), ("gicp", GicpParams), ("max_iterations", C.c_int32), ("epsilon", C.c_double),
                ("max_correspondence_distance", C.c_double), ("keyframe_delta_trans", C.c_double), ("keyframe_delta_angle", C.c_double),
                ("keyframe_delta_time", C.c_double), ("transform_thresholding", C.c_int32), ("max_acceptable_trans", C.c_double),
                ("max_acceptable_angle", C.c_double)]


class OdomStats(C.Structure):
    """``sslam_odom_stats`` (include/sslam.h)"""
    _fields_ = [("n_raw", C.c_int32), ("n_filtered", C.c_int32), ("matched", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("status", C.c_int32), ("used", C.c_int32), ("accepted", C.c_int32), ("new_keyframe", C.c_int32), ("keyframes", C.c_int32),
                ("covariance_passes", C.c_int64), ("fitness", C.c_double), ("T", C.c_double * 12), ("delta_trans", C.c_double),
                ("delta_angle", C.c_double), ("delta_time", C.c_double), ("prefilter_ms", C.c_double), ("covariance_ms", C.c_double),
                ("registration_ms", C.c_double), ("total_ms", C.c_double)]

    def __repr__(self):
        return (f"OdomStats(n_raw={self.n_raw}, n_filtered={self.n_filtered}, matched={self.matched}, iterations={self.iterations}, "
                f"status={self.status}, used={self.used}, fitness={self.fitness:.6g}, accepted={self.accepted}, new_keyframe={self.new_keyframe}, "
                f"keyframes={self.keyframes}, delta=({self.delta_trans:.4f}, {self.delta_angle:.4f}, {self.delta_time:.3f}), "
                f"ms=({self.prefilter_ms:.3f}, {self.covariance_ms:.3f}, {self.registration_ms:.3f}, {self.total_ms:.3f}))")


def default_prefilter_params() -> PrefilterParams:
    """distance filter 1 .. 100 m, VOXELGRID at leaf 0.1, STATISTICAL with 20 neighbours and multiplier 1 (radius 0.8 / 2 set for RADIUS)"""
    p = PrefilterParams()
    load_library().sslam_prefilter_default_params(C.byref(p))
    return p


def default_odom_params() -> OdomParams:
    """GICP (20, 1e-3), 64 iterations, epsilon 0.01, correspondences within 2.5 m, keyframes at 0.25 m / 0.15 / 1 s, thresholding off"""
    p = OdomParams()
    load_library().sslam_odom_default_params(C.byref(p))
    return p


def _set_prefilter(p: PrefilterParams, kw: dict) -> None:
    for name in [f[0] for f in PrefilterParams._fields_]:
        if name in kw:
            v = kw.pop(name)
            if name == "downsample" and isinstance(v, str):
                v = _DOWNSAMPLE[v.upper()]
            if name == "outlier" and isinstance(v, str):
                v = _OUTLIER[v.upper()]
            setattr(p, name, v)


def prefilter_params(**kw) -> PrefilterParams:
    """the defaults with the named fields replaced; ``downsample`` / ``outlier`` also by hdl's names ("VOXELGRID", "RADIUS", ...)"""
    p = default_prefilter_params()
    _set_prefilter(p, kw)
    if kw:
        raise TypeError(f"unknown prefilter parameters: {sorted(kw)}")
    return p


def odom_params(**kw) -> OdomParams:
    """the defaults with the named fields replaced: the fields of ``sslam_odom_params``, those of its prefilter by their own names, ``k`` and
    ``plane_epsilon`` of the generalized ICP; ``method`` also by hdl's registration_method names"""
    p = default_odom_params()
    _set_prefilter(p.prefilter, kw)
    for name in ("k", "plane_epsilon"):
        if name in kw:
            setattr(p.gicp, name, kw.pop(name))
    for name in [f[0] for f in OdomParams._fields_ if f[0] not in ("prefilter", "gicp")]:
        if name in kw:
            v = kw.pop(name)
            if name == "method" and isinstance(v, str):
                v = _METHOD[v.upper()]
            setattr(p, name, v)
    if kw:
        raise TypeError(f"unknown odometry parameters: {sorted(kw)}")
    return p


class ScanMatchingOdometry:
    """``sslam_odom``: ``push(cloud, stamp)`` returns the pose of the frame in the frame of the first one (12 doubles, R row-major then t) and
    the ``OdomStats`` of the call.  ``seg``: the frontend handle the work runs on (several odometries may share one).  ``params``: the
    keyword arguments of :func:`odom_params`."""

    def __init__(self, seg: PointCloudSegmentation, **params):
        self._lib = load_library()
        self._seg = seg                      # borrowed by the C handle: keep it alive
        self.params = odom_params(**params)
        self._h = self._lib.sslam_odom_create(seg._h, C.byref(self.params))
        if not self._h:
            from .graph_slam import SslamError
            raise SslamError(-1, self._lib.sslam_last_error().decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.sslam_odom_destroy(h)

    def _check(self, rc):
        if rc < 0:
            from .graph_slam import SslamError
            raise SslamError(rc, self._lib.sslam_last_error().decode())
        return rc

    def push(self, cloud, stamp=(0, 0)):
        """``cloud``: [n, 3] floats.  ``stamp``: (sec, nsec)."""
        pts = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        buf = pts if len(pts) else np.zeros((1, 3), np.float32)
        pose = np.zeros(12)
        st = OdomStats()
        self._check(self._lib.sslam_odom_push(self._h, buf.ctypes.data, len(pts), int(stamp[0]), int(stamp[1]), pose.ctypes.data, C.addressof(st)))
        return pose, st

    def reset(self) -> None:
        self._check(self._lib.sslam_odom_reset(self._h))

    def keyframe(self):
        """(filtered cloud [m, 3] float32, pose as 12 doubles) of the current keyframe; an empty cloud and None without one"""
        n = self._check(self._lib.sslam_odom_keyframe(self._h, None, 0, None))
        if n == 0:
            return np.zeros((0, 3), np.float32), None
        out = np.zeros((n, 3), np.float32)
        pose = np.zeros(12)
        self._check(self._lib.sslam_odom_keyframe(self._h, out.ctypes.data, n, pose.ctypes.data))
        return out, pose
