"""The scene of the odometry tests: the room of loop_scene.py seen from a DENSE trajectory -- 0.12 m of arc between frames along the same
ellipse at z = 1.0, looking 0.7 rad inwards of the direction of travel, stamps 0.1 s apart -- so that consecutive frames overlap almost
entirely and a keyframe (0.25 m by hdl's default) is taken every third frame.  Clouds are cast from the TRUE poses, in the frame of the
pose: a scan match of a frame against a keyframe measures their true relative pose, loop_scene.truth_T."""
import math

import numpy as np

import loop_scene

ARC_STEP = 0.12           # metres of arc between frames
STAMP_STEP_NS = 100000000  # 0.1 s
N_FRAMES = 45             # 5.28 m of arc


def trajectory(n=N_FRAMES):
    """true poses (x, y, z, yaw) at arc-length steps of ARC_STEP along the ellipse, counter-clockwise from its +x end"""
    th = np.linspace(0.0, 2 * math.pi, 80000)
    (cx, cy), (sx, sy) = loop_scene.CENTRE, loop_scene.SEMI
    x, y = cx + sx * np.cos(th), cy + sy * np.sin(th)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    at = np.interp(np.arange(n) * ARC_STEP, s, th)
    yaw = np.unwrap(np.arctan2(sy * np.cos(at), -sx * np.sin(at))) + 0.7
    return np.stack([cx + sx * np.cos(at), cy + sy * np.sin(at), np.full(n, 1.0), yaw], 1)


def stamp(k):
    """(sec, nsec) of frame k"""
    ns = k * STAMP_STEP_NS
    return ns // 1000000000, ns % 1000000000


_CACHE = {}


def frames(n=N_FRAMES):
    """(truth [n, 4], clouds: n arrays [48 * 36, 3] float32), cast once per process"""
    if n not in _CACHE:
        tr = trajectory(n)
        _CACHE[n] = (tr, [np.ascontiguousarray(loop_scene.cast(t).xyz()).copy() for t in tr])
    return _CACHE[n]


def holed_frame(k=0):
    """frame k with 5 % of its rows not finite: every 20th row has a NaN, a +inf or a -inf in one coordinate"""
    c = frames()[1][k].copy()
    bad = np.arange(7, len(c), 20)
    c[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[(bad // 20) % 3]
    return c


def truth_T(truth, k):
    """12 doubles: the true pose of frame k in the frame of frame 0 -- what the odometry's pose estimates"""
    return loop_scene.truth_T(truth[0], truth[k])


def pose_error(T, T_true):
    """(translation distance, rotation angle in rad) between two transforms"""
    R, Rt = np.asarray(T[:9]).reshape(3, 3), np.asarray(T_true[:9]).reshape(3, 3)
    c = min(1.0, max(-1.0, (np.trace(R.T @ Rt) - 1.0) / 2.0))
    return float(np.linalg.norm(np.asarray(T[9:]) - np.asarray(T_true[9:]))), float(math.acos(c))
