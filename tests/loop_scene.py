"""The scene and the replay of the loop-closure tests: a static room with unequal sides and one box inside, seen by analytic ray casting
from a trajectory that goes round the room twice, with an odometry that carries a constant yaw and scale bias.

Every odometry sample is a keyframe (the spacing is above keyframe_delta_trans) and brings a 48 x 36 organised cloud cast from the TRUE
pose, in the frame of that pose (x forward, y left, z up; camera_angle_deg 0), so the drift is in the odometry alone and a scan match of
two keyframes measures their true relative pose."""
import dataclasses
import math

import numpy as np

ROOM = (9.0, 6.0, 3.0)                                   # the room spans 0 .. ROOM on x, y, z
BOX = ((3.7, 2.4, 0.0), (5.3, 3.4, 1.5))                 # the box the trajectory goes round
WIDTH, HEIGHT = 48, 36
FOV_H, FOV_V = math.radians(110.0), math.radians(80.0)   # wide: two walls, the floor and the box are in view nearly everywhere
CENTRE, SEMI = (4.5, 3.0), (2.8, 1.7)                    # the ellipse of the trajectory
STEP = 0.55                                              # metres between samples: above keyframe_delta_trans = 0.5
LAPS = 2
YAW_BIAS, SCALE_BIAS = 0.004, 1.03                       # per sample: radians added to the yaw increment; factor on the distance
RUN_EVERY = 4                                            # a tick after every fourth sample: several new keyframes per tick
ODOM_STDDEV_X, ODOM_STDDEV_Q = 0.1, 0.01                 # const_stddev_x / _q of the replay: information 10 and 100 per odometry edge
# the loop parameters of the replay, where they leave sslam_loop_default_params: candidates within a metre (the drift of a lap stays under
# it), the three nearest; a loop every 2.5 m; a 0.3 m grid (a few hundred points per cloud); ICP run to 1e-4; a score threshold between
# the scores of right matches (the spacing of the grid's centroids on a surface, squared: below 0.03) and of wrong ones (above 0.09);
# loop edges weighted like a handful of odometry edges; gate and robust kernel off
LOOP_KW = dict(distance_thresh=1.0, distance_from_last_edge_thresh=2.5, epsilon=1e-4, max_candidates=3, voxel_leaf=0.3,
               fitness_score_thresh=0.04, robust_kernel=0, inf=(20.0, 0.05, 0.5, 0.02, 0.1, 0.5))


@dataclasses.dataclass
class Cloud:
    """what setPointCloudData / set_point_cloud take"""
    cloud: np.ndarray
    width: int
    height: int
    point_step: int
    row_step: int
    offsets: tuple

    def xyz(self):
        return self.cloud.view(np.float32).reshape(-1, 4)[:, :3]


@dataclasses.dataclass
class Event:
    stamp: tuple
    odom: np.ndarray          # t, q(x, y, z, w) of the biased odometry
    truth: np.ndarray         # x, y, z, yaw of the true pose
    cloud: Cloud
    run_after: bool


# The half-turn replay (path="out_and_back"): one lap, then the same lap backwards, heading along the direction of travel, seen by a
# panoramic sensor.  Every revisit then pairs two keyframes whose relative rotation is a half turn about the vertical.  A MOUNT is a fixed
# rotation C of the sensor on the robot (sensor coordinates -> robot coordinates): the pose of a sample becomes that of the sensor,
# q_yaw * q_C, and its cloud is in the sensor's frame, rows p @ C.  The relative pose of two samples is then conjugated, C^T R C: the half
# turn about the robot's z is one about the sensor axis that C maps onto z, so the three mounts put the pivot of the half-turn matrix on
# R[8], R[0] and R[4].
FOV_PANORAMA = 2 * math.pi * (WIDTH - 1) / WIDTH         # 48 columns all the way round, the first and the last not on top of each other
RETURN_OFFSET = 0.3                                      # of a STEP: the samples of the way back lie between those of the way out
MOUNTS = {"I": np.eye(3),
          "z->x": np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]),      # the sensor's x is the robot's z
          "z->y": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])}      # the sensor's y is the robot's z


def _rays(fov_h=FOV_H):
    az = np.linspace(0.5 * fov_h, -0.5 * fov_h, WIDTH)
    el = np.linspace(0.5 * FOV_V, -0.5 * FOV_V, HEIGHT)
    E, A = np.meshgrid(el, az, indexing="ij")
    return np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)


def _yaw_matrix(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _quaternion_of(C):
    """(x, y, z, w) of a rotation matrix, w >= 0; the mounts are quarter and third turns, w is far from 0"""
    w = 0.5 * math.sqrt(1.0 + C[0, 0] + C[1, 1] + C[2, 2])
    return np.array([(C[2, 1] - C[1, 2]) / (4 * w), (C[0, 2] - C[2, 0]) / (4 * w), (C[1, 0] - C[0, 1]) / (4 * w), w])


def cast(truth, fov_h=FOV_H, mount=None):
    """the organised cloud seen from the true pose (x, y, z, yaw): the nearest hit of every ray with the room's inside or the box's outside;
    with a mount, in the sensor's frame"""
    o = np.asarray(truth[:3], np.float64)
    d_local = _rays(fov_h)
    d = d_local @ _yaw_matrix(truth[3]).T
    with np.errstate(divide="ignore", invalid="ignore"):
        # the room from the inside: the far plane along each axis
        far = np.where(d > 0, (np.asarray(ROOM) - o) / d, np.where(d < 0, -o / d, np.inf))
        t = far.min(1)
        # the box from the outside: the slab method
        lo, hi = (np.asarray(BOX[0]) - o) / d, (np.asarray(BOX[1]) - o) / d
        tn, tf = np.minimum(lo, hi).max(1), np.maximum(lo, hi).min(1)
    hit = (tn <= tf) & (tn > 0)
    t = np.where(hit, np.minimum(t, tn), t)
    pts = np.zeros((len(t), 4), np.float32)
    xyz = d_local * t[:, None]
    pts[:, :3] = (xyz if mount is None else xyz @ np.asarray(mount, np.float64)).astype(np.float32)
    return Cloud(pts.view(np.uint8).reshape(-1).copy(), WIDTH, HEIGHT, 16, 16 * WIDTH, (0, 4, 8))


def _trajectory():
    """true poses (x, y, z, yaw) at arc-length steps of STEP along the ellipse, counter-clockwise, LAPS times round"""
    th = np.linspace(0.0, 2 * math.pi * LAPS, 40000 * LAPS)
    x, y = CENTRE[0] + SEMI[0] * np.cos(th), CENTRE[1] + SEMI[1] * np.sin(th)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    at = np.interp(np.arange(0.0, s[-1], STEP), s, th)
    # the tangent's heading, continuous over the laps, turned 0.7 rad towards the middle of the room: the box stays in view
    yaw = np.unwrap(np.arctan2(SEMI[1] * np.cos(at), -SEMI[0] * np.sin(at))) + 0.7
    return np.stack([CENTRE[0] + SEMI[0] * np.cos(at), CENTRE[1] + SEMI[1] * np.sin(at), 1.0 + 0.2 * np.sin(at), yaw], 1)


def _out_and_back():
    """true poses (x, y, z, yaw): one lap at arc-length steps of STEP, counter-clockwise, then the same lap backwards from where the way out
    ended, its samples RETURN_OFFSET of a step off those of the way out; the yaw is the direction of travel, continuous along each way,
    and the way back's is the way out's plus a half turn (the robot turns on the spot in between)"""
    th = np.linspace(-0.2 * math.pi, 2.2 * math.pi, 48000)
    x, y = CENTRE[0] + SEMI[0] * np.cos(th), CENTRE[1] + SEMI[1] * np.sin(th)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    s -= np.interp(0.0, th, s)                                                 # arc length 0 at th = 0
    lap = np.interp(2 * math.pi, th, s)
    out = np.arange(0.0, lap, STEP)
    back = out[::-1] - RETURN_OFFSET * STEP                                    # the last one lies just before the start of the way out
    at = np.interp(np.concatenate([out, back]), s, th)
    tangent = np.arctan2(SEMI[1] * np.cos(at), -SEMI[0] * np.sin(at))
    yaw = np.concatenate([np.unwrap(tangent[:len(out)]), np.unwrap(tangent[len(out):]) + math.pi])
    yaw[len(out):] += 2 * math.pi * np.round((yaw[len(out) - 1] - (yaw[len(out)] - math.pi)) / (2 * math.pi))   # the same branch at the turn
    return np.stack([CENTRE[0] + SEMI[0] * np.cos(at), CENTRE[1] + SEMI[1] * np.sin(at), 1.0 + 0.2 * np.sin(at), yaw], 1)


def make_events(n=None, path="laps", fov_h=FOV_H, mount=None):
    """the replay: a list of Event; the odometry starts at the true first pose and integrates the true increments with the two biases.
    path "laps" (LAPS times round, looking 0.7 rad inwards) or "out_and_back"; fov_h: the horizontal field of view of the ray table;
    mount: a rotation C of the sensor on the robot (see MOUNTS), None for none"""
    truth = {"laps": _trajectory, "out_and_back": _out_and_back}[path]()
    if n is not None:
        truth = truth[:n]
    q_mount = None if mount is None else _quaternion_of(np.asarray(mount, np.float64))
    events = []
    ox, oy, oz, oyaw = truth[0]
    for k, tr in enumerate(truth):
        if k:
            p = truth[k - 1]
            d = _yaw_matrix(p[3]).T @ (tr[:3] - p[:3])                 # the true step in the frame of the pose before
            step = _yaw_matrix(oyaw) @ (SCALE_BIAS * d)
            ox, oy, oz = ox + step[0], oy + step[1], oz + step[2]
            oyaw = oyaw + (tr[3] - p[3]) + YAW_BIAS
        odom = np.array([ox, oy, oz, 0.0, 0.0, math.sin(0.5 * oyaw), math.cos(0.5 * oyaw)])
        if q_mount is not None:                                                # q_yaw * q_C
            (cx, cy, cz, cw), sz, cwz = q_mount, odom[5], odom[6]
            odom[3:] = [cwz * cx - sz * cy, cwz * cy + sz * cx, cwz * cz + sz * cw, cwz * cw - sz * cz]
        events.append(Event((k // 10, (k % 10) * 100000000), odom, tr.copy(), cast(tr, fov_h, mount), (k + 1) % RUN_EVERY == 0))
    return events


def truth_T(a, b, mount=None):
    """12 doubles (R row-major, then t): the true pose b in the frame of the true pose a; with a mount, of the sensor at b in the frame of
    the sensor at a, C^T R C and C^T t"""
    Ra, Rb = _yaw_matrix(a[3]), _yaw_matrix(b[3])
    R, t = Ra.T @ Rb, Ra.T @ (np.asarray(b[:3]) - np.asarray(a[:3]))
    if mount is not None:
        C = np.asarray(mount, np.float64)
        R, t = C.T @ R @ C, C.T @ t
    return np.concatenate([R.reshape(-1), t])


def rms_position_error(est_xyz, truth_xyz):
    """root mean square distance of the keyframes from the truth, the first keyframe of both at the same place (it is fixed)"""
    e = np.asarray(est_xyz)[:, :3] - np.asarray(truth_xyz)[:, :3]
    return float(np.sqrt((e * e).sum(1).mean()))
