"""Reference for the odometry tests: include/sslam.h's statements for sslam_seg_radius_outlier_removal, sslam_seg_prefilter and
sslam_odom_push, in NumPy.

  * the radius count: a float32 restatement, integer for integer what the device counts;
  * the prefilter chain: oracle/np_filters.py stage by stage under the header's rules (what drops non-finite points, the skipped
    statistical stage), bit for bit what the device returns;
  * the decision rule of the odometry handle with the products in the header's order (plain Python floats: IEEE double, no fused
    multiply-add), so that a pose built from the device's own T repeats the device's pose bit for bit;
  * the matchers: registration_ref.icp_ref, and generalized ICP as gicp_ref.py states it -- the same neighbours (float32), covariances
    (np.linalg.eigh) and step (np.linalg.solve) -- evaluated for all points of a cloud at once: gicp_ref's own loops take a minute over
    the 45 frames of odom_scene.py, these a few seconds.  test_odometry_cpu.py holds one against the other.
"""
import math

import numpy as np

from fitness_ref import DBL_MAX, IDENTITY_T, nearest_f32
from gicp_ref import exp_so3, quat_of_rotation, rot_of_quat
from oracle import np_filters
from registration_ref import ERR_NUMERIC, icp_ref

F = np.float32
DOWNSAMPLE_NONE, DOWNSAMPLE_VOXELGRID = 0, 1
OUTLIER_NONE, OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1, 2
REG_ICP, REG_GICP = 0, 1
PREFILTER_DEFAULTS = dict(use_distance_filter=1, distance_near=1.0, distance_far=100.0, downsample=DOWNSAMPLE_VOXELGRID, leaf=0.1,
                          outlier=OUTLIER_STATISTICAL, mean_k=20, stddev_mul=1.0, radius=0.8, min_neighbors=2)
ODOM_DEFAULTS = dict(method=REG_GICP, k=20, plane_epsilon=1e-3, max_iterations=64, epsilon=0.01, max_correspondence_distance=2.5,
                     keyframe_delta_trans=0.25, keyframe_delta_angle=0.15, keyframe_delta_time=1.0, transform_thresholding=0,
                     max_acceptable_trans=1.0, max_acceptable_angle=1.0)


# ---- radius outlier removal ------------------------------------------------------------------------------------------------------------
def radius_counts(xyz, radius):
    """[n] int32: the OTHER finite points with d2 <= r2, d2 = (dx dx + dy dy) + dz dz in float32 with dx = x_query - x_candidate,
    r2 = (float)(radius * radius); -1 for a non-finite point"""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(p)
    out = np.full(n, -1, np.int32)
    fin = np.isfinite(p).all(1)
    q = p[fin]
    r2 = F(float(radius) * float(radius))
    cnt = np.zeros(len(q), np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(q), 512):
            blk = q[a:a + 512]
            dx = blk[:, None, 0] - q[None, :, 0]; dy = blk[:, None, 1] - q[None, :, 1]; dz = blk[:, None, 2] - q[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            cnt[a:a + 512] = (d2 <= r2).sum(1) - 1          # the point itself is at d2 = 0
    out[fin] = cnt
    return out


def radius_outlier_removal(xyz, radius=0.8, min_neighbors=2):
    """(ascending kept indices, counts)"""
    cnt = radius_counts(xyz, radius)
    return np.nonzero(cnt >= min_neighbors)[0].astype(np.int32), cnt


# ---- the prefilter chain -----------------------------------------------------------------------------------------------------------------
def prefilter(xyz, **kw):
    """(cloud [m, 3] float32, counts [3]) under the rules of sslam_seg_prefilter"""
    P = dict(PREFILTER_DEFAULTS); P.update(kw)
    cur = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    clean = False
    counts = np.zeros(3, np.int32)
    if P["use_distance_filter"] and len(cur):
        cur = cur[np_filters.distance_filter(cur, P["distance_near"], P["distance_far"])]; clean = True
    counts[0] = len(cur)
    if P["downsample"] == DOWNSAMPLE_VOXELGRID and len(cur):
        cur = np_filters.voxel_grid(cur, P["leaf"])[0]; clean = True
    counts[1] = len(cur)
    if not clean and len(cur):
        cur = cur[np.isfinite(cur).all(1)]
    if P["outlier"] == OUTLIER_STATISTICAL and len(cur) >= P["mean_k"] + 1:
        cur = cur[np_filters.statistical_outlier_removal(cur, P["mean_k"], P["stddev_mul"])[0]]
    elif P["outlier"] == OUTLIER_RADIUS and len(cur):
        cur = cur[radius_outlier_removal(cur, P["radius"], P["min_neighbors"])[0]]
    counts[2] = len(cur)
    return np.ascontiguousarray(cur, F), counts


# ---- 3 x 4 transforms as 12 doubles, the header's order of operations -------------------------------------------------------------------
def mul(A, B):
    A = [float(v) for v in A]; B = [float(v) for v in B]
    O = [0.0] * 12
    for i in range(3):
        for j in range(3):
            O[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j]
        O[9 + i] = ((A[3 * i] * B[9] + A[3 * i + 1] * B[10]) + A[3 * i + 2] * B[11]) + A[9 + i]
    return np.array(O)


def inverse(A):
    A = [float(v) for v in A]
    O = [0.0] * 12
    for i in range(3):
        for j in range(3):
            O[3 * i + j] = A[3 * j + i]
        O[9 + i] = -((A[i] * A[9] + A[3 + i] * A[10]) + A[6 + i] * A[11])
    return np.array(O)


def trans(T):
    t = [float(v) for v in T[9:12]]
    return math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])


def angle(T):
    """upstream's acos(Quaternionf(R).w()): HALF the rotation angle; w by the largest-pivot branch (csrc/sslam_math.hpp quat_of_rotation)"""
    R = [float(v) for v in T[:9]]
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = 2 * math.sqrt(1 + tr); w = s / 4; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s
    elif R[0] > R[4] and R[0] > R[8]:
        s = 2 * math.sqrt(1 + R[0] - R[4] - R[8]); x = s / 4; w = (R[7] - R[5]) / s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s
    elif R[4] > R[8]:
        s = 2 * math.sqrt(1 + R[4] - R[0] - R[8]); y = s / 4; w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; z = (R[5] + R[7]) / s
    else:
        s = 2 * math.sqrt(1 + R[8] - R[0] - R[4]); z = s / 4; w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s
    n = math.sqrt(x * x + y * y + z * z + w * w)
    return math.acos(min(1.0, abs(w / n)))


def delta_time(stamp, key_stamp):
    return (float(stamp[0]) - float(key_stamp[0])) + 1e-9 * (float(stamp[1]) - float(key_stamp[1]))


# ---- generalized ICP, a cloud at a time ---------------------------------------------------------------------------------------------------
def knn(cloud, k):
    """[n, k] indices: per point of a cloud of FINITE points its k smallest (d2, index), d2 in float32 as gicp_ref.knn_ref forms it"""
    c = np.ascontiguousarray(cloud, F).reshape(-1, 3)
    dx = c[:, None, 0] - c[None, :, 0]; dy = c[:, None, 1] - c[None, :, 1]; dz = c[:, None, 2] - c[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def covariances(cloud, k=20, eps=1e-3):
    """[n, 6]: gicp_ref.cov_ref for a cloud of at least 3 finite points"""
    c = np.ascontiguousarray(cloud, F).reshape(-1, 3)
    assert len(c) >= 3 and np.isfinite(c).all()
    q = c.astype(np.float64)[knn(c, k)]                        # [n, m, 3]
    d = q - q.mean(1, keepdims=True)
    C = np.einsum("nmi,nmj->nij", d, d) / q.shape[1]
    _, U = np.linalg.eigh(C)
    M = np.einsum("nik,k,njk->nij", U, np.array([eps, 1.0, 1.0]), U)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)


def _mats(c6):
    c6 = np.asarray(c6)
    M = np.empty((len(c6), 3, 3))
    M[:, 0, 0] = c6[:, 0]; M[:, 0, 1] = M[:, 1, 0] = c6[:, 1]; M[:, 0, 2] = M[:, 2, 0] = c6[:, 2]
    M[:, 1, 1] = c6[:, 3]; M[:, 1, 2] = M[:, 2, 1] = c6[:, 4]; M[:, 2, 2] = c6[:, 5]
    return M


def gicp_step(target, source, Ct, Cs, T, max_corr2=None):
    """gicp_ref.gicp_step_ref's first two results: (T_new or None, accepted correspondences)"""
    tg = np.ascontiguousarray(target, F).reshape(-1, 3)
    sr = np.ascontiguousarray(source, F).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(12)
    R, t = T[:9].reshape(3, 3), T[9:]
    idx, d2 = nearest_f32(tg, sr, T)
    acc = (idx >= 0) & (d2.astype(np.float64) <= (DBL_MAX if max_corr2 is None else float(max_corr2)))
    si, ti = np.nonzero(acc)[0], idx[acc]
    if len(si) < 3:
        return None, len(si)
    x = sr[si].astype(np.float64) @ R.T + t
    r = tg[ti].astype(np.float64) - x
    M = np.linalg.inv(_mats(np.asarray(Ct)[ti]) + R @ _mats(np.asarray(Cs)[si]) @ R.T)
    J = np.zeros((len(si), 3, 6))
    J[:, 0, 1] = -x[:, 2]; J[:, 0, 2] = x[:, 1]; J[:, 1, 0] = x[:, 2]; J[:, 1, 2] = -x[:, 0]; J[:, 2, 0] = -x[:, 1]; J[:, 2, 1] = x[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    MJ = M @ J
    H = np.einsum("nia,nib->ab", J, MJ)
    b = np.einsum("nia,ni->a", MJ, r)
    if not (np.isfinite(H).all() and np.isfinite(b).all()):
        return None, len(si)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None, len(si)
    delta = np.linalg.solve(H, -b)
    E = exp_so3(delta[:3])
    Rn = rot_of_quat(quat_of_rotation(E @ R))
    return np.concatenate([Rn.reshape(-1), E @ t + delta[3:]]), len(si)


def gicp(target, source, Ct, Cs, T0=None, max_corr2=None, max_iterations=50, epsilon=0.0):
    """(T, iterations, converged, status) under the rules of sslam_seg_register_pairs_gicp (gicp_ref.gicp_ref's loop)"""
    T = np.array(IDENTITY_T if T0 is None else T0, np.float64).reshape(12)
    iterations, converged, status = 0, 0, 0
    while iterations < max_iterations:
        Tn, _ = gicp_step(target, source, Ct, Cs, T, max_corr2)
        if Tn is None:
            status = ERR_NUMERIC
            break
        moved = np.abs(Tn - T).max()
        T = Tn
        iterations += 1
        if moved <= epsilon:
            converged = 1
            break
    return T, iterations, converged, status


# ---- the odometry handle ------------------------------------------------------------------------------------------------------------------
class Odometry:
    """sslam_odom_push's rule.  `match(key, frame, T0) -> (T, iterations, converged, status)` matches two entries of the kind `prepare`
    returns; the default pair is this file's prefilter + covariances and gicp / icp_ref.  push returns (pose, record) with the record's
    keys named as the fields of sslam_odom_stats."""

    def __init__(self, prepare=None, match=None, prefilter_kw=None, **kw):
        self.P = dict(ODOM_DEFAULTS); self.P.update(kw)
        self.prefilter_kw = dict(prefilter_kw or {})
        self._prepare = prepare or self._default_prepare
        self._match = match or self._default_match
        self.reset()

    def reset(self):
        self.key = None
        self.key_pose = IDENTITY_T.copy(); self.prev = IDENTITY_T.copy()
        self.key_stamp = (0, 0)
        self.keyframes = 0

    def _default_prepare(self, cloud):
        f = prefilter(cloud, **self.prefilter_kw)[0]
        cov = covariances(f, self.P["k"], self.P["plane_epsilon"]) if self.P["method"] == REG_GICP and len(f) >= 3 else None
        return f, cov

    def _default_match(self, key, frame, T0):
        mc2 = self.P["max_correspondence_distance"] * self.P["max_correspondence_distance"]
        if self.P["method"] == REG_GICP:
            if len(frame[0]) < 3 or len(key[0]) < 3:
                return np.array(T0), 0, 0, ERR_NUMERIC
            return gicp(key[0], frame[0], key[1], frame[1], T0, mc2, self.P["max_iterations"], self.P["epsilon"])
        return icp_ref(key[0], frame[0], T0, mc2, self.P["max_iterations"], self.P["epsilon"])

    def push(self, cloud, stamp=(0, 0)):
        P = self.P
        frame = self._prepare(cloud)
        rec = dict(matched=0, iterations=0, converged=0, status=0, accepted=0, new_keyframe=0, delta_trans=0.0, delta_angle=0.0, delta_time=0.0,
                   thresholding=None)
        promote = False
        if self.key is None:
            if len(frame[0]) == 0:
                raise ValueError("the first frame is empty after the prefilter")
            pose, T = IDENTITY_T.copy(), IDENTITY_T.copy()
            rec["accepted"] = 1
            promote = True
        else:
            Tm, it, conv, status = self._match(self.key, frame, self.prev.copy())
            rec.update(matched=1, iterations=it, converged=conv, status=status)
            ok = status == 0
            if ok and P["transform_thresholding"]:
                d = mul(inverse(self.prev), Tm)
                rec["thresholding"] = (trans(d), angle(d))
                if trans(d) > P["max_acceptable_trans"] or angle(d) > P["max_acceptable_angle"]:
                    ok = False
            if not ok:
                T = self.prev.copy()
                pose = mul(self.key_pose, self.prev)
            else:
                T = np.array(Tm, np.float64)
                pose = mul(self.key_pose, T)
                rec.update(accepted=1, delta_trans=trans(T), delta_angle=angle(T), delta_time=delta_time(stamp, self.key_stamp))
                promote = (rec["delta_trans"] > P["keyframe_delta_trans"] or rec["delta_angle"] > P["keyframe_delta_angle"]
                           or rec["delta_time"] > P["keyframe_delta_time"])
        if rec["accepted"]:
            self.prev = T.copy()
        if promote:
            self.key, self.key_pose, self.key_stamp = frame, pose.copy(), (int(stamp[0]), int(stamp[1]))
            self.prev = IDENTITY_T.copy()
            self.keyframes += 1
            rec["new_keyframe"] = 1
        rec["keyframes"] = self.keyframes
        rec["T"] = T.copy()
        return pose, rec


# ---- the runs the tests share ---------------------------------------------------------------------------------------------------------------
RUN_PREFILTER = dict(use_distance_filter=0, outlier=OUTLIER_NONE)     # the leaf-0.1 voxel grid alone: 1 350 - 1 600 points per frame
RUN_KW = dict(epsilon=1e-4)                                            # hdl's thresholds, correspondences within 2.5 m, at most 64 iterations
RADIUS_KW = dict(radius=0.5, min_neighbors=6)                          # a radius stage that removes some points of these leaf-0.1 clouds
GOLDEN = "odom_ref45.npz"                                              # tests/golden: reference_run(odom_scene.frames()[1]) as recorded
RUN_FIELDS = ("new_keyframe", "accepted", "status", "iterations", "delta_trans", "delta_angle", "delta_time")


def reference_run(clouds, stamps, **kw):
    """the clouds through Odometry with RUN_PREFILTER and RUN_KW (+ kw): a dict of arrays, `pose` and `T` [n, 12] and RUN_FIELDS [n]"""
    P = dict(RUN_KW); P.update(kw)
    o = Odometry(prefilter_kw=RUN_PREFILTER, **P)
    out = {k: [] for k in ("pose", "T") + RUN_FIELDS}
    for c, s in zip(clouds, stamps):
        pose, rec = o.push(c, s)
        out["pose"].append(pose)
        for k in ("T",) + RUN_FIELDS:
            out[k].append(rec[k])
    return {k: np.array(v) for k, v in out.items()}


if __name__ == "__main__":      # python tests/odom_ref.py: records the golden run again
    import os
    import odom_scene
    _, cl = odom_scene.frames()
    run = reference_run(cl, [odom_scene.stamp(k) for k in range(len(cl))])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN), **run)
    print({k: v.shape for k, v in run.items()})
