"""Reference for the fitness-score tests: the arithmetic include/sslam.h states for sslam_seg_fitness_scores, restated in NumPy float32
(brute-force argmin over the full distance matrix; np.argmin returns the FIRST minimum, which is the lowest-index tie rule), the score
as math.fsum of the accepted distances, and InformationMatrixCalculator's weight() / information matrix in plain Python."""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
DEFAULT_INF = (20.0, 0.1, 5.0, 0.05, 0.2, 0.5)   # var_gain_a, min / max stddev_x, min / max stddev_q, fitness_score_thresh


def transform_f32(src, T):
    """x' = ((r00 x + r01 y) + r02 z) + tx in float32, R and t cast from double once"""
    T = np.asarray(T, np.float64).reshape(12)
    R, t = T[:9].astype(np.float32), T[9:].astype(np.float32)
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    out = np.empty_like(s)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t[r]
    assert out.dtype == np.float32
    return out


def nearest_f32(target, source, T):
    """(index, d2) per source point: d2 = (dx dx + dy dy) + dz dz in float32 with dx = x' - x_target, smallest d2, lowest index among
    equals; (-1, -1.0) for a non-finite source point or when no target is at a finite distance; non-finite targets are never chosen"""
    tg = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    sr = np.ascontiguousarray(source, np.float32).reshape(-1, 3)
    idx = np.full(len(sr), -1, np.int32)
    d2 = np.full(len(sr), -1.0, np.float32)
    if len(tg) == 0 or len(sr) == 0:
        return idx, d2
    q = transform_f32(sr, T)
    tfin, sfin = np.isfinite(tg).all(1), np.isfinite(sr).all(1)
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - tg[None, :, 0]
        dy = q[:, None, 1] - tg[None, :, 1]
        dz = q[:, None, 2] - tg[None, :, 2]
        D = (dx * dx + dy * dy) + dz * dz
    assert D.dtype == np.float32
    D[:, ~tfin] = np.inf
    D[~sfin, :] = np.inf
    D[np.isnan(D)] = np.inf
    arg = np.argmin(D, axis=1)
    dmin = D[np.arange(len(sr)), arg]
    ok = dmin < np.inf
    idx[ok] = arg[ok]
    d2[ok] = dmin[ok]
    return idx, d2


def score_of(d2, idx, max_range=None):
    """(score, used): the accepted distances are those of found neighbours with (double)d2 <= max_range (a bound on the SQUARED distance)"""
    mr = DBL_MAX if max_range is None else float(max_range)
    acc = [float(d) for d, i in zip(d2, idx) if i >= 0 and float(d) <= mr]
    return (math.fsum(acc) / len(acc) if acc else DBL_MAX), len(acc)


def fitness_ref(target, source, T, max_range=None):
    idx, d2 = nearest_f32(target, source, T)
    score, used = score_of(d2, idx, max_range)
    return score, used, idx, d2


def weight(a, max_x, min_y, max_y, x):
    """information_matrix_calculator.hpp:20-24"""
    y = (1.0 - math.exp(-a * x)) / (1.0 - math.exp(-a * max_x))
    return min_y + (max_y - min_y) * y


def information_ref(fitness, params=DEFAULT_INF):
    """information_matrix_calculator.cpp:39-50 with the variances as stddev * stddev and w rounded to float as upstream"""
    a, min_sx, max_sx, min_sq, max_sq, thresh = params
    w_x = float(np.float32(weight(a, thresh, min_sx * min_sx, max_sx * max_sx, fitness)))
    w_q = float(np.float32(weight(a, thresh, min_sq * min_sq, max_sq * max_sq, fitness)))
    return np.diag([1.0 / w_x] * 3 + [1.0 / w_q] * 3)


def skew_T(angle=0.7, axis=(0.3, -0.5, 0.8), t=(0.11, -0.07, 0.05)):
    """12 doubles (R row-major, then t): a rotation about a skew axis plus a translation"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    return np.concatenate([R.reshape(-1), np.asarray(t, np.float64)])


IDENTITY_T = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])


def qmat(q):
    """row-major rotation of a unit quaternion (x, y, z, w), operation for operation as the library's qmat (csrc/sslam_math.hpp)"""
    x, y, z, w = (float(v) for v in q)
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [1 - 2 * (yy + zz), 2 * (xy - wz), 2 * (xz + wy),
            2 * (xy + wz), 1 - 2 * (xx + zz), 2 * (yz - wx),
            2 * (xz - wy), 2 * (yz + wx), 1 - 2 * (xx + yy)]
