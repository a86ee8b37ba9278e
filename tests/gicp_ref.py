"""Reference for the generalized-ICP tests: include/sslam.h's statements for sslam_seg_cloud_covariances and
sslam_seg_register_pairs_gicp, in NumPy.  The neighbours are a float32 restatement (bitwise the device's), everything after them is
float64: covariances through np.linalg.eigh, the step through np.linalg.solve.  Built on fitness_ref.nearest_f32 and the scenes of
registration_ref.py."""
import numpy as np

from fitness_ref import DBL_MAX, IDENTITY_T, nearest_f32
from registration_ref import ERR_NUMERIC, far_scene, scene, start_T

K_DEFAULT, EPS_DEFAULT = 20, 1e-3
GAP_MIN = 1e-2          # the covariance comparison leaves out points whose gap ratio (l1 - l0) / l2 is below this
SCENE_NAMES = ("small", "large", "mixed", "wall", "floor", "half_z", "far_half")


def load_scene(name):
    """(target, source, T_true, T0): the registration scenes by name; the far ones start from start_T(name), the others from the identity"""
    if name in ("half_z", "far_half"):
        tg, sr, Tt = far_scene(name)
        return tg, sr, Tt, start_T(name)
    tg, sr, Tt = scene(name)
    return tg, sr, Tt, IDENTITY_T.copy()


def knn_ref(cloud, k):
    """[n, k] int32: per point the k smallest (d2, index) among the finite points of the cloud, in that order, -1 padded; all -1 for
    a non-finite point.  d2 = (dx dx + dy dy) + dz dz in float32, dx = x_query - x_candidate."""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
    n = len(c)
    out = np.full((n, k), -1, np.int32)
    fin = np.isfinite(c).all(1)
    cand = np.nonzero(fin)[0]
    if len(cand) == 0:
        return out
    f = c[cand]
    with np.errstate(all="ignore"):
        for i in np.nonzero(fin)[0]:
            dx, dy, dz = c[i, 0] - f[:, 0], c[i, 1] - f[:, 1], c[i, 2] - f[:, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            order = np.lexsort((cand, d2))[:k]
            out[i, :len(order)] = cand[order]
    return out


def sym6(M):
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def mat6(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def cov_ref(cloud, k=K_DEFAULT, eps=EPS_DEFAULT):
    """(cov [n, 6], gap [n], m [n]): the regularised covariances U diag(eps, 1, 1) U^T by np.linalg.eigh, the gap ratio
    (l1 - l0) / l2 of the raw covariance (inf where none was decomposed), the neighbours used"""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
    knn = knn_ref(c, k)
    n = len(c)
    cov = np.zeros((n, 6))
    gap = np.full(n, np.inf)
    m = (knn >= 0).sum(1)
    c64 = c.astype(np.float64)
    for i in range(n):
        if not np.isfinite(c[i]).all():
            continue
        if m[i] < 3:
            cov[i] = sym6(np.eye(3))
            continue
        q = c64[knn[i, :m[i]]]
        mean = np.cumsum(q, 0)[-1] / m[i]           # the sum in neighbour order
        d = q - mean
        C = np.cumsum(d[:, :, None] * d[:, None, :], 0)[-1] / m[i]
        lam, U = np.linalg.eigh(C)
        gap[i] = (lam[1] - lam[0]) / lam[2] if lam[2] > 0 else 0.0
        cov[i] = sym6(U @ np.diag([eps, 1.0, 1.0]) @ U.T)
    return cov, gap, m


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def exp_so3(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    K = skew(w)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def quat_of_rotation(R):
    """(x, y, z, w), the largest-pivot branch of INTEGRATION.md section 2, normalised"""
    R = np.asarray(R).reshape(9)
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = 2 * np.sqrt(1 + tr); q = [(R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s, s / 4]
    elif R[0] > R[4] and R[0] > R[8]:
        s = 2 * np.sqrt(1 + R[0] - R[4] - R[8]); q = [s / 4, (R[1] + R[3]) / s, (R[2] + R[6]) / s, (R[7] - R[5]) / s]
    elif R[4] > R[8]:
        s = 2 * np.sqrt(1 + R[4] - R[0] - R[8]); q = [(R[1] + R[3]) / s, s / 4, (R[5] + R[7]) / s, (R[2] - R[6]) / s]
    else:
        s = 2 * np.sqrt(1 + R[8] - R[0] - R[4]); q = [(R[2] + R[6]) / s, (R[5] + R[7]) / s, s / 4, (R[3] - R[1]) / s]
    q = np.array(q)
    return q / np.linalg.norm(q)


def rot_of_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def accepted(target, source, T, max_corr2=None):
    """(source indices, their target indices) of the accepted correspondences at T: the fitness pass and (double)d2 <= max_corr2"""
    idx, d2 = nearest_f32(target, source, T)
    mr = DBL_MAX if max_corr2 is None else float(max_corr2)
    acc = (idx >= 0) & (d2.astype(np.float64) <= mr)
    return np.nonzero(acc)[0], idx[acc]


def gicp_step_ref(target, source, Ct, Cs, T, max_corr2=None):
    """one iteration from T: (T_new as 12 doubles, accepted correspondences, cond2(H), |delta|); T_new is None where the library
    reports SSLAM_ERR_NUMERIC (fewer than 3 accepted, H not positive definite, a non-finite sum)"""
    tg = np.ascontiguousarray(target, np.float32).reshape(-1, 3).astype(np.float64)
    sr = np.ascontiguousarray(source, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(12)
    R, t = T[:9].reshape(3, 3), T[9:]
    si, ti = accepted(target, source, T, max_corr2)
    n = len(si)
    if n < 3:
        return None, n, np.inf, 0.0
    H, b = np.zeros((6, 6)), np.zeros(6)
    for i, j in zip(si, ti):
        x = R @ sr[i] + t
        r = tg[j] - x
        M = np.linalg.inv(mat6(Ct[j]) + R @ mat6(Cs[i]) @ R.T)
        J = np.hstack([skew(x), -np.eye(3)])
        H += J.T @ M @ J
        b += J.T @ M @ r
    if not (np.isfinite(H).all() and np.isfinite(b).all()):
        return None, n, np.inf, 0.0
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None, n, np.inf, 0.0
    delta = np.linalg.solve(H, -b)
    E = exp_so3(delta[:3])
    Rn = rot_of_quat(quat_of_rotation(E @ R))
    tn = E @ t + delta[3:]
    return np.concatenate([Rn.reshape(-1), tn]), n, float(np.linalg.cond(H)), float(np.linalg.norm(delta))


def gicp_ref(target, source, Ct, Cs, T0=None, max_corr2=None, max_iterations=50, epsilon=0.0, trace=None):
    """(T, iterations, converged, status) under the rules of sslam_seg_register_pairs_gicp; `trace`, a list, collects (cond2(H), |delta|,
    accepted, largest entry change) of every step"""
    T = np.array(IDENTITY_T if T0 is None else T0, np.float64).reshape(12)
    iterations, converged, status = 0, 0, 0
    while iterations < max_iterations:
        Tn, n, cond, nd = gicp_step_ref(target, source, Ct, Cs, T, max_corr2)
        if Tn is None:
            status = ERR_NUMERIC
            break
        moved = np.abs(Tn - T).max()
        if trace is not None:
            trace.append((cond, nd, n, moved))
        T = Tn
        iterations += 1
        if moved <= epsilon:
            converged = 1
            break
    return T, iterations, converged, status

