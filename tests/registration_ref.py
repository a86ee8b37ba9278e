"""Reference for the scan-matching tests: one iteration of nearest-neighbour ICP as include/sslam.h states it for
sslam_seg_register_pairs, in NumPy.  The correspondences are the float32 search of tests/fitness_ref.py (bitwise the device's); the
update is the centred two-pass Kabsch solution in float64 (np.linalg.svd with the determinant correction), which is the closed form of
pcl::TransformationEstimationSVD solved for the absolute transform.  icp_ref iterates it with the library's convergence and status
rules; make_scene builds the clouds the tests register."""
import numpy as np

from fitness_ref import DBL_MAX, IDENTITY_T, nearest_f32

ERR_NUMERIC = -4


def correspondences(target, source, T, max_corr2=None):
    """(p, q, accepted mask): the original source points and their nearest targets, widened to float64, of the accepted source points"""
    tg = np.ascontiguousarray(target, np.float32).reshape(-1, 3)
    sr = np.ascontiguousarray(source, np.float32).reshape(-1, 3)
    idx, d2 = nearest_f32(tg, sr, T)
    mr = DBL_MAX if max_corr2 is None else float(max_corr2)
    acc = (idx >= 0) & (d2.astype(np.float64) <= mr)
    return sr[acc].astype(np.float64), tg[idx[acc]].astype(np.float64), acc


def kabsch(p, q, correct=True):
    """the rigid (R, t) minimising sum |R p + t - q|^2: centre both sets, SVD of the cross-covariance, det correction"""
    pm, qm = p.mean(0), q.mean(0)
    H = (p - pm).T @ (q - qm)
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.eye(3)
    if correct and np.linalg.det(V @ U.T) < 0:
        D[2, 2] = -1.0
    R = V @ D @ U.T
    return R, qm - R @ pm, S


def step_ref(target, source, T, max_corr2=None):
    """one iteration from T: (T_new as 12 doubles, number of accepted correspondences); T_new is None with fewer than 3"""
    p, q, acc = correspondences(target, source, T, max_corr2)
    if len(p) < 3:
        return None, len(p)
    R, t, _ = kabsch(p, q)
    return np.concatenate([R.reshape(-1), t]), len(p)


def icp_ref(target, source, T0=None, max_corr2=None, max_iterations=50, epsilon=0.0):
    """(T, iterations, converged, status) under the rules of sslam_seg_register_pairs"""
    T = np.array(IDENTITY_T if T0 is None else T0, np.float64).reshape(12)
    iterations, converged, status = 0, 0, 0
    while iterations < max_iterations:
        Tn, _ = step_ref(target, source, T, max_corr2)
        if Tn is None:
            status = ERR_NUMERIC
            break
        done = np.abs(Tn - T).max() <= epsilon
        T = Tn
        iterations += 1
        if done:
            converged = 1
            break
    return T, iterations, converged, status


def motion_T(angle=0.05, axis=(0.2, -0.3, 0.93), t=(0.07, -0.06, 0.04)):
    """12 doubles of a small rigid motion: about 0.05 rad and 0.1 m by default"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([R.reshape(-1), np.asarray(t, np.float64)])


def apply_inverse(T, pts):
    """R^T (x - t): where a point of the target frame lies in the source frame"""
    R, t = np.asarray(T[:9]).reshape(3, 3), np.asarray(T[9:])
    return (pts - t) @ R


# the room: (origin, edge u, edge v) of every rectangle; a floor, two walls and the top and two sides of a box
_RECTS = [((0, 0, 0), (2, 0, 0), (0, 1.5, 0)),
          ((0, 0, 0), (0, 1.5, 0), (0, 0, 1)),
          ((0, 0, 0), (2, 0, 0), (0, 0, 1)),
          ((0.75, 0.5, 0.25), (0.4, 0, 0), (0, 0.3, 0)),
          ((1.15, 0.5, 0), (0, 0.3, 0), (0, 0, 0.25)),
          ((0.75, 0.8, 0), (0.4, 0, 0), (0, 0, 0.25))]


def _sample(rng, n, rects):
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in rects])
    which = rng.choice(len(rects), n, p=area / area.sum())
    o = np.array([rects[k][0] for k in which], np.float64)
    u = np.array([rects[k][1] for k in which], np.float64)
    v = np.array([rects[k][2] for k in which], np.float64)
    return o + rng.random((n, 1)) * u + rng.random((n, 1)) * v


def make_scene(seed, n_target, n_source, noise=0.002, coplanar=None, T_true=None):
    """(target, source, T_true): two independent, permuted samplings of the room with `noise` m of Gaussian noise each, the source seen
    from a frame that T_true takes into the target's.  coplanar = 2 (the floor, z = 0) or 1 (a wall, y = 0): that rectangle alone, noise
    and motion inside its plane, the coordinate exactly 0 in both clouds -- the cross-covariance then has rank 2."""
    rng = np.random.default_rng(seed)
    if T_true is None:
        T_true = motion_T() if coplanar is None else motion_T(0.05, np.eye(3)[coplanar], np.array([0.07, -0.06, 0.05]) * (np.arange(3) != coplanar))
    rects = _RECTS if coplanar is None else ([_RECTS[0]] if coplanar == 2 else [_RECTS[2]])
    tg = _sample(rng, n_target, rects) + rng.normal(0.0, noise, (n_target, 3))
    sr = apply_inverse(T_true, _sample(rng, n_source, rects) + rng.normal(0.0, noise, (n_source, 3)))
    if coplanar is not None:
        tg[:, coplanar] = 0.0
        sr[:, coplanar] = 0.0
    tg, sr = tg[rng.permutation(n_target)], sr[rng.permutation(n_source)]
    return tg.astype(np.float32), sr.astype(np.float32), T_true


def pose_error(T, T_true):
    """(rotation angle in rad, translation distance) between two transforms"""
    R, Rt = np.asarray(T[:9]).reshape(3, 3), np.asarray(T_true[:9]).reshape(3, 3)
    c = np.clip((np.trace(R.T @ Rt) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.arccos(c)), float(np.linalg.norm(np.asarray(T[9:]) - np.asarray(T_true[9:])))


# the scenes of tests/test_registration_gpu.py, checked on the reference alone by tests/test_registration_cpu.py:
# name -> (seed, targets, sources, coplanar).  1500 sources span two query blocks of 1024 and six runs of 256, the last partial.
SCENES = {"large": (101, 1300, 1500, None), "small": (207, 257, 300, None), "mixed": (103, 257, 1500, None),
          "wall": (201, 257, 300, 1), "floor": (200, 257, 300, 2)}
COPLANAR = ("wall", "floor")
MAX_ITERATIONS = 50      # the cap the GPU tests pass; the reference reaches its fixed point well inside it
BOUNDED_MAX_CORR2 = 0.01  # the bounded-distance case: correspondences farther than 0.1 m are dropped


def scene(name):
    seed, nt, ns, coplanar = SCENES[name]
    return make_scene(seed, nt, ns, coplanar=coplanar)


# scenes far from the identity: what a loop closure hands the matcher when the robot comes back along its own track.
# name -> (seed, targets, sources, angle, axis, shift of both clouds on every axis).  The translation is FAR_T but for "far", which keeps
# the default small motion.  Registered from start_T(name), never from the identity.  The fixed point of ICP on 257 x 300 independently
# sampled points lies 0.01 to 0.05 rad and 1 to 13 cm from the truth, depending on the sample; the seeds are ones where it lies nearer to
# the truth than the start does (about every second one), which tests/test_registration_cpu.py asserts.
FAR_T = (0.4, -1.2, 0.3)
GENERAL_AXIS = (0.2, -0.3, 0.93)
FAR_SCENES = {"half_z": (301, 257, 300, np.pi, (0, 0, 1), 0.0), "half_x": (302, 257, 300, np.pi, (1, 0, 0), 0.0),
              "half_y": (313, 257, 300, np.pi, (0, 1, 0), 0.0), "half_g": (304, 257, 300, np.pi - 0.3, GENERAL_AXIS, 0.0),
              "wide": (305, 257, 300, 2.2, GENERAL_AXIS, 0.0), "far": (306, 257, 300, None, None, 30.0),
              "far_half": (307, 257, 300, np.pi, (0, 0, 1), 30.0), "half_large": (308, 1300, 1500, np.pi, (0, 0, 1), 0.0)}
HALF_TURNS = ("half_z", "half_x", "half_y", "half_g", "far_half", "half_large")      # the trace of their rotation is below 0
START_ANGLE, START_AXIS, START_T = 0.05, (0.5, 0.4, -0.77), (0.03, -0.04, 0.033)      # the perturbation of start_T: 0.05 rad, 6 cm


def compose_T(A, B):
    """12 doubles of x -> A(B(x))"""
    Ra, Rb = np.asarray(A[:9]).reshape(3, 3), np.asarray(B[:9]).reshape(3, 3)
    return np.concatenate([(Ra @ Rb).reshape(-1), Ra @ np.asarray(B[9:]) + np.asarray(A[9:])])


def shifted_T(T, shift):
    """T between two clouds after both were moved by `shift` on every axis: x + s -> R x + t + s"""
    s = np.full(3, float(shift))
    return np.concatenate([T[:9], T[9:] + s - np.asarray(T[:9]).reshape(3, 3) @ s])


def far_scene(name):
    """(target, source, T_true) of FAR_SCENES: make_scene's room under a large motion, both clouds moved by the shift before the
    rounding to float32"""
    seed, nt, ns, angle, axis, shift = FAR_SCENES[name]
    T = motion_T() if angle is None else motion_T(angle, axis, FAR_T)
    tg, sr, _ = make_scene(seed, nt, ns, T_true=T)
    if shift:
        tg, sr = (tg.astype(np.float64) + shift).astype(np.float32), (sr.astype(np.float64) + shift).astype(np.float32)
    return tg, sr, shifted_T(T, shift)


def far_pose_error(name, T):
    """pose_error against the scene's truth with the translation measured where the clouds are (at the shift, not at an origin 50 m from
    them, where it would be the rotation error times that lever arm)"""
    shift = FAR_SCENES[name][5]
    return pose_error(shifted_T(T, -shift), shifted_T(far_scene(name)[2], -shift))


def start_T(name):
    """the guess a far scene is registered from: the truth composed with a turn of 0.05 rad and a move of 6 cm of the source cloud about
    its own place (for the shifted scenes: about the shifted origin, not 50 m away from the cloud)"""
    shift = FAR_SCENES[name][5]
    return compose_T(far_scene(name)[2], shifted_T(motion_T(START_ANGLE, START_AXIS, START_T), shift))


def two_correspondences():
    """(target, source, max_corr2): two source points sit 1 mm from a target, the other 60 lie 10 m away: under the bound only 2 are accepted"""
    tg, sr, _ = scene("small")
    src = sr[:62] + np.float32(10.0)
    src[7] = tg[5] + np.float32(0.001)
    src[40] = tg[9] - np.float32(0.001)
    return tg, src.astype(np.float32), 0.01


def fast_pair():
    """(target, source): every other target point, shifted by about a centimetre -- far less than the spacing of the points, so the first
    pass already pairs every point with its original and the loop ends after two or three updates"""
    tg, _, _ = scene("small")
    return tg, (tg[::2] - np.array([0.01, -0.005, 0.0025], np.float32)).astype(np.float32)
