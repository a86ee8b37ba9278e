"""NumPy reference of the loop-closure gate (sslam_batch_gate): the dense inverse of the oracle's H, the error and the Jacobians of
oracle/np_graph.py, S = J Sigma J^T + Omega^-1 and d2 = e^T S^-1 e.  Shared by tests/test_gate_gpu.py and tools/gate_timing.py."""
import numpy as np
import scipy.sparse as sp

from oracle.np_graph import point_error_jac, pose_oplus, qconj, qmul, qrot, se3_error_jac

# the candidates of the tests: Omega as the generator's odometry edges carry it, Z = the current relative pose moved by DELTA
OMEGA6 = np.diag([150.0, 150.0, 150.0, 1e5, 1e5, 1e5])
OMEGA3 = np.diag([150.0, 150.0, 150.0])
DELTA = np.array([0.05, -0.03, 0.02, 0.01, -0.01, 0.02])
POSE_PAIRS = ((10, 30), (0, 39), (1, 2), (5, 38))   # indices into pose_ids; pose 0 is fixed, 1 and 2 are adjacent


def dense_inverse(gp):
    U, _ = gp.linearize()
    return np.linalg.inv((U + sp.triu(U, 1).T).toarray())


def sigma_block(gp, Hinv, vr, vc):
    """block (vr, vc) of H^-1, zeros for a fixed or edge-less vertex"""
    h, _ = gp.hessian_index()
    dr = 6 if gp.vtype[vr] == 0 else 3
    dc = 6 if gp.vtype[vc] == 0 else 3
    if h[vr] < 0 or h[vc] < 0:
        return np.zeros((dr, dc))
    return Hinv[h[vr]:h[vr] + dr, h[vc]:h[vc] + dc]


def relative_pose(Xi, Xj):
    """Xi^-1 Xj as [t, q(xyzw)]"""
    qi = qconj(Xi[3:])
    return np.concatenate([qrot(qi, Xj[:3] - Xi[:3]), qmul(qi, Xj[3:7])])


def perturbed(Z, delta=DELTA):
    """Z * fromVectorMQT(delta): a measurement that disagrees with the estimate by a known, small amount"""
    return pose_oplus(Z, np.asarray(delta, np.float64))


def error_jac(est, kind, vu, vv, z):
    """e, Ju, Jv of a candidate at the estimates est [nv, 7]"""
    if kind == "se3":
        return se3_error_jac(est[vu], est[vv], np.asarray(z, np.float64))
    return point_error_jac(est[vu], est[vv, :3], np.asarray(z, np.float64))


def assemble(e, Ju, Jv, Zuu, Zuv, Zvv, info):
    """S, d2 and cond(S) from the Jacobians and the blocks of H^-1"""
    S = Ju @ Zuu @ Ju.T + Ju @ Zuv @ Jv.T + Jv @ Zuv.T @ Ju.T + Jv @ Zvv @ Jv.T
    if info is not None:
        S = S + np.linalg.inv(np.asarray(info, np.float64))
    return S, float(e @ np.linalg.solve(S, e)), float(np.linalg.cond(S))


def gate_ref(gp, Hinv, kind, vu, vv, z, info):
    """(d2, e, S, cond(S)) of one candidate of the graph problem gp (estimates gp.est) against the dense inverse Hinv"""
    e, Ju, Jv = error_jac(gp.est, kind, vu, vv, z)
    S, d2, cond = assemble(e, Ju, Jv, sigma_block(gp, Hinv, vu, vu), sigma_block(gp, Hinv, vu, vv), sigma_block(gp, Hinv, vv, vv), info)
    return d2, e, S, cond


def pose_candidate(gp, g, a, b, info=OMEGA6):
    """the candidate EdgeSE3 between poses a and b (indices into pose_ids) of graph g"""
    vu, vv = int(gp.pose_ids[a]), int(gp.pose_ids[b])
    return (g, "se3", vu, vv, perturbed(relative_pose(gp.est[vu], gp.est[vv])), info)


def point_candidate(gp, g, a, l, info=OMEGA3):
    """the candidate EdgeSE3PointXYZ from pose a to landmark l: the predicted observation moved by the first three of DELTA"""
    vu, vv = int(gp.pose_ids[a]), int(gp.lm_ids[l])
    e0 = point_error_jac(gp.est[vu], gp.est[vv, :3], np.zeros(3), want_jac=False)
    return (g, "point", vu, vv, e0 + DELTA[:3], info)
