"""Reference computation for the position priors (hdl_graph_slam's EdgeSE3PriorXY / EdgeSE3PriorXYZ) -- test helper, not collected.

Semantics restated from hdl_graph_slam's g2o/edge_se3_priorxy.hpp / edge_se3_priorxyz.hpp:
    XYZ: e = t(X) - z (3),        XY: e = t(X)[:2] - z (2),        J = [R | 0] (XY: its top two rows)
with X <- X * exp(delta) (VertexSE3::oplus).  ``NpPriorGraph`` adds these terms to ``oracle.np_graph.NpGraph`` and orders the unknowns
the way g2o does for an arbitrary set of fixed poses: non-fixed vertices that own an edge, by id (poses 0..Np-1, then the landmarks).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle.np_graph import NpGraph, qmat, se3_error_jac, point_error_jac, plane_error_jac, pose_oplus, plane_oplus

SIGMA = 0.5   # GNSS-like position noise [m]


def make_priors(g, seed: int = 0, xyz_every: int = 25, xy_offset: int = 12):
    """Seeded GPS-like priors on a synth.make_graph graph: z = poses_true translation + N(0, SIGMA^2).  XYZ priors on every
    ``xyz_every``-th pose, XY priors on the poses ``xy_offset`` behind them, and a second (XY) prior on every other XYZ pose.
    Information: a random SPD matrix around I / SIGMA^2.  Returns a list of (pose, z, Omega) in the order they are added."""
    rng = np.random.default_rng(seed)
    Np = g.n_poses

    def info(d):
        Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        W = Q @ np.diag(rng.uniform(0.5, 1.5, d) / SIGMA ** 2) @ Q.T
        return 0.5 * (W + W.T)

    out = []
    for p in range(0, Np, xyz_every):
        out.append((p, g.poses_true[p, :3] + rng.normal(0, SIGMA, 3), info(3)))
        q = p + xy_offset
        if q < Np:
            out.append((q, g.poses_true[q, :2] + rng.normal(0, SIGMA, 2), info(2)))
        if (p // xyz_every) % 2 == 1:
            out.append((p, g.poses_true[p, :2] + rng.normal(0, SIGMA, 2), info(2)))
    return out


def add_priors(G, priors, pose_ids=None):
    """Add ``priors`` to a GraphSLAM through the public API; returns the edge ids."""
    ids = []
    for p, z, W in priors:
        v = int(p if pose_ids is None else pose_ids[p])
        ids.append(G.add_se3_prior_xyz_edge(v, z, W) if len(z) == 3 else G.add_se3_prior_xy_edge(v, z, W))
    return ids


def prior_error_jac(X, z):
    """error and Jacobian (d x 6) of one prior at pose X = [t, q]"""
    d = len(z)
    R = qmat(np.asarray(X[3:], np.float64))
    J = np.zeros((d, 6)); J[:, :3] = R[:d]
    return X[:d] - z, J


class NpPriorGraph(NpGraph):
    """NpGraph + position priors, with any set of fixed poses (default: the first, graph_slam.cpp:109-111)."""

    def __init__(self, g, priors, fixed=None):
        super().__init__(g)
        self.priors = list(priors)
        self.fixed = np.zeros(self.Np, bool)
        if fixed is None:
            self.fixed[0] = True
        else:
            self.fixed[list(fixed)] = True
        has_p = np.zeros(self.Np, bool); has_l = np.zeros(self.Nl, bool)
        has_p[g.odom_ij.ravel()] = True; has_p[g.lm_ij[:, 0]] = True; has_l[g.lm_ij[:, 1]] = True
        for p, _, _ in self.priors:
            has_p[p] = True
        self.poff = np.full(self.Np, -1, np.int64); self.loff = np.full(self.Nl, -1, np.int64)
        o = 0
        for i in range(self.Np):
            if has_p[i] and not self.fixed[i]:
                self.poff[i] = o; o += 6
        for l in range(self.Nl):
            if has_l[l]:
                self.loff[l] = o; o += 3
        self.dim = o

    def hessian_index(self):
        """g2o's hessian index of every vertex (poses, then landmarks), -1 for fixed / edge-less ones"""
        return np.concatenate([self.poff, self.loff]).tolist()

    def chi2(self, poses=None, lms=None):
        poses = self.poses if poses is None else poses
        c = super().chi2(poses, lms)
        for p, z, W in self.priors:
            e = poses[p, :len(z)] - z
            c += float(e @ W @ e)
        return c

    def build(self):
        g = self.g
        dim = self.dim
        H = np.zeros((dim, dim)); b = np.zeros(dim)

        def scatter(oa, ob, M):
            if oa >= 0 and ob >= 0:
                H[oa:oa + M.shape[0], ob:ob + M.shape[1]] += M

        i, j = g.odom_ij[:, 0], g.odom_ij[:, 1]
        e, Ji, Jj = se3_error_jac(self.poses[i], self.poses[j], g.odom_z)
        for k in range(len(i)):
            W = g.odom_info[k]
            oi, oj = self.poff[i[k]], self.poff[j[k]]
            scatter(oi, oi, Ji[k].T @ W @ Ji[k]); scatter(oj, oj, Jj[k].T @ W @ Jj[k])
            scatter(oi, oj, Ji[k].T @ W @ Jj[k]); scatter(oj, oi, Jj[k].T @ W @ Ji[k])
            if oi >= 0: b[oi:oi + 6] -= Ji[k].T @ W @ e[k]
            if oj >= 0: b[oj:oj + 6] -= Jj[k].T @ W @ e[k]
        p, l = g.lm_ij[:, 0], g.lm_ij[:, 1]
        fn = point_error_jac if self.kind == "point" else plane_error_jac
        e, Jp, Jl = fn(self.poses[p], self.lms[l], g.lm_z)
        for k in range(len(p)):
            W = g.lm_info[k]
            op, ol = self.poff[p[k]], self.loff[l[k]]
            scatter(op, op, Jp[k].T @ W @ Jp[k]); scatter(ol, ol, Jl[k].T @ W @ Jl[k])
            scatter(op, ol, Jp[k].T @ W @ Jl[k]); scatter(ol, op, Jl[k].T @ W @ Jp[k])
            if op >= 0: b[op:op + 6] -= Jp[k].T @ W @ e[k]
            if ol >= 0: b[ol:ol + 3] -= Jl[k].T @ W @ e[k]
        for pv, z, W in self.priors:
            o = self.poff[pv]
            if o < 0:
                continue
            e, J = prior_error_jac(self.poses[pv], z)
            H[o:o + 6, o:o + 6] += J.T @ W @ J
            b[o:o + 6] -= J.T @ W @ e
        return sp.csc_matrix(H), b

    def apply(self, dx, poses=None, lms=None):
        poses = (self.poses if poses is None else poses).copy()
        lms = (self.lms if lms is None else lms).copy()
        for i in range(self.Np):
            o = self.poff[i]
            if o >= 0:
                poses[i] = pose_oplus(poses[i], dx[o:o + 6])
        for l in range(self.Nl):
            o = self.loff[l]
            if o >= 0:
                lms[l] = lms[l] + dx[o:o + 3] if self.kind == "point" else plane_oplus(lms[l], dx[o:o + 3])
        return poses, lms

    def estimates(self):
        """[Np + Nl, 7] in the vertex order of GraphProblem.from_synth(g) (no interleave)"""
        out = np.zeros((self.Np + self.Nl, 7))
        out[:self.Np] = self.poses
        out[self.Np:, :self.lms.shape[1]] = self.lms
        return out
