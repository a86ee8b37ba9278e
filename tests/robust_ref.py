"""Reference computation for the per-edge robust kernels -- test helper, not collected.

The table of include/sslam.h (g2o's robust_kernel_impl.cpp, the kernels whose formulas are the same in every g2o release), with
e2 = e^T Omega e and d = delta:  H += J^T (rho1 Omega) J,  b -= J^T (rho1 Omega) e,  the edge's chi2 term is rho0.
``NpRobustGraph`` puts a kernel on any edge of ``prior_ref.NpPriorGraph``; ``NpGraph.optimize`` then is the LM mirror.
"""
from __future__ import annotations

import copy

import numpy as np

from oracle.np_graph import se3_error_jac, point_error_jac, plane_error_jac
from prior_ref import NpPriorGraph

NONE, HUBER, PSEUDOHUBER, CAUCHY, WELSCH, FAIR, SATURATED, DCS = range(8)
NAMES = ["NONE", "Huber", "PseudoHuber", "Cauchy", "Welsch", "Fair", "Saturated", "DCS"]


def rho(kind, d, e2):
    """(rho0, rho1) of kernel ``kind`` (scalar or array, broadcast against e2) with width d at e2"""
    e2 = np.asarray(e2, np.float64)
    kind = np.broadcast_to(np.asarray(kind), e2.shape)
    d = np.broadcast_to(np.asarray(d, np.float64), e2.shape)
    r0 = e2.copy(); r1 = np.ones_like(e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.where(kind == NONE, 1.0, d * d)
        s = np.sqrt(e2)
        m = (kind == HUBER) & (e2 > d2)
        r0 = np.where(m, 2 * d * s - d2, r0); r1 = np.where(m, d / s, r1)
        m = kind == PSEUDOHUBER
        a = np.sqrt(1 + e2 / d2)
        r0 = np.where(m, 2 * d2 * (a - 1), r0); r1 = np.where(m, 1 / a, r1)
        m = kind == CAUCHY
        a = 1 + e2 / d2
        r0 = np.where(m, d2 * np.log(a), r0); r1 = np.where(m, 1 / a, r1)
        m = kind == WELSCH
        a = np.exp(-e2 / d2)
        r0 = np.where(m, d2 * (1 - a), r0); r1 = np.where(m, a, r1)
        m = kind == FAIR
        a = s / np.where(m, d, 1.0)
        r0 = np.where(m, 2 * d2 * (a - np.log1p(a)), r0); r1 = np.where(m, 1 / (1 + a), r1)
        m = (kind == SATURATED) & (e2 > d2)
        r0 = np.where(m, d2, r0); r1 = np.where(m, 0.0, r1)
        m = kind == DCS
        sc = np.minimum(1.0, (2 * d / (d + e2)) ** 2)
        r0 = np.where(m, e2 * sc, r0); r1 = np.where(m, sc, r1)
    return r0, r1


class NpRobustGraph(NpPriorGraph):
    """NpPriorGraph + a (kind, delta) per edge.  Edge ids as GraphProblem.from_synth(g) + add_priors hand them out: the EdgeSE3 edges
    (odometry, then loop closures), the landmark edges, the priors.  dcs_phi > 0: DCS on the landmark edges without a kernel of their own."""

    def __init__(self, g, priors=(), fixed=None, dcs_phi: float = 0.0):
        super().__init__(g, priors, fixed)
        self.Eo, self.El, self.Ep = len(g.odom_ij), len(g.lm_ij), len(self.priors)
        n = self.Eo + self.El + self.Ep
        self.kind = g.landmark_kind
        self.rk = np.zeros(n, np.int64); self.rd = np.ones(n)
        self.dcs_phi = float(dcs_phi)

    def set_kernel(self, edge_id, kind, delta):
        self.rk[edge_id] = kind; self.rd[edge_id] = delta

    def _kernels(self):
        rk, rd = self.rk.copy(), self.rd.copy()
        if self.dcs_phi > 0:
            sl = slice(self.Eo, self.Eo + self.El)
            plain = rk[sl] == NONE
            rk[sl] = np.where(plain, DCS, rk[sl]); rd[sl] = np.where(plain, self.dcs_phi, rd[sl])
        return rk, rd

    def e2(self, poses=None, lms=None):
        """e^T Omega e of every edge, in edge id order"""
        poses = self.poses if poses is None else poses
        lms = self.lms if lms is None else lms
        g = self.g
        e = se3_error_jac(poses[g.odom_ij[:, 0]], poses[g.odom_ij[:, 1]], g.odom_z, False)
        out = [np.einsum('ei,eij,ej->e', e, g.odom_info, e)]
        fn = point_error_jac if self.kind == "point" else plane_error_jac
        el = fn(poses[g.lm_ij[:, 0]], lms[g.lm_ij[:, 1]], g.lm_z, False)
        out.append(np.einsum('ei,eij,ej->e', el, g.lm_info, el))
        ep = []
        for p, z, W in self.priors:
            r = poses[p, :len(z)] - z
            ep.append(float(r @ W @ r))
        out.append(np.asarray(ep, np.float64))
        return np.concatenate(out)

    def edge_chi2(self, poses=None, lms=None):
        """(e2, rho0, rho1) per edge"""
        e2 = self.e2(poses, lms)
        rk, rd = self._kernels()
        r0, r1 = rho(rk, rd, e2)
        return e2, r0, r1

    def chi2(self, poses=None, lms=None):
        return float(self.edge_chi2(poses, lms)[1].sum())

    def build(self):
        """the system of the plain graph whose information matrices are scaled by the edges' rho1"""
        _, _, r1 = self.edge_chi2()
        g0, p0 = self.g, self.priors
        g = copy.copy(g0)
        g.odom_info = g0.odom_info * r1[:self.Eo, None, None]
        g.lm_info = g0.lm_info * r1[self.Eo:self.Eo + self.El, None, None]
        self.g = g
        self.priors = [(p, z, W * r1[self.Eo + self.El + k]) for k, (p, z, W) in enumerate(p0)]
        try:
            return super().build()
        finally:
            self.g, self.priors = g0, p0
