"""The references themselves on dense information matrices, full 3-D attitudes and negated quaternions (tests/dense_info.py): the C
oracle against the NumPy restatement, the share of H that the dense terms carry, and the gauge invariance of the oracle.  These pin
what tests/test_dense_information_gpu.py compares the HIP path with."""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_info as D
from oracle import np_graph
from oracle.oracle import GraphProblem
from semantic_slam_amd.synth import make_graph


def _full(U):
    return (U + sp.triu(U, 1).T).tocsc()


@pytest.mark.parametrize("cond", [1e2, 1e6])
@pytest.mark.parametrize("kind,tol", [("point", 1e-12), ("plane", 1e-6)])
def test_oracle_matches_numpy_on_dense_information(kind, tol, cond):
    """tolerances of test_linearize_matches_numpy_restatement (plane Jacobians are finite differences on both sides)"""
    g = D.with_dense_information(make_graph(60, 12, seed=3, landmark_kind=kind), seed=11, cond=cond)
    for W in (g.odom_info, g.lm_info):
        assert np.array_equal(W, W.transpose(0, 2, 1))
        ev = np.linalg.eigvalsh(W)
        assert ev.min() > 0 and np.allclose(ev[:, -1] / ev[:, 0], cond, rtol=1e-6)
        assert len({float(w[0, 1]) for w in W}) == len(W)          # a different matrix on every edge
    sq, so = D.coupling_share(g)
    print(f"{kind} cond {cond:g}: coupling share {sq:.3e} off-diagonal share {so:.3e}")
    assert sq >= 1e-2 and so >= 5e-2
    gp = GraphProblem.from_synth(g)
    G = np_graph.NpGraph(g)
    U, b = gp.linearize()
    H, bn = G.build()
    dH = abs(_full(U) - H).max() / abs(H).max()
    db = np.abs(b - bn).max() / np.abs(bn).max()
    dc = abs(gp.chi2() - G.chi2()) / G.chi2()
    print(f"{kind} cond {cond:g}: oracle vs NumPy dH {dH:.3e} db {db:.3e} dchi2 {dc:.3e}")
    assert dH <= tol and db <= tol
    assert dc <= 1e-12


@pytest.mark.parametrize("mode", ["coupling", "blocks", "landmark"])
def test_localising_variants_are_what_they_say(mode):
    g0 = make_graph(60, 12, seed=3)
    g = D.with_dense_information(g0, seed=12, cond=1e2, mode=mode)
    assert np.linalg.eigvalsh(g.odom_info).min() > 0 and np.linalg.eigvalsh(g.lm_info).min() > 0
    sq, so = D.coupling_share(g)
    if mode == "coupling":
        assert D.schur_min_eig(g.odom_info) > 0
        assert np.array_equal(g.odom_info[:, :3, :3], g0.odom_info[:, :3, :3]) and np.array_equal(g.lm_info, g0.lm_info)
        assert sq >= 1e-2
    elif mode == "blocks":
        assert not g.odom_info[:, :3, 3:].any() and sq == 0.0 and so >= 5e-2
    else:
        assert np.array_equal(g.odom_info, g0.odom_info) and sq == 0.0
        assert D.landmark_share(g) >= 5e-2


@pytest.mark.parametrize("cond", [1e2, 1e6])
def test_oracle_is_gauge_invariant(cond):
    """the whole graph moved by a rigid transform, half the quaternions negated: chi2, the pose-pose blocks of H and the pose part of b
    stay (the increments are the poses' own); the landmark blocks of point landmarks turn with R"""
    g = D.with_dense_information(make_graph(60, 12, seed=3), seed=11, cond=cond)
    gm, n_neg, T = D.rigid_move(g, seed=5)
    assert n_neg > 0
    assert gm.poses_init[:, 6].min() < -0.1 and np.abs(gm.poses_init[:, 3:5]).max() > 0.3      # full attitude, non-canonical signs
    gp, gq = GraphProblem.from_synth(g), GraphProblem.from_synth(gm)
    c0, c1 = gp.chi2(), gq.chi2()
    assert abs(c1 - c0) <= 1e-12 * c0
    (U0, b0), (U1, b1) = gp.linearize(), gq.linearize()
    H0, H1 = _full(U0).toarray(), _full(U1).toarray()
    o = 6 * (g.n_poses - 1)
    dH = np.abs(H1[:o, :o] - H0[:o, :o]).max() / np.abs(H0).max()
    db = np.abs(b1[:o] - b0[:o]).max() / np.abs(b0).max()
    R = np_graph.qmat(T[3:])
    Rl = np.kron(np.eye(g.n_landmarks), R)
    dL = np.abs(H1[o:, o:] - Rl @ H0[o:, o:] @ Rl.T).max() / np.abs(H0[o:, o:]).max()
    print(f"cond {cond:g}: moved graph dchi2 {abs(c1 - c0) / c0:.3e} dH_pp {dH:.3e} db_p {db:.3e} dH_ll {dL:.3e} "
          f"min quaternion w {gm.poses_init[:, 6].min():.2f}, {n_neg} EdgeSE3 with a negative error quaternion")
    assert dH <= 1e-12
    assert db <= 1e-11            # measured 2.4e-14 here; up to 1e-12 with other transforms at cond 1e6 (|t| up to 50 m cancels in t_j - t_i)
    assert dL <= 1e-12
    # and the NumPy restatement agrees on the moved graph
    Hn, bn = np_graph.NpGraph(gm).build()
    assert abs(H1 - Hn).max() <= 1e-12 * abs(Hn).max() and np.abs(b1 - bn).max() <= 1e-12 * np.abs(bn).max()


def test_moved_plane_graph_oracle_matches_numpy():
    g = D.with_dense_information(make_graph(60, 12, seed=3, landmark_kind="plane"), seed=11, cond=1e2)
    gm, n_neg, _ = D.rigid_move(g, seed=5)
    assert n_neg > 0
    gp, gq = GraphProblem.from_synth(g), GraphProblem.from_synth(gm)
    assert abs(gq.chi2() - gp.chi2()) <= 1e-12 * gp.chi2()
    U, b = gq.linearize()
    Hn, bn = np_graph.NpGraph(gm).build()
    assert abs(_full(U) - Hn).max() <= 1e-6 * abs(Hn).max() and np.abs(b - bn).max() <= 1e-6 * np.abs(bn).max()


def test_oplus_beyond_the_unit_ball_takes_the_identity_rotation():
    """g2o's fromCompactQuaternion: w^2 = 1 - |dq|^2 < 0 gives the identity rotation (the translation part is still applied); at
    |dq| = 1 exactly w = 0, a half turn.  Oracle and NumPy agree on both sides of the branch."""
    g = make_graph(8, 3, seed=1)
    gp = GraphProblem.from_synth(g)
    _, n = gp.hessian_index()
    dx = np.random.default_rng(2).normal(0, 0.05, n)
    dx[:18].reshape(3, 6)[:, 3:] = D.OPLUS_EDGE_DQ
    assert np.allclose(np.linalg.norm(D.OPLUS_EDGE_DQ, axis=1), [0.999999, 1.0, 1.5], rtol=1e-12, atol=0)
    ref = np_graph.pose_oplus(gp.est[1:8].copy(), dx[:42].reshape(7, 6))
    before = gp.est.copy()
    gp.oplus(dx)
    assert np.abs(gp.est[1:8] - ref).max() < 1e-13
    assert np.abs(np.sum(gp.est[1, 3:] * before[1, 3:])) < 2e-3     # |dq| = 0.999999: w = 1.4e-3, almost a half turn
    assert np.abs(np.sum(gp.est[2, 3:] * before[2, 3:])) < 1e-15    # |dq| = 1: w = 0, a half turn
    assert np.abs(gp.est[3, 3:] - before[3, 3:]).max() < 1e-15      # |dq| = 1.5: rotation untouched ...
    assert np.abs(gp.est[3, :3] - before[3, :3]).max() > 1e-3       # ... translation applied
