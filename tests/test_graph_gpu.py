"""GPU parity of the ps_graph_slam backend: HIP path (through the C-ABI) vs the CPU oracle.

Reference semantics under test: GraphSLAM::optimize (reference src/ps_graph_slam/graph_slam.cpp:182-219)
and the g2o types it instantiates.  Tolerances: analytic edges H/b 1e-11 relative; plane edges
(numeric Jacobian, delta=1e-9) 1e-5; converged estimates <= 1e-4 relative (north_star), chi2 1e-6.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from semantic_slam_amd.synth import make_graph
from oracle.oracle import GraphProblem

pytestmark = pytest.mark.gpu


def _full(U):
    return (U + sp.triu(U, 1).T).tocsc()


@pytest.mark.parametrize("kind,interleave,tol", [("point", False, 1e-11), ("point", True, 1e-11), ("plane", False, 2e-5)])
def test_linearize_matches_oracle(gpu_lib, kind, interleave, tol):
    from semantic_slam_amd import GraphSLAM
    g = make_graph(60, 12, seed=3, landmark_kind=kind)
    gp = GraphProblem.from_synth(g, interleave=interleave)
    G = GraphSLAM.from_problem(gp)
    U, b = G.linearize()
    Uo, bo = gp.linearize()
    assert U.shape == Uo.shape
    scale = abs(Uo).max()
    assert abs(_full(U) - _full(Uo)).max() <= tol * scale
    assert np.abs(b - bo).max() <= tol * max(1.0, np.abs(bo).max())
    assert abs(G.chi2() - gp.chi2()) <= 1e-12 * gp.chi2()
    h, n = gp.hessian_index()
    assert [G.hessian_index(v) for v in range(gp.nv)] == list(h)


def test_linearize_with_repeated_edges(gpu_lib):
    """Two edges on the same vertex pair (a repeated loop closure / a landmark matched twice in one
    keyframe) share one off-diagonal block; the gather-form Jacobian build must sum them."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(60, 12, seed=8)
    gp0 = GraphProblem.from_synth(g, interleave=True)
    Eo = len(g.odom_ij)
    dup = [3, 17, Eo + 5, Eo + 40, 3]
    rng = np.random.default_rng(1)
    meas = np.concatenate([gp0.meas, gp0.meas[dup] + rng.normal(0, 1e-3, (len(dup), 7))])
    meas[:, 3:7] /= np.where(np.linalg.norm(meas[:, 3:7], axis=1, keepdims=True) > 0.5, np.linalg.norm(meas[:, 3:7], axis=1, keepdims=True), 1.0)
    gp = GraphProblem(gp0.vtype, gp0.vfixed, gp0.est, np.concatenate([gp0.etype, gp0.etype[dup]]),
                      np.concatenate([gp0.evi, gp0.evi[dup]]), np.concatenate([gp0.evj, gp0.evj[dup]]),
                      meas, np.concatenate([gp0.info, gp0.info[dup]]))
    G = GraphSLAM.from_problem(gp)
    U, b = G.linearize()
    Uo, bo = gp.linearize()
    assert abs(_full(U) - _full(Uo)).max() <= 1e-11 * abs(Uo).max()
    assert np.abs(b - bo).max() <= 1e-11 * np.abs(bo).max()
    assert G.optimize(5)
    st = gp.optimize(5)
    assert G.last_stats.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)


def test_jacobian_build_is_bitwise_deterministic(gpu_lib):
    from semantic_slam_amd import GraphSLAM
    gp = GraphProblem.from_synth(make_graph(200, 40, seed=9))
    G = GraphSLAM.from_problem(gp)
    U1, b1 = G.linearize()
    U2, b2 = G.linearize()
    assert np.array_equal(U1.data, U2.data) and np.array_equal(b1, b2)


def test_optimize_is_bitwise_repeatable(gpu_lib):
    """no atomics anywhere on the default path (gather-form Jacobian build, left-looking Cholesky with ordered partial sums,
    segmented reductions): two runs from the same state give identical bits"""
    from semantic_slam_amd import GraphSLAM
    gp = GraphProblem.from_synth(make_graph(300, 60, seed=21))
    runs = []
    for _ in range(2):
        G = GraphSLAM.from_problem(gp)
        assert G.optimize(6)
        runs.append((G.estimates().copy(), G.last_stats.chi2_after))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_oplus_matches_oracle(gpu_lib):
    from semantic_slam_amd import GraphSLAM
    for kind in ("point", "plane"):
        g = make_graph(40, 9, seed=5, landmark_kind=kind)
        gp = GraphProblem.from_synth(g, interleave=True)
        G = GraphSLAM.from_problem(gp)
        _, n = gp.hessian_index()
        dx = np.random.default_rng(0).normal(0, 0.05, n)
        G.oplus(dx)
        gp.oplus(dx)
        assert np.abs(G.estimates() - gp.est).max() < 1e-13


@pytest.mark.parametrize("lam", [5.0, 1e-3])
def test_pcg_solve_matches_oracle_cholesky(gpu_lib, lam):
    from semantic_slam_amd import GraphSLAM
    g = make_graph(120, 25, seed=1)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", 0)
    x, its = G.solve(lam)
    xo = gp.solve(lam)
    assert its > 0
    assert np.abs(x - xo).max() <= 1e-6 * np.abs(xo).max()


@pytest.mark.parametrize("lam", [5.0, 1e-3])
def test_schur_pcg_solve_matches_oracle_cholesky(gpu_lib, lam):
    """solver 2: landmarks eliminated (Hll is block diagonal), PCG on the reduced pose system applied matrix-free, landmarks
    back-substituted; same solution as the oracle's Cholesky.  A short LM run on top follows the oracle."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(120, 25, seed=1)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", 2)
    G.set_option("pcg_tol", 1e-10)
    x, its = G.solve(lam)
    xo = gp.solve(lam)
    assert its > 0
    assert np.abs(x - xo).max() <= 1e-6 * np.abs(xo).max()
    if lam == 5.0:
        assert G.optimize(4)
        st = gp.optimize(4)
        assert G.last_stats.iterations == st.iterations
        assert G.last_stats.chi2_after == pytest.approx(st.chi2_after, rel=1e-5)


@pytest.mark.parametrize("lam", [5.0, 1e-3, 0.0])
def test_cholesky_solve_matches_oracle_cholesky(gpu_lib, lam):
    from semantic_slam_amd import GraphSLAM
    g = make_graph(150, 30, seed=7)
    gp = GraphProblem.from_synth(g, interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", 1)
    x, its = G.solve(lam)
    xo = gp.solve(lam)
    assert its == 0
    assert np.abs(x - xo).max() <= 1e-9 * np.abs(xo).max()
    # and the residual of the normal equations themselves
    U, b = G.linearize()
    H = _full(U) + lam * sp.identity(U.shape[0])
    assert np.abs(H @ x - b).max() <= 1e-9 * np.abs(b).max()


@pytest.mark.parametrize("env", [
    {"cap_leaf": "400", "cap_tail": "700", "tail_width": "2", "min_chunk": "1", "pcap_leaf": "16", "nt_leaf": "256"},   # many pieces, split lists, a multi-piece tail
    {"cap_leaf": "400", "cap_tail": "700", "tail_width": "0"},     # no tail: one launch per depth
    {"cap_leaf": "900", "cap_tail": "2000", "nt_tail": "1024"},    # 1024-thread tail workgroups
    {"cap_leaf": "400", "group_cap": "1500", "nt_leaf": "512", "ustage": "0"},   # groups of subtrees per workgroup
    {"cap_leaf": "400", "group_cap": "1200", "nt_leaf": "64", "min_chunk": "1"},
    {"split_min": "4", "tail_width": "2"},      # depths launched in parts, by LDS need
    # round 5, mid class: the depths between the bottom and the tail as larger pieces on 256-thread workgroups (per-depth launches: no k_chol_flow)
    {"flow": "0", "cap_leaf": "400", "tail_width": "2", "mid_width": "12", "cap_mid": "1200"},
    {"flow": "0", "cap_leaf": "400", "tail_width": "0", "mid_width": "8", "cap_mid": "1500", "nt_mid": "512"},
    # round 6, front tables (one blob of relative indices per workgroup; k_front_pieces / k_front_tail): all three classes, groups, no tail, the single launch
    {"front": "1", "flow": "0", "cap_leaf": "400", "tail_width": "2", "mid_width": "12", "cap_mid": "1200"},
    {"front": "1", "flow": "0", "cap_leaf": "300", "group_cap": "1200", "nt_leaf": "128", "tail_width": "0", "mid_width": "8", "cap_mid": "1500"},
    {"front": "1", "cap_leaf": "400", "cap_tail": "700", "tail_width": "2"},
    # widths outside the instantiated sets: planned and launched as their normalised values (chol_opts_normalise)
    {"front": "1", "flow": "0", "cap_leaf": "400", "cap_tail": "700", "tail_width": "2", "nt_ftail": "2048", "nt_btail": "100", "nt_bleaf": "100"},
])
def test_cholesky_pieces_of_every_shape(gpu_lib, monkeypatch, env):
    """The piece plan is cut by LDS capacity; caps far below the defaults force what the 5000-pose graph has (pieces with
    external updates, split update lists summed through partial tiles, a tail of several pieces) onto a 150-pose graph
    whose solution is checked against the oracle's Cholesky.  The same plans are pinned on the CPU by tests/test_chol_plan_cpu.py."""
    from semantic_slam_amd import GraphSLAM
    monkeypatch.setenv("SSLAM_CHOL_OPTS", ",".join(f"{k}={v}" for k, v in env.items()))   # plan options by field name (chol_plan.hpp CholOpts)
    g = make_graph(150, 30, seed=5)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    for lam in (1e-3, 4.0):
        x, _ = G.solve(lam)
        xo = gp.solve(lam)
        assert np.abs(x - xo).max() <= 1e-9 * np.abs(xo).max()
    assert G.optimize(8)
    st = gp.optimize(8)
    assert G.last_stats.iterations == st.iterations and G.last_stats.trials == st.trials
    assert G.last_stats.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()


def test_batch_member_with_too_few_edges_is_left_alone(gpu_lib):
    """graph_slam.cpp:184-186 inside a batch: a member with fewer than 10 edges is not optimised (status TOO_FEW_EDGES), the others are."""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gp = GraphProblem.from_synth(make_graph(60, 12, seed=10))
    big = GraphSLAM.from_problem(gp)
    small = GraphSLAM()
    a = small.add_se3_node([0, 0, 0, 0, 0, 0, 1]); b = small.add_se3_node([1.1, 0, 0, 0, 0, 0, 1])
    for _ in range(3):
        small.add_se3_edge(a, b, [1, 0, 0, 0, 0, 0, 1], np.eye(6))
    B = GraphBatch([big, small]); B.upload()
    st = B.optimize(5); B.download()
    assert st[0].iterations == 5 and st[0].chi2_after < st[0].chi2_before
    assert st[1].status == -5 and st[1].iterations == 0
    assert np.array_equal(small.estimate(b), [1.1, 0, 0, 0, 0, 0, 1])
    # a graph that gains an edge after the batch was compiled invalidates the batch (no out-of-bounds access)
    from semantic_slam_amd import SslamError
    small.add_se3_edge(a, b, [1, 0, 0, 0, 0, 0, 1], np.eye(6))
    with pytest.raises(SslamError):
        B.optimize(1)


@pytest.mark.parametrize("kind,solver", [("point", 1), ("plane", 1), ("point", 0), ("plane", 0)])
def test_optimize_small_graph_matches_oracle(gpu_lib, kind, solver):
    from semantic_slam_amd import GraphSLAM
    g = make_graph(100, 20, seed=2, landmark_kind=kind)
    gp = GraphProblem.from_synth(g, interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", solver)
    assert G.optimize(12) is True
    st = gp.optimize(12)
    s = G.last_stats
    assert s.chi2_before == pytest.approx(st.chi2_before, rel=1e-12)
    assert s.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    E, Eo = G.estimates(), gp.est
    assert np.abs(E - Eo).max() <= 1e-4 * np.abs(Eo).max()


@pytest.mark.parametrize("solver", [1, 0])
def test_optimize_S_config_10_iterations(gpu_lib, solver):
    """BASELINE.json configs[1]: 500 poses / 100 landmarks, exactly 10 LM iterations."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(500, 100, seed=0)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", solver)
    assert G.optimize(10)
    st = gp.optimize(10)
    s = G.last_stats
    assert s.iterations == st.iterations == 10
    assert s.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    E, Eo = G.estimates(), gp.est
    assert np.abs(E - Eo).max() <= 1e-4 * np.abs(Eo).max()
    # gauge: the fixed first vertex does not move (graph_slam.cpp:109-111)
    assert np.array_equal(E[0], g.poses_init[0])


def test_schur_pcg_on_the_S_config(gpu_lib):
    """BASELINE.json configs[1] through solver 2 (north_star's "Schur-complement + PCG": landmarks eliminated, matrix-free PCG on the
    reduced pose system with the block-Jacobi preconditioner): ten LM iterations land on the oracle's chi2 / estimates.  The CG
    iteration count per trial is what keeps this solver from being the default: printed, and bounded here."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(500, 100, seed=0)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", 2)
    G.set_option("pcg_tol", 1e-10)
    assert G.optimize(10)
    st = gp.optimize(10)
    s = G.last_stats
    assert s.iterations == st.iterations == 10
    assert s.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()
    per_trial = s.solver_iterations / max(s.trials, 1)
    print(f"schur+pcg S config: {s.solver_iterations} CG iterations over {s.trials} trials ({per_trial:.0f} per trial)")
    assert 10 < per_trial < 6000


def test_schur_pcg_on_the_L_config(gpu_lib):
    """BASELINE.json configs[2] through solver 2 (round 6; the verdict's missing parity case): three LM iterations of the 5000-pose graph
    land on the oracle's chi2 / estimates.  ~1000 CG iterations per trial with the block-Jacobi preconditioner -- two orders of magnitude
    slower than the sparse Cholesky, which is why it is not a solver for this configuration (sslam.h; DESIGN.md section 5: an exact
    block-tridiagonal preconditioner of the odometry chain brings the count to ~110 at the price of two 5000-step sequential sweeps per
    CG iteration)."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(5000, 1000, seed=0)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", 2)
    G.set_option("pcg_tol", 1e-10)
    assert G.optimize(3)
    st = gp.optimize(3)
    s = G.last_stats
    assert s.iterations == st.iterations == 3
    assert s.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()
    per_trial = s.solver_iterations / max(s.trials, 1)
    print(f"schur+pcg L config: {s.solver_iterations} CG iterations over {s.trials} trials ({per_trial:.0f} per trial)")
    assert 100 < per_trial < 20000


def test_optimize_L_config(gpu_lib):
    """BASELINE.json configs[2]: 5000 poses / 1000 landmarks + loop closures; 10 iterations, then to termination."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(5000, 1000, seed=0)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    assert G.optimize(10)
    st = gp.optimize(10)
    s = G.last_stats
    assert s.iterations == st.iterations == 10
    assert s.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()
    # run both to LM termination (cap 1024 as graph_slam.cpp:205): converged estimates must agree
    assert G.optimize(1024)
    st2 = gp.optimize(1024)
    assert G.last_stats.status == 1 and st2.status == 1
    assert G.last_stats.chi2_after == pytest.approx(st2.chi2_after, rel=1e-8)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()
    print(f"L graph to termination: HIP {G.last_stats.iterations} iterations / {G.last_stats.trials} trials, "
          f"oracle {st2.iterations} / {st2.trials}")


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_L_config_termination_iteration(gpu_lib, seed):
    """SURVEY §7 hard part 3: g2o's LM stops when rho == 0 or ten trials in a row fail.  At the optimum chi2 stalls at
    the rounding level of the sum over 20,099 edges and the sign of rho = (chi2_old - chi2_new) / scale is decided by the
    last bits; the HIP path and the oracle sum in different orders, so the two may stop a few iterations apart.  What must
    agree: every iteration before either side stalls (same count, same trials), and the converged chi2 / estimates."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(5000, 1000, seed=seed)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    assert G.optimize(14)
    st = gp.optimize(14)
    assert G.last_stats.iterations == st.iterations == 14 and G.last_stats.trials == st.trials
    assert G.optimize(64)
    st2 = gp.optimize(64)
    s2 = G.last_stats
    print(f"seed {seed}: after 14 iterations HIP terminates {s2.iterations} (trials {s2.trials}) further on, oracle {st2.iterations} (trials {st2.trials})")
    assert s2.status == 1 and st2.status == 1
    assert abs(s2.iterations - st2.iterations) <= 8
    assert s2.chi2_after == pytest.approx(st2.chi2_after, rel=1e-9)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-6 * np.abs(gp.est).max()


def test_dcs_robust_kernel_matches_oracle(gpu_lib):
    """opt-in RobustKernelDCS on the landmark edges (sslam_graph_set_option "robust_kernel_dcs" = phi): chi2, the
    normal equations and the optimised estimates equal the oracle's with the same kernel, for point and plane landmarks, with a few gross
    outliers among the landmark measurements"""
    from semantic_slam_amd import GraphSLAM
    from oracle import oracle as O
    for kind, tol in (("point", 1e-11), ("plane", 2e-5)):
        g = make_graph(120, 24, seed=8, landmark_kind=kind)
        gp = GraphProblem.from_synth(g, interleave=True)
        out = np.nonzero(gp.etype != 0)[0][::17]
        gp.meas[out, :3] += np.array([0.8, -0.6, 0.5]) if kind == "point" else np.array([0.3, -0.2, 0.1])
        if kind == "plane":
            gp.meas[out, :3] /= np.linalg.norm(gp.meas[out, :3], axis=1, keepdims=True)
        G = GraphSLAM.from_problem(gp)
        G.set_option("robust_kernel_dcs", 1.0)
        try:
            O.set_dcs(1.0)
            assert G.chi2() == pytest.approx(gp.chi2(), rel=1e-12)
            U, b = G.linearize()
            Uo, bo = gp.linearize()
            assert np.abs((U - Uo).toarray()).max() <= tol * np.abs(Uo.toarray()).max() and np.abs(b - bo).max() <= tol * np.abs(bo).max()
            assert G.optimize(15)
            st = gp.optimize(15)
        finally:
            O.set_dcs(0.0)
        assert G.last_stats.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
        assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()
        G.set_option("robust_kernel_dcs", 0.0)
        assert G.chi2() == pytest.approx(gp.chi2(), rel=1e-9)          # kernel off again: the plain chi2 of the optimised state


@pytest.mark.parametrize("solver", [1, 0])
def test_point_point_edges_match_oracle(gpu_lib, solver, tmp_path):
    """add_point_xyz_point_xyz_edge (g2o::EdgePointXYZ, reference graph_slam.cpp:168-180): landmark-landmark blocks in H (the landmark
    block is no longer block diagonal), two edges on one vertex pair; chi2, the normal equations, the optimised estimates and the g2o
    text round trip against the oracle; solver 2 (Schur on the landmarks) refuses such a graph"""
    from semantic_slam_amd import GraphSLAM
    from semantic_slam_amd.graph_slam import SslamError
    from tests.test_oracle_graph import _with_point_point_edges
    rng = np.random.default_rng(9)
    gp = _with_point_point_edges(GraphProblem.from_synth(make_graph(90, 18, seed=6), interleave=True), rng, n_extra=20)
    G = GraphSLAM.from_problem(gp)
    G.set_option("solver", solver)
    assert G.chi2() == pytest.approx(gp.chi2(), rel=1e-12)
    U, b = G.linearize()
    Uo, bo = gp.linearize()
    assert np.abs((U - Uo).toarray()).max() <= 1e-11 * np.abs(Uo.toarray()).max() and np.abs(b - bo).max() <= 1e-11 * np.abs(bo).max()
    x, _ = G.solve(0.7)
    xr = gp.solve(0.7)
    assert np.abs(x - xr).max() <= (1e-6 if solver == 0 else 1e-8) * np.abs(xr).max()
    path = str(tmp_path / "pp.g2o")
    G.save(path)
    G2 = GraphSLAM(); G2.load(path)
    assert G2.num_edges() == gp.ne and G2.chi2() == pytest.approx(gp.chi2(), rel=1e-12)
    assert G.optimize(12)
    st = gp.optimize(12)
    assert G.last_stats.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    assert np.abs(G.estimates() - gp.est).max() <= 1e-4 * np.abs(gp.est).max()
    if solver == 1:
        G.set_option("solver", 2)
        with pytest.raises(SslamError):
            G.solve(0.7)


def test_too_few_edges_returns_false(gpu_lib):
    from semantic_slam_amd import GraphSLAM
    G = GraphSLAM()
    a = G.add_se3_node([0, 0, 0, 0, 0, 0, 1])
    b = G.add_se3_node([1, 0, 0, 0, 0, 0, 1])
    G.add_se3_edge(a, b, [1, 0, 0, 0, 0, 0, 1], np.eye(6))
    assert G.optimize() is False          # graph_slam.cpp:184-186
    assert np.array_equal(G.estimate(b), [1, 0, 0, 0, 0, 0, 1])


def test_noise_free_graph_is_a_fixed_point(gpu_lib):
    from semantic_slam_amd import GraphSLAM
    g = make_graph(50, 10, seed=4, noise_scale=0.0)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    assert G.chi2() < 1e-18
    G.optimize(3)
    assert G.last_stats.chi2_after < 1e-18
    E = G.estimates()[:50]
    sign = np.where(np.sum(E[:, 3:] * g.poses_true[:, 3:], axis=1, keepdims=True) < 0, -1.0, 1.0)  # q ~ -q
    assert np.abs(E[:, :3] - g.poses_true[:, :3]).max() < 1e-9
    assert np.abs(sign * E[:, 3:] - g.poses_true[:, 3:]).max() < 1e-9


def test_batch_matches_individual(gpu_lib):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    sizes = [(60, 12), (45, 9), (80, 15)]
    gps = [GraphProblem.from_synth(make_graph(a, b, seed=10 + i)) for i, (a, b) in enumerate(sizes)]
    singles = [GraphSLAM.from_problem(gp) for gp in gps]
    for G in singles:
        G.optimize(8)
    batch_graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(batch_graphs)
    B.upload()
    stats = B.optimize(8)
    B.download()
    for G1, G2, st in zip(singles, batch_graphs, stats):
        assert st.iterations == G1.last_stats.iterations
        assert st.chi2_after == pytest.approx(G1.last_stats.chi2_after, rel=1e-9)
        assert np.abs(G1.estimates() - G2.estimates()).max() < 1e-9


def test_large_batch_of_unequal_graphs_matches_individual(gpu_lib):
    """a batch of >= 32 graphs switches the factorisation to the wider per-graph tail (levels <= 4 columns wide);
    every graph has its own structure, one is noise-free (fixed point from the first iteration)"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = []
    for i in range(34):
        g = make_graph(40 + 3 * i, 8 + (i % 5), seed=100 + i, noise_scale=0.0 if i == 7 else 1.0)
        gps.append(GraphProblem.from_synth(g, interleave=bool(i & 1)))
    singles = [GraphSLAM.from_problem(gp) for gp in gps]
    for G in singles:
        G.optimize(6)
    batch_graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(batch_graphs)
    B.upload()
    stats = B.optimize(6)
    B.download()
    for G1, G2, st in zip(singles, batch_graphs, stats):
        assert st.iterations == G1.last_stats.iterations
        assert st.chi2_after == pytest.approx(G1.last_stats.chi2_after, rel=1e-9, abs=1e-18)
        assert np.abs(G1.estimates() - G2.estimates()).max() < 1e-9


def test_batch_regime_plan_with_all_three_piece_classes_matches_the_oracle(gpu_lib):
    """Round 5: a batch of >= 32 graphs takes the throughput plan -- groups of leaf pieces on 128-thread workgroups, mid pieces on 256, a tail
    per graph.  32 distinct graphs of ~600 poses (all three classes present: the plan is also walked on the CPU by
    tests/test_chol_plan_cpu.py) against the oracle on a sample and against their own single-handle runs (the latency plan) on all."""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(600 + 7 * k, 120 + k, seed=500 + k), interleave=bool(k & 1)) for k in range(32)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs); B.upload()
    stats = B.optimize(6)
    B.download()
    for k in (0, 13, 31):
        st = gps[k].optimize(6)
        assert stats[k].iterations == st.iterations and stats[k].trials == st.trials
        assert stats[k].chi2_after == pytest.approx(st.chi2_after, rel=1e-9)
        assert np.abs(graphs[k].estimates() - gps[k].est).max() <= 1e-6 * np.abs(gps[k].est).max()
    gps2 = [GraphProblem.from_synth(make_graph(600 + 7 * k, 120 + k, seed=500 + k), interleave=bool(k & 1)) for k in range(32)]
    for k in range(0, 32, 5):
        G = GraphSLAM.from_problem(gps2[k])
        assert G.optimize(6)
        assert G.last_stats.iterations == stats[k].iterations
        assert G.last_stats.chi2_after == pytest.approx(stats[k].chi2_after, rel=1e-9)
        assert np.abs(G.estimates() - graphs[k].estimates()).max() <= 1e-8 * np.abs(G.estimates()).max()


def test_stream_group_matches_the_single_stream_batch(gpu_lib):
    """sslam_batch_create_streams: the graphs split over several batches, each on its own stream + host thread.  Every graph runs its own
    LM, so the parts only change what overlaps on the chip: with parts of >= 32 graphs (same plan parameters as the whole batch) the
    results are bitwise those of one batch; info keys are sums over the parts; the edge-sharded mode refuses a group"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    from semantic_slam_amd.graph_slam import SslamError
    gps = []
    for i in range(70):
        g = make_graph(40 + 2 * i, 8 + (i % 5), seed=300 + i, noise_scale=0.0 if i == 11 else 1.0)
        gps.append(GraphProblem.from_synth(g, interleave=bool(i & 1)))
    one = [GraphSLAM.from_problem(gp) for gp in gps]
    B1 = GraphBatch(one)
    B1.upload()
    s1 = B1.optimize(7)
    B1.download()
    grp = [GraphSLAM.from_problem(gp) for gp in gps]
    B2 = GraphBatch(grp, streams=2)
    assert B2.info("streams") == 2 and B1.info("streams") == 1
    B2.upload()
    s2 = B2.optimize(7)
    B2.download()
    for a, b, G1, G2 in zip(s1, s2, one, grp):
        assert (a.iterations, a.trials, a.status) == (b.iterations, b.trials, b.status)
        assert a.chi2_after == b.chi2_after
        assert np.array_equal(G1.estimates(), G2.estimates())
    assert B2.info("dim") == B1.info("dim") and B2.info("factor_lnz") == B1.info("factor_lnz")
    assert B2.linearize_bytes() == B1.linearize_bytes()
    f, v = B2.time_solver(1)
    assert f > 0 and v > 0
    with pytest.raises(SslamError):
        B2.set_edge_shard(0, 2)
    with pytest.raises(SslamError):
        B2.linearize_hb()
    # more streams than a part can fill: parts of 3-4 graphs, a second optimize on the same handle continues from the first
    few = [GraphSLAM.from_problem(gp) for gp in gps[:10]]
    B3 = GraphBatch(few, streams=3)
    B3.upload()
    s3 = B3.optimize(7)
    B3.download()
    for a, b, G1, G3 in zip(s1, s3, one, few):
        assert a.iterations == b.iterations
        assert b.chi2_after == pytest.approx(a.chi2_after, rel=1e-9, abs=1e-18)
        assert np.abs(G1.estimates() - G3.estimates()).max() < 1e-9


def _endgame_run(gps, build, iters, monkeypatch, compact):
    """one batch through optimize(iters) with the compaction of the LM endgame on or off (SSLAM_CHOL_OPTS compact, read when the plan is built)"""
    from semantic_slam_amd import GraphBatch
    if compact:
        monkeypatch.delenv("SSLAM_CHOL_OPTS", raising=False)
    else:
        monkeypatch.setenv("SSLAM_CHOL_OPTS", "compact=0")
    graphs = build(gps)
    B = GraphBatch(graphs); B.upload()
    stats = B.optimize(iters)
    B.download()
    monkeypatch.delenv("SSLAM_CHOL_OPTS", raising=False)
    return graphs, stats, B.info("compact_rounds")


def _assert_runs_bitwise_equal(run_a, run_b):
    (ga, sa, _), (gb, sb, _) = run_a, run_b
    for k, (a, b, Ga, Gb) in enumerate(zip(sa, sb, ga, gb)):
        assert (a.status, a.iterations, a.trials) == (b.status, b.iterations, b.trials), k
        assert a.chi2_before == b.chi2_before and a.chi2_after == b.chi2_after, k
        assert np.array_equal(Ga.estimates(), Gb.estimates()), k


def test_lm_endgame_compacts_once_most_of_the_batch_is_done(gpu_lib, monkeypatch):
    """batch_optimize looks at the LM states every 8 steps and, once at most half of a batch of >= 8 graphs is still active, sizes the
    factor / solve launches by index lists of the active graphs' pieces (chol_set_active).  Deterministic trigger: eight of twelve members
    have 9 edges -- TOO_FEW_EDGES, inactive from k_lm_init on, yet owners of pieces in the plan -- so the first look finds 4 of 12 active and
    steps 9 .. 24 of the four noisy graphs run off the index lists.  Against the oracle at the bars of the batch-regime test, and bitwise
    against the same batch with the compaction switched off (SSLAM_CHOL_OPTS compact=0).
    The noisy graphs are far from converged after 24 iterations (noise_scale 25 for points, 3 for planes: the oracle needs all 24, with
    rejected trials on the way, and its counts do not move under 1e-13 perturbations of the measurements): iteration and trial counts at
    the noise floor are decided by last bits (test_L_config_termination_iteration) and are not what this test is about."""
    from semantic_slam_amd import GraphSLAM
    noisy = [(80, 16, 840, 25.0), (110, 22, 860, 3.0), (140, 28, 843, 25.0), (170, 34, 867, 3.0)]
    gps = [GraphProblem.from_synth(make_graph(a, b, seed=s, noise_scale=ns, landmark_kind="plane" if i & 1 else "point"), interleave=bool(i & 1))
           for i, (a, b, s, ns) in enumerate(noisy)]

    def small(k):
        """a 5-pose chain (4 odometry edges) and one landmark seen from all five poses: 9 edges"""
        G = GraphSLAM()
        ps = [G.add_se3_node([1.0 * j + 0.05 * k, 0.02 * j * j, 0, 0, 0, 0, 1]) for j in range(5)]
        l = G.add_point_xyz_node([2.0, 1.0 + 0.1 * k, 0.5])
        for j in range(4):
            G.add_se3_edge(ps[j], ps[j + 1], [1, 0, 0, 0, 0, 0, 1], np.eye(6))
        for j in range(5):
            G.add_se3_point_xyz_edge(ps[j], l, [2.0 - j, 1.0, 0.5], np.eye(3))
        assert G.num_edges() == 9
        return G

    order = ["s", "s", 0, "s", "s", 1, "s", "s", 2, "s", "s", 3]          # batch order: the noisy graphs between the small members

    def build(gps):
        return [small(k) if m == "s" else GraphSLAM.from_problem(gps[m]) for k, m in enumerate(order)]

    run1 = _endgame_run(gps, build, 24, monkeypatch, compact=True)
    run0 = _endgame_run(gps, build, 24, monkeypatch, compact=False)
    assert run1[2] >= 1 and run0[2] == 0
    _assert_runs_bitwise_equal(run1, run0)
    graphs, stats, _ = run1
    untouched = build(gps)
    for k, m in enumerate(order):
        if m == "s":
            assert stats[k].status == -5 and stats[k].iterations == 0
            assert np.array_equal(graphs[k].estimates(), untouched[k].estimates())
    ref = {}
    for k, m in enumerate(order):                        # every figure is printed before anything is asserted
        if m == "s":
            continue
        gp = gps[m].copy()
        ref[k] = (gp, gp.optimize(24))
        st = ref[k][1]
        chi_rel = abs(stats[k].chi2_after - st.chi2_after) / st.chi2_after
        est_rel = np.abs(graphs[k].estimates() - gp.est).max() / np.abs(gp.est).max()
        print(f"noisy graph {m}: HIP iterations {stats[k].iterations} trials {stats[k].trials}, oracle {st.iterations} {st.trials}; chi2 rel {chi_rel:.3e} estimates rel {est_rel:.3e}")
    for k, (gp, st) in ref.items():
        assert stats[k].iterations == st.iterations and stats[k].trials == st.trials
        assert stats[k].chi2_after == pytest.approx(st.chi2_after, rel=1e-9)
        assert np.abs(graphs[k].estimates() - gp.est).max() <= 1e-6 * np.abs(gp.est).max()


def test_lm_endgame_compaction_at_natural_termination(gpu_lib, monkeypatch):
    """Sixteen graphs run to termination.  Eight (noise_scale 1) stop after at most 29 trials in the oracle, under 1e-13 perturbations of
    their measurements as well (the count at the noise floor is decided by last bits); eight (noise_scale 50 / 100) need at least 59.  For
    a batch of >= 8 graphs one step is one trial, so the look after 32 or 40 steps finds the early half done with trials to spare and the
    late half active: the rest of the run goes off index lists.  compact_rounds >= 1 is the condition on these inputs."""
    from semantic_slam_amd import GraphSLAM
    early = [(30, 6, 700, False), (36, 8, 702, True), (42, 6, 704, False), (48, 8, 706, True), (54, 6, 708, False), (60, 8, 710, True),
             (72, 8, 714, True), (84, 8, 718, True)]
    late = [(85, 13, 765, 50.0, False), (90, 14, 766, 50.0, True), (95, 15, 767, 50.0, True), (100, 12, 768, 50.0, False),
            (90, 14, 766, 100.0, True), (95, 15, 767, 100.0, True), (100, 12, 768, 100.0, False), (105, 13, 769, 100.0, False)]
    gps = []
    for e, l in zip(early, late):                                            # early and late alternate in batch order
        gps.append(GraphProblem.from_synth(make_graph(e[0], e[1], seed=e[2]), interleave=e[3]))
        gps.append(GraphProblem.from_synth(make_graph(l[0], l[1], seed=l[2], noise_scale=l[3]), interleave=l[4]))

    def build(gps):
        return [GraphSLAM.from_problem(gp) for gp in gps]

    run1 = _endgame_run(gps, build, 1024, monkeypatch, compact=True)
    run0 = _endgame_run(gps, build, 1024, monkeypatch, compact=False)
    print("trials:", [s.trials for s in run1[1]], "compact rounds", run1[2])
    assert run1[2] >= 1 and run0[2] == 0
    _assert_runs_bitwise_equal(run1, run0)
    graphs, stats, _ = run1
    assert all(s.status == 1 for s in stats)
    for k, gp0 in enumerate(gps):
        gp = gp0.copy()
        st = gp.optimize(1024)
        assert st.status == 1
        chi_rel = abs(stats[k].chi2_after - st.chi2_after) / st.chi2_after
        est_rel = np.abs(graphs[k].estimates() - gp.est).max() / np.abs(gp.est).max()
        print(f"graph {k}: HIP trials {stats[k].trials}, oracle {st.trials}; chi2 rel {chi_rel:.3e} estimates rel {est_rel:.3e}")
        assert stats[k].chi2_after == pytest.approx(st.chi2_after, rel=1e-9)
        assert est_rel <= 1e-6


def test_edge_shards_sum_to_the_full_system(gpu_lib):
    """SURVEY 8e mode E on one device: the partial normal equations of the edge shards of 3 ranks (graph-local edge ranges
    identical to distributed.shard_range) add up to the full [H || b]; with world = 1 the mode is off again."""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    from semantic_slam_amd.distributed import shard_range
    gps = [GraphProblem.from_synth(make_graph(80, 15, seed=31), interleave=True), GraphProblem.from_synth(make_graph(50, 9, seed=32, landmark_kind="plane"))]
    B = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps]); B.upload()
    full = B.linearize_hb()
    assert np.abs(full).max() > 0
    parts = []
    for r in range(3):
        B.set_edge_shard(r, 3)
        parts.append(B.linearize_hb())
    tot = parts[0] + parts[1] + parts[2]
    assert np.abs(tot - full).max() <= 1e-12 * np.abs(full).max()
    assert all(np.abs(p).max() > 0 and np.abs(p - full).max() > 0 for p in parts)
    # the first rank's share of graph 0 is exactly the oracle system of that edge range
    lo, hi = shard_range(gps[0].ne, 0, 3)
    assert (lo, hi) == (0, (gps[0].ne + 2) // 3)
    B.set_edge_shard(0, 1)
    assert np.array_equal(B.linearize_hb(), full)
    st = B.optimize(4)
    assert st[0].iterations == 4 and st[0].chi2_after < st[0].chi2_before


def test_edge_shards_of_the_L_graph_sum_to_the_full_system(gpu_lib):
    """BASELINE.json configs[4] geometry on one device: the 8 edge shards of a 5000-pose / 1000-landmark graph (the ranges 8 ranks
    would own) each build their partial [H || b] with the product's shard-masked kernels; their sum is the full system."""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    from semantic_slam_amd.distributed import shard_range
    g = make_graph(5000, 1000, seed=0)
    G = GraphSLAM.from_synth(g)
    B = GraphBatch([G]); B.upload()
    full = B.linearize_hb()
    tot = np.zeros_like(full)
    ne = G.num_edges()
    covered = 0
    for r in range(8):
        B.set_edge_shard(r, 8)
        part = B.linearize_hb()
        assert np.abs(part).max() > 0 and np.abs(part - full).max() > 0
        tot += part
        lo, hi = shard_range(ne, r, 8)
        covered += hi - lo
    assert covered == ne == 20099
    assert np.abs(tot - full).max() <= 1e-12 * np.abs(full).max()
    B.set_edge_shard(0, 1)
    assert np.array_equal(B.linearize_hb(), full)


def test_single_rank_communicator_runs_the_allreduce_inside_the_lm_loop(gpu_lib, monkeypatch):
    """The RCCL path of the edge-sharded mode with a live communicator on ONE GPU (SSLAM_FORCE_COMM=1): ncclCommInitRank(world 1),
    shard-masked Jacobian kernels, the out-of-place ncclAllReduce of [H || b] on the batch stream inside batch_optimize.  Results
    are bit-identical to the unsharded run, including the steps in which a graph only retries a rejected trial (its partial system
    is not rebuilt; the all-reduce must leave its H as it was -- round-2 ADVICE)."""
    import ctypes as C
    from semantic_slam_amd import GraphSLAM, GraphBatch, load_library
    lib = load_library()
    gps = [GraphProblem.from_synth(make_graph(70 + 5 * i, 14, seed=40 + i), interleave=bool(i & 1)) for i in range(5)]
    gps.append(GraphProblem.from_synth(make_graph(50, 9, seed=46, landmark_kind="plane")))

    def run(force):
        gs = [GraphSLAM.from_problem(gp) for gp in gps]
        B = GraphBatch(gs); B.upload()
        if force:
            buf = C.create_string_buffer(128)
            assert lib.sslam_comm_unique_id(buf) == 0, lib.sslam_last_error()
            B.comm_init(buf.raw, 0, 1)
        st = B.optimize(60)
        B.download()
        return B, st, [G.estimates() for G in gs]

    _, s0, e0 = run(False)
    monkeypatch.setenv("SSLAM_FORCE_COMM", "1")
    B, s1, e1 = run(True)
    assert B.info("allreduce_calls") >= max(st.trials for st in s1) > 0
    assert any(st.trials > st.iterations for st in s1)          # some graph retried with a raised lambda
    for a, b, x, y in zip(s0, s1, e0, e1):
        assert (a.iterations, a.trials, a.status) == (b.iterations, b.trials, b.status)
        assert a.chi2_after == b.chi2_after and a.chi2_before == b.chi2_before
        assert np.array_equal(x, y)


def test_marginals_match_oracle(gpu_lib):
    from semantic_slam_amd import GraphSLAM
    g = make_graph(40, 8, seed=6)
    gp = GraphProblem.from_synth(g, interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.optimize(6)
    gp.est[:] = G.estimates()
    ids = [int(v) for v in gp.lm_ids]
    blocks = G.computeLandmarkMarginals(ids)
    ref = gp.marginals(ids).reshape(-1, 3, 3)
    for a, r in zip(blocks, ref):
        assert np.abs(a - r).max() <= 1e-6 * np.abs(r).max()


def test_diagonal_blocks_do_not_depend_on_the_rest_of_the_request_list(gpu_lib):
    """Every request is one wave of the pair kernel (k_chol_marginal_pairs) walking the elimination-tree path of its vertex.  A
    diagonal-only request list and the same list with an off-diagonal pair appended give the same diagonal blocks, bit for bit -- neither
    the place of a request in the list nor its neighbours enter its arithmetic -- and they equal the dense inverse of the oracle's H:
    landmark 3x3 and pose 6x6 blocks."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(60, 12, seed=4)
    gp = GraphProblem.from_synth(g, interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.optimize(5)
    gp.est[:] = G.estimates()
    U, _ = gp.linearize()
    Hinv = np.linalg.inv((U + sp.triu(U, 1).T).toarray())
    hs = [G.hessian_index(int(v)) for v in gp.lm_ids] + [G.hessian_index(int(gp.pose_ids[k])) for k in (1, 7, 30, 59)]
    diag = [(h, h) for h in hs]
    a = G.computeMarginals(diag)
    b = G.computeMarginals(diag + [(hs[0], hs[1])])
    for (r, c) in diag:
        ref = Hinv[r:r + a[(r, c)].shape[0], c:c + a[(r, c)].shape[1]]
        assert a[(r, c)].shape == b[(r, c)].shape and a[(r, c)].shape[0] in (3, 6)
        assert np.abs(a[(r, c)] - ref).max() <= 1e-9 * np.abs(Hinv).max()
        assert np.array_equal(a[(r, c)], b[(r, c)])


def _graph40():
    return GraphProblem.from_synth(make_graph(40, 8, seed=6), interleave=True)


@pytest.fixture(scope="module")
def marg40(gpu_lib):
    """make_graph(40, 8, seed=6) after six LM iterations on a single handle, and the dense inverse of the oracle's H at the downloaded
    estimates: the reference of the single-handle marginals tests below (tolerance 1e-6 |Hinv|.max(), the project's for marginals).  The
    tests only ask the handle for marginals; none moves its estimates."""
    from semantic_slam_amd import GraphSLAM
    gp = _graph40()
    G = GraphSLAM.from_problem(gp)
    G.optimize(6)
    gp.est[:] = G.estimates()
    U, _ = gp.linearize()
    return gp, G, np.linalg.inv((U + sp.triu(U, 1).T).toarray())


def test_marginals_of_a_single_handle_from_scratch_placement(marg40, monkeypatch):
    """Landmark and pose diagonals, a pose-pose pair, a pose-landmark pair both ways round and a landmark-landmark pair through
    computeMarginals, with Y in LDS and -- SSLAM_MARGINAL_LDS_BYTES=1, read on every call -- in the device scratch buffer, the placement
    of paths that LDS does not hold.  Both match the dense inverse and each other exactly (same body, same order of operations)."""
    gp, G, Hinv = marg40
    lm = [G.hessian_index(int(v)) for v in gp.lm_ids]
    po = {k: G.hessian_index(int(gp.pose_ids[k])) for k in (7, 39, 10, 30, 12)}
    pairs = [(h, h) for h in lm] + [(po[7], po[7]), (po[39], po[39]), (po[10], po[30]), (po[12], lm[3]), (lm[3], po[12]), (lm[0], lm[5])]
    in_lds = G.computeMarginals(pairs)
    monkeypatch.setenv("SSLAM_MARGINAL_LDS_BYTES", "1")
    in_scratch = G.computeMarginals(pairs)
    monkeypatch.delenv("SSLAM_MARGINAL_LDS_BYTES")
    assert {blk.shape for blk in in_lds.values()} == {(3, 3), (6, 6), (6, 3), (3, 6)}
    tol = 1e-6 * np.abs(Hinv).max()
    for (r, c) in pairs:
        a, s = in_lds[(r, c)], in_scratch[(r, c)]
        ref = Hinv[r:r + a.shape[0], c:c + a.shape[1]]
        print(f"block ({r}, {c}) shape {a.shape} max error LDS {np.abs(a - ref).max():.3e} scratch {np.abs(s - ref).max():.3e} bound {tol:.3e}")
        assert np.abs(a - ref).max() <= tol and np.abs(s - ref).max() <= tol
        assert np.array_equal(a, s)
    pl, lp = in_lds[(po[12], lm[3])], in_lds[(lm[3], po[12])]
    print(f"pose-landmark against transposed landmark-pose: max difference {np.abs(pl - lp.T).max():.3e}")
    assert pl.shape == (6, 3) and np.abs(pl - lp.T).max() <= tol


def test_marginals_of_a_single_handle_with_inactive_vertices(gpu_lib, marg40):
    """A fixed vertex in the list of computeLandmarkMarginals: zeros of its shape at its place, the other blocks as without it.  By
    hessian index there is no way to name it: a pair with an index that starts no active vertex is SSLAM_ERR_INVALID, nothing written."""
    import ctypes as C
    gp, G, Hinv = marg40
    lm, fixed, pose = [int(v) for v in gp.lm_ids], int(gp.pose_ids[0]), int(gp.pose_ids[5])
    assert G.hessian_index(fixed) < 0
    without = G.computeLandmarkMarginals(lm + [pose])
    blocks = G.computeLandmarkMarginals(lm[:3] + [fixed] + lm[3:] + [pose])
    assert blocks[3].shape == (6, 6) and np.all(blocks[3] == 0)
    rest = blocks[:3] + blocks[4:]
    assert len(rest) == len(without)
    tol = 1e-6 * np.abs(Hinv).max()
    for v, a, w in zip(lm + [pose], rest, without):
        h = G.hessian_index(v)
        assert np.array_equal(a, w)
        assert np.abs(a - Hinv[h:h + a.shape[0], h:h + a.shape[1]]).max() <= tol
    h0 = G.hessian_index(lm[0])
    for bad in ([h0, h0, h0 + 1, h0], [h0, h0, h0, Hinv.shape[0]], [-1, h0]):
        rc_pairs = np.ascontiguousarray(bad, np.int32)
        out = np.full(40, -7.0)
        rc = gpu_lib.sslam_graph_marginals_by_hessian_index(G._h, rc_pairs.ctypes.data_as(C.POINTER(C.c_int)), len(bad) // 2,
                                                            out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == -1                                                              # SSLAM_ERR_INVALID ...
        assert np.all(out == -7.0)                                                   # ... and nothing written, the good pair included


def test_marginals_do_not_depend_on_the_calls_before_them(marg40):
    """marginals, optimize(2), marginals on one handle against a fresh handle brought to the same estimates: the same bits.  The marginals
    call leaves the handle as any other call that linearises does -- the optimisation after it is the one of a handle that never made it."""
    from semantic_slam_amd import GraphSLAM
    gp, G, Hinv = marg40
    ids = [int(v) for v in gp.lm_ids] + [int(gp.pose_ids[k]) for k in (1, 20, 39)]
    A = GraphSLAM.from_problem(_graph40())
    A.optimize(6)
    first = A.computeLandmarkMarginals(ids)
    for a, r in zip(first, G.computeLandmarkMarginals(ids)):
        assert np.array_equal(a, r)
    A.optimize(2)
    second = A.computeLandmarkMarginals(ids)
    plain = GraphSLAM.from_problem(_graph40())
    plain.optimize(6)
    plain.optimize(2)
    assert np.array_equal(A.estimates(), plain.estimates())
    fresh = GraphSLAM.from_problem(_graph40())
    for v in range(gp.nv):
        fresh.set_estimate(v, A.estimate(v))
    for a, r in zip(second, fresh.computeLandmarkMarginals(ids)):
        assert np.array_equal(a, r)


def _optimize_variant(gp, iters, env, fused, spec=1):
    import os
    from semantic_slam_amd import GraphSLAM
    env = {"SSLAM_CHOL_OPTS": ",".join(f"{k}={v}" for k, v in env.items())} if env else {}   # plan options by field name (chol_plan.hpp CholOpts)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        G = GraphSLAM.from_problem(gp)
        G.set_option("fused_small_graph", fused)
        G.set_option("speculative_trials", spec)
        assert G.optimize(iters)          # the plan is built inside, under `env`
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k)
            else: os.environ[k] = v
    return G.last_stats.iterations, G.last_stats.trials, G.last_stats.chi2_after, G.estimates().copy()


def test_single_launch_solve_and_fused_steps_equal_the_stand_alone_kernels(gpu_lib):
    """Round 4's launch-count work on small batches, against the round-3 launch sequence:
    (s) opt-in for a single small graph ("speculative_trials"): the (up to ten) damping trials of an LM iteration side by side in the lanes of one
        k_chol_spec_round launch, which also replays the accept / reject sequence -> bitwise (a), same iteration AND trial counts;
    (a) Jacobian kernels + k_lm_begin_small + k_chol_flow (factor and both solves in one dependency-driven launch) + k_lm_end_small;
    (b) the same plan with the stand-alone LM kernels round the single-launch solve -> bitwise (a);
    (c) SSLAM_CHOL_OPTS flow=0: a launch per depth of the tree (other work-item cuts: same result up to rounding);
    and all of them equal the oracle."""
    for (n, m, kind, iters) in [(120, 24, "point", 40), (80, 16, "plane", 12), (300, 60, "point", 10)]:
        g = make_graph(n, m, seed=11, landmark_kind=kind)
        gp = GraphProblem.from_synth(g, interleave=True)
        sp = _optimize_variant(gp, iters, {}, 1, spec=1)      # adaptive: the lanes join after the first rejected trial of an iteration
        sp2 = _optimize_variant(gp, iters, {}, 1, spec=2)     # every round with all lanes
        a = _optimize_variant(gp, iters, {}, 1, spec=0)
        assert sp[:3] == a[:3] and np.array_equal(sp[3], a[3]), (sp[:3], a[:3])
        assert sp2[:3] == a[:3] and np.array_equal(sp2[3], a[3]), (sp2[:3], a[:3])
        b = _optimize_variant(gp, iters, {}, 0)
        c = _optimize_variant(gp, iters, {"flow": 0}, 0)
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3]), (a[:3], b[:3])
        st = gp.optimize(iters)
        for r in (a, c):
            assert abs(r[2] - st.chi2_after) <= 1e-8 * st.chi2_after
            assert np.abs(r[3] - gp.est).max() <= 1e-5 * np.abs(gp.est).max()
        gp = GraphProblem.from_synth(g, interleave=True)   # gp.optimize moved the estimates: fresh problem for the next size


def test_front_tables_through_every_launch_form(gpu_lib):
    """Round 6: the front tables (csrc/front_plan.hpp, front_kernels.hpp -- one blob of relative indices per workgroup, dense update matrices,
    team-factored diagonal blocks) are the default of batches >= 32 (covered by the batch tests against the oracle); forced onto a single small
    graph (front=1) they also run inside the dependency-driven launches: k_chol_flow, the speculative lanes, and a launch per depth.  Same
    iteration and trial counts as the record kernels, chi2 / estimates equal to the oracle's; bitwise repeatable."""
    for (n, m, kind, iters) in [(120, 24, "point", 12), (80, 16, "plane", 12), (300, 60, "point", 10)]:   # (before g2o's LM reaches its noise floor, where trial counts follow the last bit of H)
        g = make_graph(n, m, seed=13, landmark_kind=kind)
        gp = GraphProblem.from_synth(g, interleave=True)
        rec = _optimize_variant(gp, iters, {"front": 0}, 1, spec=0)
        fs = _optimize_variant(gp, iters, {"front": 1}, 1, spec=1)       # speculative lanes (k_chol_spec_round)
        fa = _optimize_variant(gp, iters, {"front": 1}, 1, spec=0)       # k_chol_flow with the LM halves
        fa2 = _optimize_variant(gp, iters, {"front": 1}, 1, spec=0)
        fc = _optimize_variant(gp, iters, {"front": 1, "flow": 0}, 0)    # a launch per depth (k_front_pieces / k_front_tail)
        assert fa[:3] == fa2[:3] and np.array_equal(fa[3], fa2[3])
        assert fs[:3] == fa[:3] and np.array_equal(fs[3], fa[3]), (fs[:3], fa[:3])
        st = gp.optimize(iters)
        for r in (rec, fa, fc):
            assert abs(r[2] - st.chi2_after) <= 1e-8 * st.chi2_after
            assert np.abs(r[3] - gp.est).max() <= 1e-5 * np.abs(gp.est).max()


def test_single_launch_solve_on_the_L_graph_and_a_small_batch(gpu_lib):
    """k_chol_flow with more pieces than workgroups (one 5000-pose graph: ~1500 pieces over a persistent grid, walked in rounds) and on a batch of four
    distinct graphs: same chi2 / estimates as the launch-per-depth path up to rounding."""
    import os
    from semantic_slam_amd import GraphSLAM, GraphBatch
    g = make_graph(5000, 1000, seed=2)
    gp = GraphProblem.from_synth(g)
    a = _optimize_variant(gp, 4, {"flow": 2}, 1)     # 2: the single launch over the whole wide tree (by default such a graph keeps its per-depth launches: measured faster)
    c = _optimize_variant(gp, 4, {"flow": 0}, 0)
    assert a[0] == c[0] and abs(a[2] - c[2]) <= 1e-9 * c[2]
    assert np.abs(a[3] - c[3]).max() <= 1e-7 * np.abs(c[3]).max()
    out = []
    for flow in (1, 0):
        os.environ["SSLAM_CHOL_OPTS"] = f"flow={flow}"
        try:
            graphs = [GraphSLAM.from_synth(make_graph(90 + 7 * k, 18 + k, seed=20 + k)) for k in range(4)]
            bt = GraphBatch(graphs); bt.upload()
            st = bt.optimize(15)
            bt.download()
        finally:
            os.environ.pop("SSLAM_CHOL_OPTS")
        out.append(([(int(s.iterations), float(s.chi2_after)) for s in st], [G.estimates().copy() for G in graphs]))
    for (ia, ca), (ib, cb) in zip(out[0][0], out[1][0]):
        assert abs(ca - cb) <= 1e-9 * cb
    for x, y in zip(out[0][1], out[1][1]):
        assert np.abs(x - y).max() <= 1e-6 * np.abs(y).max()


@pytest.mark.parametrize("kind", ["point", "plane"])
def test_golden_graph_through_g2o_loader(gpu_lib, kind):
    """Committed golden vectors (tests/golden/make_golden.py): .g2o file -> C-ABI loader -> HIP optimise."""
    import os
    from semantic_slam_amd import GraphSLAM
    gold = os.path.join(os.path.dirname(__file__), "golden")
    exp = np.load(os.path.join(gold, f"graph20_{kind}_expected.npz"))
    G = GraphSLAM(); G.load(os.path.join(gold, f"graph20_{kind}.g2o"))
    assert G.chi2() == pytest.approx(float(exp["chi2_before"]), rel=1e-12)
    U, b = G.linearize()
    tol = 1e-11 if kind == "point" else 2e-5
    assert np.abs(U.data - exp["H_upper_data"]).max() <= tol * np.abs(exp["H_upper_data"]).max()
    assert np.abs(b - exp["b"]).max() <= tol * np.abs(exp["b"]).max()
    assert G.optimize(25)
    assert G.last_stats.chi2_after == pytest.approx(float(exp["chi2_after"]), rel=1e-6)
    assert np.abs(G.estimates() - exp["estimates"]).max() <= 1e-4 * np.abs(exp["estimates"]).max()


def test_cpp_shim_end_to_end(gpu_lib, tmp_path):
    """The reference-named C++ classes (include/ps_graph_slam_amd/graph_slam.hpp, include/planar_segmentation_amd/
    point_cloud_segmentation.hpp) drive the GPU path: optimise + computeLandmarkMarginals with the reference's own argument
    (hessian-index pairs), and segmentallPointCloudData on a synthetic frame whose planes must equal the Python mirror's."""
    import os, re, subprocess
    from semantic_slam_amd import library_path
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    from semantic_slam_amd.synth import make_frame
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_check")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_compile_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    fr = make_frame(seed=1, n_boxes=12)
    seg = PointCloudSegmentation()
    planes = seg.segmentallPointCloudData(fr.robot_pose, fr.cam_angle, fr.boxes, fr)
    assert len(planes) > 0
    path = str(tmp_path / "frame.bin")
    with open(path, "wb") as f:
        np.array([fr.width, fr.height, fr.point_step, len(fr.boxes)], "<i4").tofile(f)
        for b in fr.boxes:
            np.array([b["tl_x"], b["tl_y"], b["width"], b["height"]], "<i4").tofile(f)
        np.concatenate([fr.robot_pose, [fr.cam_angle]]).astype("<f4").tofile(f)
        f.write(fr.cloud.tobytes())
    # the legacy k-means path of the shim (computeKmeans / clusterAndSegmentAllPlanes) on a floor + table + two walls scene
    rng = np.random.default_rng(4)

    def patch(n, origin, u, v, normal):
        ab = rng.uniform(0, 1, (n, 2))
        p = np.asarray(origin) + ab[:, :1] * np.asarray(u) + ab[:, 1:] * np.asarray(v) + rng.normal(0, 0.002, (n, 1)) * np.asarray(normal)
        return p.astype(np.float32), (np.asarray(normal) + rng.normal(0, 0.02, (n, 3))).astype(np.float32)
    parts = [patch(6000, [-1, -1, -1.0], [2.0, 0, 0], [0, 2.0, 0], [0, 0, 1.0]), patch(4000, [0.2, 0.2, -0.4], [0.8, 0, 0], [0, 0.6, 0], [0, 0, 1.0]),
             patch(5000, [1.5, -1, -1.0], [0, 2.0, 0], [0, 0, 1.5], [-1.0, 0, 0]), patch(5000, [-1, 1.5, -1.0], [2.0, 0, 0], [0, 0, 1.5], [0, -1.0, 0])]
    xyz = np.vstack([p for p, _ in parts]); nr = np.vstack([q for _, q in parts])
    nr[::97] = np.nan
    rows = seg.clusterAndSegmentAllPlanes(xyz, nr, np.eye(4, dtype=np.float32), seed=1)
    scene = str(tmp_path / "scene.bin")
    with open(scene, "wb") as f:
        np.array([len(xyz)], "<i4").tofile(f); xyz.astype("<f4").tofile(f); nr.astype("<f4").tofile(f)
    out = subprocess.run([exe, path, str(len(planes)), scene], capture_output=True, text=True)
    assert out.returncode == 0 and "shim ok: chi2" in out.stdout and "frontend shim ok" in out.stdout and "orchestrator shim ok" in out.stdout, out.stdout + out.stderr
    m = re.search(r"legacy shim ok: (\d+) rows rowsum (\S+)", out.stdout)
    assert m and int(m.group(1)) == len(rows) >= 6, out.stdout
    assert float(m.group(2)) == pytest.approx(float((rows.astype(np.float64) * np.arange(1, 9)).sum()), rel=1e-9)
    cs = sum(float(p.normal_orientation[0]) + 2.0 * float(p.normal_orientation[1]) + 3.0 * float(p.normal_orientation[2])
             + 0.5 * float(p.normal_orientation[3]) + float(p.num_points) for p in planes)
    got = float(re.search(r"checksum (\S+)", out.stdout).group(1))
    assert got == pytest.approx(cs, rel=1e-9)


def test_marginals_by_hessian_index_pairs(gpu_lib):
    """computeMarginals with (hessianIndex, hessianIndex) pairs as the reference builds them (semantic_graph_slam.cpp:186-191),
    including an off-diagonal pair, against the dense inverse of the oracle's H."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(40, 8, seed=6)
    gp = GraphProblem.from_synth(g, interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.optimize(6)
    gp.est[:] = G.estimates()
    U, _ = gp.linearize()
    Hinv = np.linalg.inv((U + sp.triu(U, 1).T).toarray())
    lm = [int(v) for v in gp.lm_ids]
    hi = [G.hessian_index(v) for v in lm]
    pose_h = G.hessian_index(int(gp.pose_ids[5]))
    pairs = [(h, h) for h in hi] + [(hi[0], hi[1]), (pose_h, hi[2])]
    blocks = G.computeMarginals(pairs)
    for (r, c), blk in blocks.items():
        ref = Hinv[r:r + blk.shape[0], c:c + blk.shape[1]]
        assert np.abs(blk - ref).max() <= 1e-6 * np.abs(Hinv).max()
    assert blocks[(pose_h, hi[2])].shape == (6, 3)


def test_marginals_L_config_sample(gpu_lib):
    """computeLandmarkMarginals at BASELINE scale: all 1000 landmark blocks in one call, one wave per block;
    a sample of them is checked against the oracle's Cholesky."""
    from semantic_slam_amd import GraphSLAM
    g = make_graph(5000, 1000, seed=1)
    gp = GraphProblem.from_synth(g)
    G = GraphSLAM.from_problem(gp)
    G.optimize(6)
    gp.est[:] = G.estimates()
    ids = [int(v) for v in gp.lm_ids]
    blocks = G.computeLandmarkMarginals(ids)
    assert len(blocks) == 1000
    sample = ids[::97]
    ref = gp.marginals(sample).reshape(-1, 3, 3)
    for v, r in zip(sample, ref):
        a = blocks[ids.index(v)]
        assert np.abs(a - r).max() <= 1e-6 * np.abs(r).max()
        assert np.linalg.eigvalsh(0.5 * (a + a.T)).min() > 0


def test_seg_golden_patch(gpu_lib):
    """Committed 96x72 golden patch: normals + label image from the HIP path, bit-exact."""
    import os
    from semantic_slam_amd.segmentation import PointCloudSegmentation, default_params
    from semantic_slam_amd.synth import BOX_DTYPE
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "patch96x72.npz"))
    w, h = 96, 72
    buf = np.zeros((h, w, 8), np.float32); buf[:, :, :3] = g["points"].reshape(h, w, 3)
    boxes = np.zeros(1, BOX_DTYPE); boxes["width"] = w; boxes["height"] = h; boxes["class_id"] = 1; boxes["prob"] = 1
    p = default_params(); p.num_point_seg = 100; p.norm_point_thres = 1000; p.image_width = w; p.image_height = h
    seg = PointCloudSegmentation(params=p)
    seg.segmentallPointCloudData(np.zeros(6, np.float32), 0.59, boxes, buf.reshape(-1).view(np.uint8), width=w, height=h,
                                 point_step=32, row_step=32 * w)
    assert np.array_equal(seg.normals(0).reshape(-1, 4), g["normals"], equal_nan=True)
    assert np.array_equal(seg.labels(0).reshape(-1), g["labels"])


def test_concurrent_handles_with_persistent_launches_equal_their_sequential_runs(gpu_lib):
    """Round-4 ADVICE: k_chol_flow / k_chol_spec_round are persistent grids sized for an otherwise free device; several graph handles (each
    with its own stream) driven from several host threads used to be able to leave each launch partly resident.  Persistent launches are now
    chained per device (PersistScope in sslam_chol.hip): four handles optimised concurrently give, bit for bit, what each gives alone.
    Round 6: the chain is a BUDGET -- launches whose grids together fit the device overlap, the others wait -- so four concurrent 100-pose
    optimisations must take less than twice one of them (round 5 ran them one at a time: four times)."""
    import threading, time
    from semantic_slam_amd import GraphSLAM
    gps = [GraphProblem.from_synth(make_graph(100 + 15 * k, 20 + 3 * k, seed=40 + k), interleave=True) for k in range(4)]
    alone = []
    for gp in gps:
        G = GraphSLAM.from_problem(gp)
        assert G.optimize(30)
        alone.append((G.last_stats.iterations, G.last_stats.trials, G.last_stats.chi2_after, G.estimates().copy()))
    for rep in range(2):
        Gs = [GraphSLAM.from_problem(gp) for gp in gps]
        ok = [False] * len(Gs)

        def run(k):
            ok[k] = bool(Gs[k].optimize(30))
        th = [threading.Thread(target=run, args=(k,)) for k in range(len(Gs))]
        for t in th: t.start()
        for t in th: t.join()
        assert all(ok)
        for G, ref in zip(Gs, alone):
            assert (G.last_stats.iterations, G.last_stats.trials, G.last_stats.chi2_after) == ref[:3]
            assert np.array_equal(G.estimates(), ref[3])
    # timing: the same 100-pose graph in four handles, warm (plans built, clocks up), best of three
    gp = GraphProblem.from_synth(make_graph(100, 20, seed=44), interleave=True)

    def timed(n_handles):
        best = 1e9
        for rep in range(3):
            Gs = [GraphSLAM.from_problem(gp) for _ in range(n_handles)]
            for G in Gs:
                G.set_option("speculative_trials", 0)     # the plain single-launch solve: a tenth of the device per handle (ten lanes would fill it)
                assert G.optimize(2)                       # plan + first launches outside the timed part
            th = [threading.Thread(target=lambda G=G: G.optimize(40)) for G in Gs]
            t0 = time.perf_counter()
            for t in th: t.start()
            for t in th: t.join()
            best = min(best, time.perf_counter() - t0)
        return best
    one, four = timed(1), timed(4)
    assert four < 2.0 * one, (one, four)
