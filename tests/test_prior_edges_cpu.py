"""Position priors (hdl_graph_slam's EdgeSE3PriorXY / EdgeSE3PriorXYZ; reference graph_slam.hpp:115-126, graph_slam.cpp:31-32, both
commented out there) on a box without a GPU: the host bookkeeping of the C-ABI, the g2o text rows, the analytic Jacobian against g2o's
numeric one, and the C++ shim's factories."""
import os
import subprocess

import numpy as np
import pytest

from oracle.np_graph import pose_oplus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose(t, rotvec):
    from semantic_slam_amd.synth import quat_from_rotvec
    return np.concatenate([np.asarray(t, float), quat_from_rotvec(np.asarray(rotvec, float))])


def test_prior_bookkeeping(hip_lib):
    from semantic_slam_amd import GraphSLAM, SslamError
    G = GraphSLAM()
    a = G.add_se3_node(_pose([0, 0, 0], [0, 0, 0]))
    b = G.add_se3_node(_pose([1, 0, 0], [0, 0, 0.3]))
    p = G.add_point_xyz_node([1.0, 2.0, 3.0])
    c = G.add_se3_node(_pose([2, 1, 0], [0.1, 0, 0]))          # owns nothing but a prior below
    e0 = G.add_se3_edge(a, b, _pose([1, 0, 0], [0, 0, 0.3]), np.eye(6))
    e1 = G.add_se3_prior_xyz_edge(b, [1.0, 0.1, 0.0], np.diag([4.0, 4.0, 1.0]))
    e2 = G.add_se3_point_xyz_edge(b, p, [0.5, 2.0, 3.0], np.eye(3))
    W2 = np.array([[4.0, 0.5], [0.5, 2.0]])
    e3 = G.add_se3_prior_xy_edge(b, [1.0, 0.0], W2)
    assert (e0, e1, e2, e3) == (0, 1, 2, 3)                      # one counter for binary and unary edges
    assert G.num_edges() == 4 and G.num_vertices() == 4
    assert G.hessian_index(c) == -1                              # no edge yet: inactive, as in g2o
    assert G.add_se3_prior_xyz_edge(c, [2.0, 1.0, 0.0], np.eye(3)) == 4
    # the first pose is fixed; b, p by id; c is active through its prior alone
    assert [G.hessian_index(v) for v in (a, b, p, c)] == [-1, 0, 6, 9]
    # a prior on the fixed first pose changes nothing in the ordering
    assert G.add_se3_prior_xy_edge(a, [0.0, 0.0], np.eye(2)) == 5
    assert [G.hessian_index(v) for v in (a, b, p, c)] == [-1, 0, 6, 9]
    with pytest.raises(SslamError):
        G.add_se3_prior_xyz_edge(p, [0, 0, 0], np.eye(3))         # a point vertex is not a VertexSE3
    with pytest.raises(SslamError):
        G.add_se3_prior_xy_edge(7, [0, 0], np.eye(2))             # no such vertex
    with pytest.raises(SslamError):
        G.add_se3_prior_xy_edge(-1, [0, 0], np.eye(2))
    with pytest.raises(SslamError):
        G.add_se3_prior_xy_edge(b, [0, 0], np.array([[1.0, 0.3], [0.0, 1.0]]))          # not symmetric
    with pytest.raises(SslamError):
        G.add_se3_prior_xyz_edge(b, [0, 0, 0], np.diag([1.0, np.inf, 1.0]))            # not finite
    assert G.num_edges() == 6                                     # refused edges leave no trace


def test_prior_graph_of_ten_edges_is_not_refused_on_the_host(hip_lib):
    """g2o counts graph->edges() for the < 10 rule (graph_slam.cpp:184-186): priors count.  Nine EdgeSE3 + one prior = 10."""
    from semantic_slam_amd import GraphSLAM, SslamError
    G = GraphSLAM()
    a = G.add_se3_node(_pose([0, 0, 0], [0, 0, 0])); b = G.add_se3_node(_pose([1, 0, 0], [0, 0, 0]))
    for _ in range(9):
        G.add_se3_edge(a, b, _pose([1, 0, 0], [0, 0, 0]), np.eye(6))
    assert G.optimize() is False and G.last_stats.status == -5
    G.add_se3_prior_xy_edge(b, [1.0, 0.0], np.eye(2))
    if hip_lib.sslam_device_count() == 0:
        with pytest.raises(SslamError) as ei:                     # past the edge count: the device is what is missing now
            G.optimize()
        assert ei.value.code == -2


G2O_TEXT = """PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1
VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1
FIX 0
VERTEX_SE3:QUAT 1 1 0.25 0 0 0 0.19866933079506122 0.98006657784124163
VERTEX_SE3:QUAT 2 2 0.5 0.125 0 0 0 1
EDGE_SE3:QUAT 0 1 1 0.25 0 0 0 0.19866933079506122 0.98006657784124163 100 0 0 0 0 0 100 0 0 0 0 100 0 0 0 10000 0 0 10000 0 10000
EDGE_SE3:QUAT 1 2 1 0.25 0.125 0 0 0 1 100 0 0 0 0 0 100 0 0 0 0 100 0 0 0 10000 0 0 10000 0 10000
EDGE_SE3_PRIORXYZ 2 2.0499999999999998 0.5 0.10000000000000001 4 0.5 0 4 0 1
EDGE_SE3_PRIORXY 1 0.97999999999999998 0.25 4 -0.25 2
EDGE_SE3_PRIORXY 2 2 0.5 1 0 1
"""


def test_g2o_rows_with_priors_load_and_save_back(hip_lib, tmp_path):
    """EDGE_SE3_PRIORXYZ / EDGE_SE3_PRIORXY rows (hdl_graph_slam's read / write: vertex, z, upper triangle of Omega) load as priors --
    before they were skipped as unknown rows and the graph lost them -- and save back to the same text."""
    from semantic_slam_amd import GraphSLAM
    path = tmp_path / "prior.g2o"
    path.write_text(G2O_TEXT)
    G = GraphSLAM(); G.load(str(path))
    assert G.num_vertices() == 3 and G.num_edges() == 5
    assert [G.hessian_index(v) for v in range(3)] == [-1, 0, 6]
    out = tmp_path / "prior_out.g2o"
    G.save(str(out))
    assert out.read_text() == G2O_TEXT
    # the same graph through the API saves to the same text
    H = GraphSLAM()
    H.add_se3_node([0, 0, 0, 0, 0, 0, 1], fixed=1)
    H.add_se3_node([1, 0.25, 0, 0, 0, 0.19866933079506122, 0.98006657784124163], fixed=0)
    H.add_se3_node([2, 0.5, 0.125, 0, 0, 0, 1], fixed=0)
    W6 = np.diag([100.0, 100, 100, 1e4, 1e4, 1e4])
    H.add_se3_edge(0, 1, [1, 0.25, 0, 0, 0, 0.19866933079506122, 0.98006657784124163], W6)
    H.add_se3_edge(1, 2, [1, 0.25, 0.125, 0, 0, 0, 1], W6)
    H.add_se3_prior_xyz_edge(2, [2.05, 0.5, 0.1], [[4, 0.5, 0], [0.5, 4, 0], [0, 0, 1]])
    H.add_se3_prior_xy_edge(1, [0.98, 0.25], [[4, -0.25], [-0.25, 2]])
    H.add_se3_prior_xy_edge(2, [2, 0.5], np.eye(2))
    out2 = tmp_path / "api.g2o"
    H.save(str(out2))
    assert out2.read_text() == G2O_TEXT


def test_unknown_g2o_rows_are_still_skipped(hip_lib, tmp_path):
    from semantic_slam_amd import GraphSLAM
    path = tmp_path / "unknown.g2o"
    path.write_text(G2O_TEXT + "EDGE_SE3_PRIORQUAT 2 0 0 0 1 1 0 0 0 1 0 0 1 0 1\n")
    G = GraphSLAM(); G.load(str(path))
    assert G.num_edges() == 5


def test_analytic_prior_jacobian_matches_g2o_central_differences():
    """Upstream defines no linearizeOplus: g2o differentiates the error numerically, central differences with delta 1e-9 through
    VertexSE3::oplus.  The analytic [R | 0] the device uses agrees to the rounding of those differences, ~|t| eps / delta: ~1e-6 at the
    |t| ~ 20 m drawn here."""
    from prior_ref import prior_error_jac
    rng = np.random.default_rng(4)
    delta = 1e-9
    for k in range(50):
        X = _pose(rng.uniform(-20, 20, 3), rng.normal(0, 1.0, 3))
        for d in (2, 3):
            z = X[:d] + rng.normal(0, 0.5, d)
            e, J = prior_error_jac(X, z)
            Jn = np.zeros((d, 6))
            for c in range(6):
                dv = np.zeros(6); dv[c] = delta
                ep = pose_oplus(X, dv)[:d] - z
                em = pose_oplus(X, -dv)[:d] - z
                Jn[:, c] = (ep - em) / (2 * delta)
            assert np.abs(J - Jn).max() <= 1e-5, (k, d, np.abs(J - Jn).max())
            assert np.array_equal(J[:, 3:], np.zeros((d, 3)))


def test_prior_shim_compiles_and_links(hip_lib, tmp_path):
    from semantic_slam_amd import library_path
    exe = str(tmp_path / "shim_prior")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "shim_prior_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shim prior ok" in out.stdout
