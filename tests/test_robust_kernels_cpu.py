"""Per-edge robust kernels on a box without a GPU: the formula table (tests/robust_ref.py) pinned by rho1 = d rho0 / d e2, DCS pinned by
the oracle's, the host bookkeeping of the C-ABI (set / get, refusals, save / load, hessian indices) and the C++ shim's add_robust_kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import robust_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", [R.HUBER, R.PSEUDOHUBER, R.CAUCHY, R.WELSCH, R.FAIR, R.SATURATED])
@pytest.mark.parametrize("d", [0.5, 1.0, 3.0])
def test_rho1_is_the_derivative_of_rho0(kind, d):
    # both sides of d^2, the kink itself left out
    e2 = d * d * np.array([0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.1, 1.5, 3.0, 10.0, 50.0])
    h = 1e-6 * e2
    r0, r1 = R.rho(kind, d, e2)
    num = (R.rho(kind, d, e2 + h)[0] - R.rho(kind, d, e2 - h)[0]) / (2 * h)
    # central differences with step h = 1e-6 e2 >= 1e-7 d^2: truncation ~h^2 ~ 1e-12; rounding: rho0 is a difference of terms of size
    # ~d^2 (sqrt(1 + x) - 1, a - log1p(a)), each good to a few ulp ~ 1e-15 d^2, so the quotient is good to 1e-15 d^2 / 1e-7 d^2 = 1e-8
    assert np.abs(num - r1).max() <= 1e-8
    assert np.all(r0 <= e2 * (1 + 1e-15))
    assert np.all((r1 >= 0) & (r1 <= 1))
    if kind in (R.HUBER, R.SATURATED):
        assert np.all(r1[e2 < d * d] == 1.0) and np.all(r1[e2 > d * d] < 1.0)
    tiny = d * d * 1e-12
    t0, t1 = R.rho(kind, d, tiny)
    assert t0 == pytest.approx(tiny, rel=1e-5) and t1 == pytest.approx(1.0, abs=1e-5)


def test_kind_none_is_plain_least_squares():
    e2 = np.array([0.0, 0.5, 7.0])
    r0, r1 = R.rho(R.NONE, 1.0, e2)
    assert np.array_equal(r0, e2) and np.all(r1 == 1.0)


def test_dcs_equals_the_oracle(hip_lib):
    """kind 7 on every landmark edge == the oracle's global DCS (g2o::RobustKernelDCS) on a small graph"""
    from oracle import oracle as O
    from oracle.oracle import GraphProblem
    from semantic_slam_amd.synth import make_graph
    g = make_graph(40, 8, seed=2, noise_scale=4.0)
    gp = GraphProblem.from_synth(g)
    ref = R.NpRobustGraph(g)
    for k in range(ref.Eo, ref.Eo + ref.El):
        ref.set_kernel(k, R.DCS, 1.0)
    try:
        O.set_dcs(1.0)
        chi = gp.chi2()
    finally:
        O.set_dcs(0.0)
    e2, r0, r1 = ref.edge_chi2()
    assert np.count_nonzero(r1[ref.Eo:] < 1) > 0 and np.count_nonzero(r1[ref.Eo:] == 1) > 0
    assert ref.chi2() == pytest.approx(chi, rel=1e-12)
    assert R.NpRobustGraph(g, dcs_phi=1.0).chi2() == pytest.approx(chi, rel=1e-12)


def _pose(t, rotvec=(0, 0, 0)):
    from semantic_slam_amd.synth import quat_from_rotvec
    return np.concatenate([np.asarray(t, float), quat_from_rotvec(np.asarray(rotvec, float))])


def _six_edge_graph():
    """one edge of each of the six edge types; returns (graph, edge ids)"""
    from semantic_slam_amd import GraphSLAM
    G = GraphSLAM()
    a = G.add_se3_node(_pose([0, 0, 0])); b = G.add_se3_node(_pose([1, 0, 0], [0, 0, 0.2]))
    p = G.add_point_xyz_node([1.0, 2.0, 3.0]); q = G.add_point_xyz_node([2.0, 2.0, 3.0])
    pl = G.add_plane_node([0.0, 0.0, 1.0, -1.0])
    ids = [G.add_se3_edge(a, b, _pose([1, 0, 0], [0, 0, 0.2]), np.eye(6)),
           G.add_se3_point_xyz_edge(b, p, [0.5, 2.0, 3.0], np.eye(3)),
           G.add_se3_plane_edge(b, pl, [0.0, 0.0, 1.0, -1.0], np.eye(3)),
           G.add_point_xyz_point_xyz_edge(p, q, [1.0, 0.0, 0.0], np.eye(3)),
           G.add_se3_prior_xy_edge(b, [1.0, 0.0], np.eye(2)),
           G.add_se3_prior_xyz_edge(b, [1.0, 0.0, 0.0], np.eye(3))]
    return G, ids


def test_set_get_round_trip_on_every_edge_type(hip_lib):
    from semantic_slam_amd.graph_slam import ROBUST_KERNELS
    G, ids = _six_edge_graph()
    assert ids == list(range(6))
    hidx = [G.hessian_index(v) for v in range(G.num_vertices())]
    assert all(G.edge_robust_kernel(e) == ("NONE", 0.0) for e in ids)
    names = list(ROBUST_KERNELS)
    assert names == R.NAMES and [ROBUST_KERNELS[n] for n in names] == list(range(8))
    for k, e in enumerate(ids):
        G.add_robust_kernel(e, names[1 + k], 0.25 * (k + 1))
    for k, e in enumerate(ids):
        assert G.edge_robust_kernel(e) == (names[1 + k], 0.25 * (k + 1))
    G.add_robust_kernel(ids[0], "DCS", 2.0)
    assert G.edge_robust_kernel(ids[0]) == ("DCS", 2.0)
    G.add_robust_kernel(ids[0], "NONE", 5.0)                       # removes the kernel; the width is not kept
    assert G.edge_robust_kernel(ids[0]) == ("NONE", 0.0)
    assert [G.hessian_index(v) for v in range(G.num_vertices())] == hidx     # kernels are values, not structure
    assert G.num_edges() == 6


def test_invalid_arguments_are_refused_and_leave_the_graph_untouched(hip_lib):
    from semantic_slam_amd import SslamError
    G, ids = _six_edge_graph()
    G.add_robust_kernel(ids[1], "Cauchy", 1.5)
    lib, h = G._lib, G._h
    before = [G.edge_robust_kernel(e) for e in ids]
    bad = [(ids[1], -1, 1.0), (ids[1], 8, 1.0), (ids[1], 1, 0.0), (ids[1], 1, -2.0), (ids[1], 3, float("nan")), (ids[1], 4, float("inf")),
           (-1, 1, 1.0), (6, 1, 1.0), (1 << 20, 0, 0.0)]
    for e, kind, d in bad:
        assert lib.sslam_graph_set_edge_robust_kernel(h, e, kind, d) == -1      # SSLAM_ERR_INVALID
        assert [G.edge_robust_kernel(x) for x in ids] == before
    assert lib.sslam_graph_set_edge_robust_kernel(None, 0, 1, 1.0) == -1
    kind, d = C.c_int(-7), C.c_double(-7.0)
    for e in (-1, 6):
        assert lib.sslam_graph_get_edge_robust_kernel(h, e, C.byref(kind), C.byref(d)) == -1
        assert kind.value == -7 and d.value == -7.0
    assert lib.sslam_graph_get_edge_robust_kernel(h, ids[1], None, None) == 0     # outputs are optional
    with pytest.raises(ValueError):
        G.add_robust_kernel(ids[0], "Tukey", 1.0)                   # left out on purpose (include/sslam.h)
    with pytest.raises(SslamError):
        G.add_robust_kernel(ids[0], "Huber", 0.0)
    with pytest.raises(SslamError):
        G.edge_chi2([99])                                           # refused on the host, before any device work
    assert [G.edge_robust_kernel(x) for x in ids] == before


def test_symbols_and_constants(hip_lib):
    for name in ("sslam_graph_set_edge_robust_kernel", "sslam_graph_get_edge_robust_kernel", "sslam_graph_edge_chi2"):
        assert getattr(hip_lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "sslam.h")).read()
    for k, n in enumerate(["NONE", "HUBER", "PSEUDOHUBER", "CAUCHY", "WELSCH", "FAIR", "SATURATED", "DCS"]):
        assert f"#define SSLAM_ROBUST_{n} {k}\n" in hdr
    assert "GemanMcClure" in hdr and "Tukey" in hdr


def test_save_drops_kernels_and_load_yields_none(hip_lib, tmp_path):
    from semantic_slam_amd import GraphSLAM
    G, ids = _six_edge_graph()
    plain = str(tmp_path / "plain.g2o"); rob = str(tmp_path / "robust.g2o")
    G.save(plain)
    for k, e in enumerate(ids):
        G.add_robust_kernel(e, R.NAMES[2 + k], 1.0 + k)
    G.save(rob)
    assert open(plain).read() == open(rob).read()                   # no new rows, no new columns
    G2 = GraphSLAM()
    G2.load(rob)
    assert G2.num_edges() == 6 and all(G2.edge_robust_kernel(e) == ("NONE", 0.0) for e in range(6))


def test_cpp_shim_add_robust_kernel_compiles_and_links(hip_lib, tmp_path):
    from semantic_slam_amd import library_path
    exe = str(tmp_path / "robust_shim_check")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "robust_shim_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "robust shim ok" in out.stdout
