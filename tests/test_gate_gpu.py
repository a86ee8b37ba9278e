"""sslam_batch_gate / sslam_graph_gate on the GPU: the Mahalanobis distance d2 = e^T S^-1 e of candidate edges that are not in the graph, one
wave per candidate (k_chol_gate_pairs).  Reference: tests/gate_ref.py (the dense inverse of the oracle's H at the downloaded estimates, the
NumPy error and Jacobians).
Tolerances, derived and not tuned: S at 1e-6 of max|S_ref| (the bar the marginals tests hold against the same dense inverse), e at 1e-11
(the linearisation parity of DESIGN.md row a4), d2 at 1e-6 * cond(S_ref) relative (a relative error of 1e-6 in S moves S^-1 e by that much
times the condition number).  Every candidate has cond(S_ref) <= 1e4, which the tests assert; they print the errors actually seen."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gate_ref import (OMEGA6, POSE_PAIRS, assemble, dense_inverse, error_jac, gate_ref, perturbed, point_candidate,
                      pose_candidate, relative_pose)
from oracle.oracle import GraphProblem
from semantic_slam_amd.synth import make_graph

pytestmark = pytest.mark.gpu

TOL_S, TOL_E, TOL_D2, MAX_COND = 1e-6, 1e-11, 1e-6, 1e4


def _check_against_ref(gp, Hinv, cand, d2, e, S, what):
    rd2, re_, rS, cond = gate_ref(gp, Hinv, *cand[1:])
    err_s, err_e, err_d = np.abs(S - rS).max() / np.abs(rS).max(), np.abs(e - re_).max(), abs(d2 - rd2) / abs(rd2)
    print(f"{what} {cand[1]} ({cand[2]}, {cand[3]}) info {'yes' if cand[5] is not None else 'no'}: d2 {d2:.6g} ref {rd2:.6g} rel err {err_d:.3e} "
          f"(bound {TOL_D2 * cond:.3e}) | cond(S) {cond:.3e} | S rel err {err_s:.3e} | e abs err {err_e:.3e}")
    assert cond <= MAX_COND
    assert S.shape == rS.shape and e.shape == re_.shape
    assert err_s <= TOL_S, what
    assert err_e <= TOL_E, what
    assert err_d <= TOL_D2 * cond, what


def _candidates(gp, g):
    """per graph: the four pose pairs (the fixed pose 0 and the adjacent poses 1, 2 among them), two pose -> landmark candidates and one
    candidate without an information matrix"""
    return ([pose_candidate(gp, g, a, b) for a, b in POSE_PAIRS] + [point_candidate(gp, g, 12, 3), point_candidate(gp, g, 0, 5)]
            + [pose_candidate(gp, g, 10, 30, info=None)])


def _with_env(name, value, f):
    """f() with the variable set (None: as it is); the library reads both per call"""
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = str(value)
    try:
        return f()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _with_lds_budget(nbytes, f):
    return _with_env("SSLAM_MARGINAL_LDS_BYTES", nbytes, f)


def _same(a, b):
    """bitwise, NaN included"""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def three(gpu_lib):
    """three distinct graphs, two LM iterations in one batch, the estimates downloaded, the candidates of every graph in one gate call"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=s), interleave=True) for s in (4, 5, 6)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    B.upload()
    B.optimize(2)
    B.download()
    cand = []
    for g, gp in enumerate(gps):
        gp.est[:] = graphs[g].estimates()
        cand += _candidates(gp, g)
    d2, e, S = B.gate(cand, return_cov=True)
    return gps, graphs, B, cand, (d2, e, S)


def test_three_distinct_graphs_match_the_reference(three):
    gps, graphs, B, cand, (d2, e, S) = three
    Hinv = [dense_inverse(gp) for gp in gps]
    assert d2.shape == (len(cand),) and len(e) == len(S) == len(cand)
    assert {s.shape for s in S} == {(6, 6), (3, 3)}
    for k, c in enumerate(cand):
        _check_against_ref(gps[c[0]], Hinv[c[0]], c, d2[k], e[k], S[k], f"graph {c[0]}")
    assert np.array_equal(B.gate(cand), d2)                      # without e and S: the same distances


def test_consistent_with_the_librarys_own_marginals(three):
    """S assembled on the host from B.marginals blocks and the NumPy Jacobians: both come from the same factor, so 1e-9 relative"""
    gps, graphs, B, cand, (d2, e, S) = three
    blocks = iter(B.marginals([rq for g, _, vu, vv, _, _ in cand for rq in ((g, vu, vu), (g, vu, vv), (g, vv, vv))]))
    for k, (g, kind, vu, vv, z, info) in enumerate(cand):
        Zuu, Zuv, Zvv = next(blocks), next(blocks), next(blocks)
        re_, Ju, Jv = error_jac(gps[g].est, kind, vu, vv, z)
        rS, rd2, cond = assemble(re_, Ju, Jv, Zuu, Zuv, Zvv, info)
        err = np.abs(S[k] - rS).max() / np.abs(rS).max()
        print(f"graph {g} {kind} ({vu}, {vv}): S rel err {err:.3e}, d2 {d2[k]:.6g} host {rd2:.6g}")
        assert err <= 1e-9


def test_placements_agree_bitwise(three):
    """SSLAM_MARGINAL_LDS_BYTES = 1: every candidate out of its scratch slice.  A budget of the fixed area + 16 + 308 bytes per path
    entry for a few entries holds a candidate with one path (a fixed end) and not one with two: both launches in one call."""
    gps, graphs, B, cand, first = three
    again = B.gate(cand, return_cov=True)
    scratch = _with_lds_budget(1, lambda: B.gate(cand, return_cov=True))
    for a, b, c in zip(first, again, scratch):
        assert _same(a, b) and _same(a, c)
    for entries in (0, 4, 8, 16, 24, 32):
        mixed = _with_lds_budget(296 * 8 + 16 + 308 * entries, lambda: B.gate(cand, return_cov=True))
        for a, c in zip(first, mixed):
            assert _same(a, c)


def test_quaternion_sign(three):
    gps, graphs, B, cand, (d2, e, S) = three
    flipped = [(g, kind, vu, vv, np.concatenate([z[:3], -z[3:]]) if kind == "se3" else z, info) for g, kind, vu, vv, z, info in cand]
    assert sum(c[1] == "se3" for c in cand) == 15
    f2, fe, fS = B.gate(flipped, return_cov=True)
    assert np.array_equal(f2, d2) and _same(fe, e) and _same(fS, S)


@pytest.fixture(scope="module")
def fixed_ends(gpu_lib):
    """a graph with two fixed poses, and candidates with one or both ends at them"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gp = GraphProblem.from_synth(make_graph(40, 8, seed=4), interleave=True)
    f0, f1 = int(gp.pose_ids[0]), int(gp.pose_ids[20])
    gp.vfixed[f1] = 1
    G = GraphSLAM.from_problem(gp)                               # add_se3_node(..., fixed=1) for both
    assert G.hessian_index(f0) == -1 and G.hessian_index(f1) == -1
    B = GraphBatch([G])
    B.upload()
    B.optimize(2)
    B.download()
    gp.est[:] = G.estimates()
    both = pose_candidate(gp, 0, 0, 20)
    cand = [both, both[:5] + (None,), pose_candidate(gp, 0, 20, 30), pose_candidate(gp, 0, 31, 0), point_candidate(gp, 0, 20, 3),
            pose_candidate(gp, 0, 0, 39, info=None)]
    return gp, B, both, cand, B.gate(cand, return_cov=True)


def test_zero_length_paths(fixed_ends):
    """two fixed poses: a candidate between them has no path on either side (S = Omega^-1, d2 = e^T Omega e; without Omega S = 0 and d2 is
    NaN with the call succeeding); a candidate with one fixed end matches the reference with that end's blocks zero"""
    gp, B, both, cand, (d2, e, S) = fixed_ends
    re_ = error_jac(gp.est, "se3", both[2], both[3], both[4])[0]
    want = float(re_ @ OMEGA6 @ re_)
    print(f"both ends fixed: d2 {d2[0]:.17g} e^T Omega e {want:.17g} rel err {abs(d2[0] - want) / want:.3e}")
    assert abs(d2[0] - want) <= 1e-11 * want
    assert np.abs(S[0] * OMEGA6 - np.eye(6)).max() <= 8 * np.finfo(float).eps      # a square root and two divisions per diagonal entry
    assert np.isnan(d2[1]) and np.all(S[1] == 0) and np.array_equal(e[1], e[0])
    Hinv = dense_inverse(gp)
    for k in (2, 3, 4, 5):
        _check_against_ref(gp, Hinv, cand[k], d2[k], e[k], S[k], "one fixed end")
    for lds in (1, 296 * 8 + 16):                                # the same in scratch, and with LDS for the fixed area alone
        assert all(_same(a, b) for a, b in zip((d2, e, S), _with_lds_budget(lds, lambda: B.gate(cand, return_cov=True))))


def test_rounds_agree_bitwise(three, fixed_ends):
    """SSLAM_PATH_ROUND_INTS cuts a call into rounds of candidates (each its own upload, launches, download and scatter): at 1 every
    candidate with a column is a round, at 64 a round takes a few; d2, e and S are those of the one-round call, NaN included.  With the
    default budget (every path in LDS), and with a budget of 8 path entries that puts both placements into one round.  The candidates
    with fixed ends add records without columns, which do not close a round."""
    _, _, B3, cand3, first3 = three
    _, B1, _, cand1, first1 = fixed_ends
    assert np.isnan(first1[0][1])
    for B, cand, first in ((B3, cand3, first3), (B1, cand1, first1)):
        for budget in (None, 2368 + 16 + 308 * 8):
            for ints in (1, 64):
                got = _with_env("SSLAM_PATH_ROUND_INTS", ints, lambda: _with_lds_budget(budget, lambda: B.gate(cand, return_cov=True)))
                assert all(_same(a, c) for a, c in zip(first, got)), (len(cand), budget, ints)


def test_batch_of_one_against_the_single_graph_handle(gpu_lib):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gp = GraphProblem.from_synth(make_graph(40, 8, seed=6), interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.optimize(4)
    gp.est[:] = G.estimates()
    Hinv = dense_inverse(gp)
    cand = _candidates(gp, 0)
    M = GraphSLAM.from_problem(gp)
    for v in range(gp.nv):
        M.set_estimate(v, G.estimate(v))
    B = GraphBatch([M])
    B.upload()
    d2, e, S = B.gate(cand, return_cov=True)
    for k, c in enumerate(cand):
        one = (G.gate_se3 if c[1] == "se3" else G.gate_point)(c[2], c[3], c[4], c[5])
        assert one == d2[k], f"candidate {k}: handle {one!r} batch of one {d2[k]!r}"
        _check_against_ref(gp, Hinv, c, d2[k], e[k], S[k], "batch of one")


def test_front_kernel_family(gpu_lib):
    """32 graphs: the flat factor the gate reads is written by the front kernels (see tests/test_batch_marginals_gpu.py)"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=700 + k), interleave=bool(k & 1)) for k in range(32)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    assert B.info("factor_front") == 1
    B.upload()
    B.optimize(2)
    B.download()
    cand = []
    for g in (0, 15, 31):
        gps[g].est[:] = graphs[g].estimates()
        cand += _candidates(gps[g], g)
    d2, e, S = B.gate(cand, return_cov=True)
    Hinv = {g: dense_inverse(gps[g]) for g in (0, 15, 31)}
    for k, c in enumerate(cand):
        _check_against_ref(gps[c[0]], Hinv[c[0]], c, d2[k], e[k], S[k], f"graph {c[0]}")


def test_stream_group(gpu_lib):
    """the parts of a stream group hold two graphs each, the plain batch four: every graph is ordered and factored on its own, so the
    results are the plain batch's bitwise (the argument of tests/test_batch_marginals_gpu.py::test_contract_edges)"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=s), interleave=True) for s in (4, 5, 6, 7)]
    cand = [c for g in (3, 0, 2, 1, 3) for c in _candidates(gps[g], g)]
    one = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps])
    one.upload()
    grp = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps], streams=2)
    assert grp.info("streams") == 2
    grp.upload()
    for a, b in zip(one.gate(cand, return_cov=True), grp.gate(cand, return_cov=True)):
        assert _same(a, b)


def test_no_side_effects(gpu_lib):
    """optimize(2), gate, optimize(3), marginals, download against the same without the gate call: statistics, blocks, estimates bitwise"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    runs = []
    for with_gate in (True, False):
        gps = [GraphProblem.from_synth(make_graph(40 + 6 * k, 8 + k, seed=50 + k), interleave=bool(k & 1)) for k in range(3)]
        graphs = [GraphSLAM.from_problem(gp) for gp in gps]
        B = GraphBatch(graphs)
        B.upload()
        s1 = B.optimize(2)
        if with_gate:
            cand = [c for g, gp in enumerate(gps) for c in _candidates(gp, g)]
            assert len(B.gate(cand)) == len(cand)
            _with_lds_budget(1, lambda: B.gate(cand))
        s2 = B.optimize(3)
        blocks = B.marginals([(g, int(gp.lm_ids[1]), int(gp.pose_ids[9])) for g, gp in enumerate(gps)])
        B.download()
        stats = [(s.iterations, s.trials, s.status, s.host_plan_us, s.chi2_before, s.chi2_after, s.lambda_, s.solver_iterations) for s in s1 + s2]
        runs.append((stats, blocks + [G.estimates() for G in graphs]))
    assert runs[0][0] == runs[1][0]
    assert _same(runs[0][1], runs[1][1])


def _raw(lib, handle, fn, cand, z, info, n, outs):
    dp = C.POINTER(C.c_double)
    cand = np.ascontiguousarray(cand, np.int32).reshape(-1)
    z, info = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (z, info)]
    return getattr(lib, fn)(handle, cand.ctypes.data_as(C.POINTER(C.c_int32)) if cand.size else None,
                            *[None if a is None else a.ctypes.data_as(dp) for a in (z, info)], n,
                            *[None if o is None else o.ctypes.data_as(dp) for o in outs])


def test_contract(gpu_lib):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=s), interleave=True) for s in (4, 5)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    B.upload()
    gp = gps[1]
    p0, p1, lm = int(gp.pose_ids[3]), int(gp.pose_ids[17]), int(gp.lm_ids[2])
    z = perturbed(relative_pose(gp.est[p0], gp.est[p1]))
    W = OMEGA6.reshape(-1)
    good = [1, 0, p0, p1]

    def fresh():
        return [np.full(2, -7.0), np.full(12, -7.0), np.full(72, -7.0)]

    def untouched(outs):
        return all(np.all(o == -7.0) for o in outs)

    outs = fresh()
    assert _raw(gpu_lib, B._h, "sslam_batch_gate", [], None, None, 0, outs) == 0 and untouched(outs)          # n == 0
    assert _raw(gpu_lib, B._h, "sslam_batch_gate", good, z, W, 1, outs) == 0
    assert outs[0][0] > 0 and outs[0][1] == -7.0 and np.all(outs[1][:6] != -7.0) and np.all(outs[1][6:] == -7.0) and np.all(outs[2][36:] == -7.0)
    d2 = outs[0][0]
    assert _raw(gpu_lib, B._h, "sslam_batch_gate", good, z, W, 1, [outs[0], None, None]) == 0 and outs[0][0] == d2   # e_out, cov_out NULL
    nan, zq = z.copy(), z.copy()
    nan[1] = np.nan
    zq[3:] = 0
    Wn = W.copy()
    Wn[7] = np.inf
    bad = [([2, 0, p0, p1], z, W), ([-1, 0, p0, p1], z, W),                    # graph index out of range
           ([1, 2, p0, p1], z, W), ([1, -1, p0, p1], z, W),                    # kind out of range
           ([1, 0, gp.nv, p1], z, W), ([1, 0, p0, -1], z, W),                  # vertex id out of range
           ([1, 0, p0, lm], z, W), ([1, 1, p0, p1], z, W), ([1, 1, lm, p0], z, W), ([1, 0, lm, p1], z, W),   # wrong vertex type for the kind
           ([1, 0, p0, p0], z, W),                                             # v_from == v_to
           (good, nan, W), (good, z, Wn), (good, zq, W)]                       # non-finite z, non-finite info, quaternion of zero norm
    for cand, zz, ww in bad:
        outs = fresh()
        # the bad candidate after a good one: nothing is written, the good one's outputs included
        assert _raw(gpu_lib, B._h, "sslam_batch_gate", good + cand, np.concatenate([z, zz]), np.concatenate([W, ww]), 2, outs) == -1, cand
        assert untouched(outs), cand
    outs = fresh()
    dp = C.POINTER(C.c_double)
    zp, cp = z.ctypes.data_as(dp), np.array(good, np.int32)
    ip = cp.ctypes.data_as(C.POINTER(C.c_int32))
    o = [a.ctypes.data_as(dp) for a in outs]
    assert gpu_lib.sslam_batch_gate(B._h, None, zp, None, 1, *o) == -1                    # NULL cand, z, d2_out with n > 0
    assert gpu_lib.sslam_batch_gate(B._h, ip, None, None, 1, *o) == -1
    assert gpu_lib.sslam_batch_gate(B._h, ip, zp, None, 1, None, o[1], o[2]) == -1
    assert gpu_lib.sslam_batch_gate(None, None, None, None, 0, None, None, None) == -1    # a NULL handle, before n == 0
    assert untouched(outs)
    # the single-graph entry: the same checks, cand = (kind, v_from, v_to)
    G = graphs[1]
    assert _raw(gpu_lib, G._h, "sslam_graph_gate", [], None, None, 0, outs) == 0 and untouched(outs)
    assert gpu_lib.sslam_graph_gate(None, None, None, None, 0, None, None, None) == -1
    for cand, zz, ww in bad[2:]:
        assert _raw(gpu_lib, G._h, "sslam_graph_gate", cand[1:], zz, ww, 1, outs) == -1 and untouched(outs), cand
    # the iterative solvers have no factor to walk; an edge shard holds a partial H
    pcg = [GraphSLAM.from_problem(gp) for gp in gps]
    for S in pcg:
        S.set_option("solver", 0)
    Bp = GraphBatch(pcg)
    Bp.upload()
    assert _raw(gpu_lib, Bp._h, "sslam_batch_gate", good, z, W, 1, outs) == -6 and untouched(outs)
    assert _raw(gpu_lib, pcg[1]._h, "sslam_graph_gate", good[1:], z, W, 1, outs) == -6 and untouched(outs)
    sch = [GraphSLAM.from_problem(gp) for gp in gps]
    for S in sch:
        S.set_option("solver", 2)
    Bs = GraphBatch(sch)
    Bs.upload()
    assert _raw(gpu_lib, Bs._h, "sslam_batch_gate", good, z, W, 1, outs) == -6 and untouched(outs)
    Be = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps])
    Be.upload()
    Be.set_edge_shard(0, 2)
    assert _raw(gpu_lib, Be._h, "sslam_batch_gate", good, z, W, 1, outs) == -6 and untouched(outs)
    # a structure change since creation
    graphs[0].add_point_xyz_node([0.0, 0.0, 0.0])
    assert _raw(gpu_lib, B._h, "sslam_batch_gate", good, z, W, 1, outs) == -1 and untouched(outs)


def _gate_chain():
    """the chain of tests/shim_gate_check.cpp through the Python mirror: keep the two in step"""
    from semantic_slam_amd import GraphSLAM
    G = GraphSLAM()
    W = np.diag([150.0] * 3 + [1e5] * 3)
    nodes = []
    for i in range(20):
        nodes.append(G.add_se3_node([0.55 * i, 0.02 * i, 0, 0, 0, 0, 1]))
        if i > 0:
            G.add_se3_edge(nodes[i - 1], nodes[i], [0.5, 0, 0, 0, 0, 0, 1], W)
    pts = []
    for l in range(4):
        pts.append(G.add_point_xyz_node([2.5 * l + 1.0, 1.5, 0.5]))
        for i in range(5 * l, 5 * l + 4):
            G.add_se3_point_xyz_edge(nodes[i], pts[l], [2.5 * l + 1.0 - 0.5 * i, 1.5, 0.5], np.eye(3) * 50.0)
    return G, nodes, pts, W


def test_cpp_shim_gate_end_to_end(gpu_lib, tmp_path):
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_gate")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_gate_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"shim gate ok: se3 (\S+) point (\S+) no-info (\S+)", out.stdout)
    assert m, out.stdout
    G, nodes, pts, W = _gate_chain()
    assert G.optimize()
    want = (G.gate_se3(nodes[2], nodes[18], [8.1, 0.1, 0, 0, 0, 0, 1], W), G.gate_point(nodes[17], pts[0], [-7.4, 1.4, 0.6], np.eye(3) * 50.0),
            G.gate_se3(nodes[2], nodes[18], [8.1, 0.1, 0, 0, 0, 0, 1], None))
    for got, ref in zip(m.groups(), want):
        print("shim", got, "mirror", ref)
        assert np.isfinite(ref) and ref > 0
        assert abs(float(got) - ref) <= 1e-9 * ref
