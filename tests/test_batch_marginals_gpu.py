"""sslam_batch_marginals on the GPU: blocks of H^-1 for (graph, row vertex, column vertex) requests of a batch -- diagonal and
off-diagonal, one wave per request along the elimination-tree paths (k_chol_marginal_pairs), Y in LDS or in a device scratch buffer.
References: the dense inverse of the oracle's H at the downloaded estimates, and sslam_graph_marginals of the downloaded host graphs (the
same kernel from a batch of one: a check of the plumbing, not an independent reference).
Tolerance, everywhere a tolerance is used: the project's own for marginals, |a - ref|.max() <= 1e-6 |ref|.max() per block."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from semantic_slam_amd.synth import make_graph
from oracle.oracle import GraphProblem

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _close(a, ref, what=""):
    err, scale = np.abs(a - ref).max(), np.abs(ref).max()
    print(f"{what} shape {a.shape} max error {err:.3e} reference scale {scale:.3e} ratio {err / scale:.3e}")
    assert a.shape == ref.shape
    assert err <= TOL * scale, what


def _dense_inverse(gp):
    U, _ = gp.linearize()
    return np.linalg.inv((U + sp.triu(U, 1).T).toarray())


def _ref_block(gp, Hinv, vr, vc):
    h, _ = gp.hessian_index()
    dr = 6 if gp.vtype[vr] == 0 else 3
    dc = 6 if gp.vtype[vc] == 0 else 3
    if h[vr] < 0 or h[vc] < 0:
        return np.zeros((dr, dc))
    return Hinv[h[vr]:h[vr] + dr, h[vc]:h[vc] + dc]


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


@pytest.fixture(scope="module")
def three(gpu_lib):
    """three distinct graphs, two LM iterations in one batch, the estimates downloaded; every landmark diagonal, two pose diagonals, one
    pose-pose, one pose-landmark (both ways round) and one landmark-landmark pair per graph"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=s), interleave=True) for s in (4, 5, 6)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    B.upload()
    B.optimize(2)
    B.download()
    req = []
    for g, gp in enumerate(gps):
        gp.est[:] = graphs[g].estimates()
        lm, po = [int(v) for v in gp.lm_ids], [int(v) for v in gp.pose_ids]
        req += [(g, v, v) for v in lm]
        req += [(g, po[7], po[7]), (g, po[39], po[39])]
        req += [(g, po[10], po[30]), (g, po[12], lm[3]), (g, lm[3], po[12]), (g, lm[0], lm[5])]
    blocks = B.marginals(req)
    return gps, graphs, B, req, blocks


def test_three_distinct_graphs_match_the_dense_inverse(three):
    gps, graphs, B, req, blocks = three
    Hinv = [_dense_inverse(gp) for gp in gps]
    assert len(blocks) == len(req)
    shapes = set()
    for (g, vr, vc), a in zip(req, blocks):
        _close(a, _ref_block(gps[g], Hinv[g], vr, vc), f"graph {g} block ({vr}, {vc})")
        shapes.add(a.shape)
    assert shapes == {(3, 3), (6, 6), (6, 3), (3, 6)}
    # the pose-landmark pair both ways round: transposes of each other
    for k, (g, vr, vc) in enumerate(req):
        if gps[g].vtype[vr] == 0 and gps[g].vtype[vc] != 0:
            assert req[k + 1] == (g, vc, vr)
            _close(blocks[k + 1].T, blocks[k], f"graph {g} transpose of ({vc}, {vr})")


def test_scratch_placement_equals_lds_bitwise(three):
    """SSLAM_MARGINAL_LDS_BYTES = 1: no path fits, every request runs out of its slice of the device scratch buffer.  The kernel body and
    the order of its operations are those of the LDS form, so the blocks are equal exactly, not within a tolerance."""
    gps, graphs, B, req, blocks = three
    again = B.marginals(req)                       # the call repeats itself (same placement) ...
    scratch = _with_lds_budget(1, lambda: B.marginals(req))
    for a, b, c in zip(blocks, again, scratch):
        assert np.array_equal(a, b)
        assert np.array_equal(a, c)                # ... and the other placement gives the same bits
    # a budget that holds the single paths of the diagonal requests but not the two paths of a pair: both placements in one call
    for entries in (8, 16, 24, 32):                # (288 + 16 bytes, and 308 per path entry: its Y block, its record, its y offset)
        mixed = _with_lds_budget(36 * 8 + 16 + 308 * entries, lambda: B.marginals(req))
        for a, c in zip(blocks, mixed):
            assert np.array_equal(a, c)


def test_rounds_agree_bitwise(three):
    """SSLAM_PATH_ROUND_INTS cuts a call into rounds of requests (each its own upload, launches, download and scatter): at 1 every request
    is a round, at 64 a round takes a few; the blocks are those of the one-round call.  With the default budget (every path in LDS), and
    with a budget of 16 path entries that puts both placements into one round."""
    gps, graphs, B, req, blocks = three
    for budget in (None, 288 + 16 + 308 * 16):
        for ints in (1, 64):
            got = _with_env("SSLAM_PATH_ROUND_INTS", ints, lambda: _with_lds_budget(budget, lambda: B.marginals(req)))
            assert len(got) == len(blocks)
            for a, c in zip(blocks, got):
                assert np.array_equal(a, c), (budget, ints)


def test_front_kernel_family(gpu_lib):
    """The flat factor the marginals read is written by the front kernels (k_front_pieces / k_front_tail) in the throughput regime:
    chol_throughput_regime is B >= 32 or (B >= 2 and >= 8000 block rows), and front tables are its default (chol_symbolic: front = thr).
    32 graphs of 40 poses and 8 landmarks are the smallest batch of small graphs that gets there (31 would take the record kernels);
    info("factor_front") says which family the plan runs."""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=700 + k), interleave=bool(k & 1)) for k in range(32)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    assert B.info("factor_front") == 1
    B.upload()
    B.optimize(2)
    B.download()
    sample = (0, 15, 31)
    ids = {g: [int(v) for v in gps[g].lm_ids] + [int(gps[g].pose_ids[k]) for k in (3, 39)] for g in sample}
    got = B.landmark_marginals([ids.get(g, []) for g in range(32)])
    assert [len(x) for x in got] == [len(ids.get(g, [])) for g in range(32)]
    for g in sample:
        gps[g].est[:] = graphs[g].estimates()
        Hinv = _dense_inverse(gps[g])
        ref = graphs[g].computeLandmarkMarginals(ids[g])   # the same pair kernel on the record kernels' factor: not independent, hence Hinv
        for v, a, r in zip(ids[g], got[g], ref):
            _close(a, r, f"graph {g} vertex {v}")
            _close(a, _ref_block(gps[g], Hinv, v, v), f"graph {g} vertex {v} against the dense inverse")
    small = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps[:4]])
    assert small.info("factor_front") == 0


def test_batch_of_one_against_the_single_graph_handle(gpu_lib):
    """A handle owns a batch of one: sslam_graph_marginals and sslam_batch_marginals of a batch of one factor and walk identically, the
    blocks are equal bit for bit.  The dense inverse of the oracle's H is the independent reference."""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gp = GraphProblem.from_synth(make_graph(40, 8, seed=6), interleave=True)
    G = GraphSLAM.from_problem(gp)
    G.optimize(4)
    gp.est[:] = G.estimates()
    Hinv = _dense_inverse(gp)
    ids = [int(v) for v in gp.lm_ids] + [int(gp.pose_ids[k]) for k in (1, 20, 39)]
    ref = G.computeLandmarkMarginals(ids)
    M = GraphSLAM.from_problem(gp)
    for v in range(gp.nv):
        M.set_estimate(v, G.estimate(v))
    B = GraphBatch([M])
    B.upload()
    got = B.marginals([(0, v, v) for v in ids])
    for v, a, r in zip(ids, got, ref):
        _close(a, _ref_block(gp, Hinv, v, v), f"vertex {v} against the dense inverse")
        _close(r, _ref_block(gp, Hinv, v, v), f"vertex {v} of the handle against the dense inverse")
        assert np.array_equal(a, r), f"vertex {v}: max difference {np.abs(a - r).max():.3e}"


def test_edge_data_travels(gpu_lib):
    """a position prior (EdgeSE3PriorXYZ) and a Huber kernel on a landmark edge whose measurement is off by two metres (rho1 < 1): the
    batch's linearisation carries both, as sslam_graph_marginals' does on the downloaded graphs"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    graphs, gps = [], []
    for s in (21, 22):
        g = make_graph(40, 8, seed=s)
        gp = GraphProblem.from_synth(g, interleave=True)
        k = len(g.odom_ij) + 5                       # a landmark edge
        if s == 21:
            gp.meas[k, :3] += [2.0, -1.5, 1.0]
        G = GraphSLAM.from_problem(gp)
        if s == 21:
            G.add_se3_prior_xyz_edge(int(gp.pose_ids[25]), g.poses_init[25][:3] + 0.05, np.diag([40.0, 40.0, 10.0]))
            G.add_robust_kernel(k, "Huber", 1.0)
            G.corrupted_edge = k
        graphs.append(G); gps.append(gp)
    B = GraphBatch(graphs)
    B.upload()
    B.optimize(2)
    B.download()
    w = graphs[0].edge_chi2([graphs[0].corrupted_edge])[2][0]
    print("Huber weight of the corrupted edge", w)
    assert 0 < w < 1
    for g, (G, gp) in enumerate(zip(graphs, gps)):
        ids = [int(v) for v in gp.lm_ids] + [int(gp.pose_ids[25]), int(gp.pose_ids[39])]
        got = B.marginals([(g, v, v) for v in ids])
        ref = G.computeLandmarkMarginals(ids)
        for v, a, r in zip(ids, got, ref):
            _close(a, r, f"graph {g} vertex {v}")
    # the kernel matters: without it the corrupted edge pulls with its full weight and the landmark's covariance is another one
    lm = int(gps[0].evj[graphs[0].corrupted_edge])
    with_k = B.marginals([(0, lm, lm)])[0]
    graphs[0].add_robust_kernel(graphs[0].corrupted_edge, "NONE", 0.0)
    B.upload()
    without_k = B.marginals([(0, lm, lm)])[0]
    assert np.abs(with_k - without_k).max() > 1e-3 * np.abs(with_k).max()


def test_no_side_effects(gpu_lib):
    """optimize(2), marginals, optimize(2), download against the same without the marginals call: statistics and estimates bitwise"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    runs = []
    for with_marginals in (True, False):
        gps = [GraphProblem.from_synth(make_graph(40 + 6 * k, 8 + k, seed=50 + k), interleave=bool(k & 1)) for k in range(3)]
        graphs = [GraphSLAM.from_problem(gp) for gp in gps]
        B = GraphBatch(graphs)
        B.upload()
        s1 = B.optimize(2)
        if with_marginals:
            req = [(g, int(v), int(v)) for g, gp in enumerate(gps) for v in gp.lm_ids] + [(1, int(gps[1].pose_ids[3]), int(gps[1].lm_ids[2]))]
            assert len(B.marginals(req)) == len(req)
            _with_lds_budget(1, lambda: B.marginals(req))
        s2 = B.optimize(2)
        B.download()
        stats = [(s.iterations, s.trials, s.status, s.host_plan_us, s.chi2_before, s.chi2_after, s.lambda_, s.solver_iterations) for s in s1 + s2]
        runs.append((stats, [G.estimates() for G in graphs]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)


def _raw(lib, B, req, out):
    req = np.ascontiguousarray(req, np.int32).reshape(-1)
    return lib.sslam_batch_marginals(B._h, req.ctypes.data_as(C.POINTER(C.c_int32)), len(req) // 3, out.ctypes.data_as(C.POINTER(C.c_double)))


def test_contract_edges(gpu_lib):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    from semantic_slam_amd.graph_slam import SslamError
    gps = [GraphProblem.from_synth(make_graph(40, 8, seed=s), interleave=True) for s in (4, 5, 6, 7)]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    B.upload()
    fixed, lm, po = int(gps[1].pose_ids[0]), int(gps[1].lm_ids[2]), int(gps[1].pose_ids[9])
    z = B.marginals([(1, fixed, fixed), (1, fixed, lm), (1, lm, fixed), (1, lm, lm)])
    assert [b.shape for b in z] == [(6, 6), (6, 3), (3, 6), (3, 3)]
    assert all(np.all(b == 0) for b in z[:3]) and np.all(np.diag(z[3]) > 0)      # a fixed vertex on either side: zeros
    assert B.marginals([]) == []
    out = np.full(80, -7.0)
    assert _raw(gpu_lib, B, [], out) == 0 and _raw(gpu_lib, B, [0, lm, lm], out) == 0
    assert np.all(out[:9] != -7.0) and np.all(out[9:] == -7.0)
    for bad in ([(0, lm, lm), (4, 0, 0)], [(0, lm, lm), (-1, 0, 0)], [(0, lm, lm), (2, gps[2].nv, 0)], [(0, lm, lm), (2, 0, -1)]):
        out = np.full(80, -7.0)
        assert _raw(gpu_lib, B, bad, out) == -1                                      # SSLAM_ERR_INVALID ...
        assert np.all(out == -7.0)                                                   # ... and nothing written, the good request included
    assert gpu_lib.sslam_batch_marginals(B._h, None, 1, out.ctypes.data_as(C.POINTER(C.c_double))) == -1
    with pytest.raises(IndexError):
        B.marginals([(2, gps[2].nv, 0)])
    # a stream group of two parts over the four graphs: every request goes to its part.  The parts are batches of two graphs, the single
    # stream a batch of four: the same plan regime, and every graph of a batch is ordered, cut into pieces and factored on its own -- its
    # plan does not depend on its neighbours, so the blocks are those of the single-stream batch bitwise.
    req = []
    for g in (3, 0, 2, 1, 3):
        req += [(g, int(v), int(v)) for v in gps[g].lm_ids[:4]] + [(g, int(gps[g].pose_ids[5]), int(gps[g].lm_ids[1])), (g, int(gps[g].pose_ids[11]), int(gps[g].pose_ids[33]))]
    one = B.marginals(req)
    grp = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps], streams=2)
    assert grp.info("streams") == 2
    grp.upload()
    two = grp.marginals(req)
    for k, (a, b) in enumerate(zip(one, two)):
        assert np.array_equal(a, b), f"request {k} {req[k]}: max difference {np.abs(a - b).max():.3e}"
    # the iterative solvers have no factor to walk
    pcg = [GraphSLAM.from_problem(gp) for gp in gps[:2]]
    for G in pcg:
        G.set_option("solver", 0)
    Bp = GraphBatch(pcg)
    Bp.upload()
    with pytest.raises(SslamError) as ei:
        Bp.marginals([(0, lm, lm)])
    assert ei.value.code == -6
