"""sslam_batch_solve on the GPU: one linear solve (H_g + lambda_g I) x_g = b_g of every graph of a batch, through the launches the LM loop
takes -- the single launch of small batches, the per-depth record and front kernels, their compacted (index-list) forms of the LM endgame,
the stream group and the iterative solvers -- against an extended-precision reference (tests/solve_ref.py).

Reference system: the GPU's own normal equations of the graph, from a fresh single handle (test_linearize_matches_oracle pins them), so
that an error of the linearisation does not leak into the solve bar.
Forward bar:  max|x - x_ref| <= bound * max|x_ref|, bound = min(1e-9, max(1e-13, 10 * double_error)).
Backward bar: longdouble max|(H + lambda I) x - b| <= min(1e-9, 10 * that of the oracle's own solve / max|b|) * max|b|.
double_error is what an honest double factorisation does on the very system (solve_ref.double_error), 1e-9 the project's existing bar
as a ceiling, and the factor 10 covers another elimination and summation order.  Iterative solvers: 1e-6 with pcg_tol 1e-10, forward only."""
import ctypes as C

import numpy as np
import pytest

import solve_ref as R
from semantic_slam_amd.synth import make_graph
from oracle.oracle import GraphProblem

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 1e-3, 0.05, 0.7, 5.0)


def _lams(n, only=None):
    """lambda of graph g: the cycle above, so that no two neighbours share one; -1 (sits out) for the graphs not in `only`"""
    return [LAMBDAS[g % len(LAMBDAS)] if only is None or g in only else -1.0 for g in range(n)]


def _check(gp, x, lam, what, iterative=False):
    """one graph's solution against the refined reference of the GPU's own system"""
    from semantic_slam_amd import GraphSLAM
    U, b = GraphSLAM.from_problem(gp).linearize()
    assert x is not None and x.shape == b.shape, what
    x_ref, _ = R.refined_solve(U, b, lam)
    err = R.rel_error(x, x_ref)
    if iterative:
        print(f"{what}: dim {len(b)} lambda {lam:g} error {err:.3e} bound 1e-06 (iterative)")
        assert err <= 1e-6, what
        return
    x_or = gp.solve(lam)
    de = R.double_error(gp, U, b, lam, x_ref, x_oracle=x_or)
    bound = min(1e-9, max(1e-13, 10 * de))
    bmax = float(np.abs(b).max())
    res = float(np.abs(R.residual(U, b, lam, x)).max()) / bmax
    res_o = float(np.abs(R.residual(U, b, lam, x_or)).max()) / bmax
    rbound = min(1e-9, 10 * res_o)
    print(f"{what}: dim {len(b)} lambda {lam:g} | forward: double {de:.3e} achieved {err:.3e} bound {bound:.3e} | "
          f"backward: oracle {res_o:.3e} achieved {res:.3e} bound {rbound:.3e}")
    assert err <= bound, what
    assert res <= rbound, what


def _batch(gps, streams=0, solver=None):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    if solver is not None:
        for G in graphs:
            G.set_option("solver", solver)
            G.set_option("pcg_tol", 1e-10)
    B = GraphBatch(graphs, streams=streams)
    B.upload()
    return graphs, B


def _same(a, b):
    return a is not None and b is not None and np.array_equal(a, b)


# ---- 1. small batch: the single launch ---------------------------------------------------------------------------------------------
def test_small_batch_single_launch(gpu_lib):
    """B = 3 < 8: k_chol_flow, every graph with its own lambda"""
    sizes = [(60, 12), (45, 9), (80, 15)]
    gps = [GraphProblem.from_synth(make_graph(a, b, seed=10 + i), interleave=bool(i & 1)) for i, (a, b) in enumerate(sizes)]
    _, B = _batch(gps)
    assert B.info("factor_front") == 0
    lam = _lams(3)
    xs = B.solve(lam)
    assert B.last_solver_iterations == [0, 0, 0]
    for g, gp in enumerate(gps):
        _check(gp, xs[g], lam[g], f"small batch graph {g}")
    # a graph sitting out of a small batch: no compaction below 8 graphs, the others' bits do not move
    xm = B.solve([lam[0], -1.0, lam[2]])
    assert xm[1] is None and _same(xm[0], xs[0]) and _same(xm[2], xs[2])
    assert B.info("compact_rounds") == 0


# ---- 2. / 3. per-depth plans and their compacted forms -----------------------------------------------------------------------------
def _ten():
    return [GraphProblem.from_synth(make_graph(40 + 5 * i, 8 + i, seed=900 + i, landmark_kind="plane" if i & 1 else "point"), interleave=bool(i & 2))
            for i in range(10)]


def _masked_rounds(B, gps, full, lam, sample):
    n = len(gps)
    few = {1, 4, 6, 9}
    c0 = B.info("compact_rounds")
    xb = B.solve(_lams(n, few))                          # (b) 4 of 10: compacted
    assert B.info("compact_rounds") == c0 + 1
    for g in range(n):
        if g in few:
            assert _same(xb[g], full[g]), f"graph {g}: compacted launch differs from the full one"
        else:
            assert xb[g] is None
    rest = set(range(n)) - few
    xc = B.solve(_lams(n, rest))                         # (c) 6 of 10: more than half, full ranges
    assert B.info("compact_rounds") == c0 + 1
    for g in range(n):
        assert (_same(xc[g], full[g]) if g in rest else xc[g] is None), g
    xd = B.solve(lam)                                    # (d) the compaction does not outlive its call
    assert B.info("compact_rounds") == c0 + 1
    for g in range(n):
        assert _same(xd[g], full[g]), g
    for g in sample:
        _check(gps[g], xb[g] if g in few else xc[g], lam[g], f"graph {g} (masked call)")


def test_record_plan_with_compaction(gpu_lib):
    """B = 10: a launch per depth with the record kernels (k_chol_pieces, k_chol_tail, k_chol_back_*); with 4 of 10 graphs taking part the
    launches run off index lists, as in the LM endgame"""
    gps = _ten()
    _, B = _batch(gps)
    assert B.info("factor_front") == 0
    lam = _lams(10)
    full = B.solve(lam)                                  # (a)
    assert B.info("compact_rounds") == 0
    for g, gp in enumerate(gps):
        _check(gp, full[g], lam[g], f"record plan graph {g}")
    _masked_rounds(B, gps, full, lam, sample=())


@pytest.mark.parametrize("env,front", [
    ({"cap_leaf": "400", "cap_tail": "700", "tail_width": "2", "min_chunk": "1", "pcap_leaf": "16", "nt_leaf": "256"}, 0),   # a multi-piece tail, split lists
    ({"cap_leaf": "400", "group_cap": "1500", "nt_leaf": "512", "ustage": "0"}, 0),                                        # groups
    ({"flow": "0", "cap_leaf": "400", "tail_width": "2", "mid_width": "12", "cap_mid": "1200"}, 0),                        # the mid class
    ({"front": "1", "flow": "0", "cap_leaf": "300", "group_cap": "1200", "nt_leaf": "128", "tail_width": "0", "mid_width": "8", "cap_mid": "1500"}, 1),   # front tables, groups, no tail
])
def test_forced_plan_shapes_under_compaction(gpu_lib, monkeypatch, env, front):
    """the plan shapes of test_cholesky_pieces_of_every_shape on the batch of ten: the index-list form of the leaf, mid, group, tail and
    backward kernels of both families under the bar"""
    monkeypatch.setenv("SSLAM_CHOL_OPTS", ",".join(f"{k}={v}" for k, v in env.items()))   # read when the plan is built
    gps = _ten()
    _, B = _batch(gps)
    assert B.info("factor_front") == front
    lam = _lams(10)
    full = B.solve(lam)
    for g in (0, 5, 7):
        _check(gps[g], full[g], lam[g], f"forced shape graph {g}")
    _masked_rounds(B, gps, full, lam, sample=(4, 6, 9))


# ---- 4. throughput regime by batch size --------------------------------------------------------------------------------------------
def test_throughput_regime_by_batch_size(gpu_lib):
    """32 graphs of ~600 poses: groups of leaf pieces, mid pieces and a tail per graph through the front kernels; then 4 of 32 off index lists"""
    gps = [GraphProblem.from_synth(make_graph(600 + 7 * k, 120 + k, seed=500 + k, landmark_kind="plane" if k & 1 else "point"), interleave=bool(k & 1))
           for k in range(32)]
    _, B = _batch(gps)
    assert B.info("factor_front") == 1
    lam = _lams(32)
    full = B.solve(lam)
    for g in (0, 13, 31):
        _check(gps[g], full[g], lam[g], f"throughput batch graph {g}")
    few = {0, 5, 13, 31}
    c0 = B.info("compact_rounds")
    xm = B.solve(_lams(32, few))
    assert B.info("compact_rounds") == c0 + 1
    for g in range(32):
        assert (_same(xm[g], full[g]) if g in few else xm[g] is None), g


# ---- 5. throughput regime by rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,seeds,front", [
    (((3400, 700), (3450, 710)), (7, 8), 1),      # 8260 block rows: the throughput plan on the front kernels
    (((3400, 700), (3450, 710)), (40, 41), 0),    # the same regime, but front_build refuses these trees (a level wider than a workgroup's teams): its record kernels
    (((3200, 650), (3200, 650)), (40, 41), 0),    # 7700 block rows: the small-batch plan, one launch
])
def test_regime_switch_by_block_rows(gpu_lib, sizes, seeds, front):
    """chol_throughput_regime's rows clause, B >= 2 and >= 8000 block rows, on both sides of the line.  Above it the plan is cut for
    throughput (groups on 128 threads, mid class) and runs the front kernels where the front tables can be built; for most pairs of
    graphs of this size they cannot (chol_symbolic: a level of a piece with more columns than 2 * nt / 8), the library says so on stderr
    and the same cut runs on the record kernels: both families are held to the bars here."""
    interleave = seeds == (7, 8)
    gps = [GraphProblem.from_synth(make_graph(a, b, seed=s), interleave=interleave or bool(i & 1)) for i, ((a, b), s) in enumerate(zip(sizes, seeds))]
    _, B = _batch(gps)
    rows = sum(a + b for a, b in sizes)
    assert B.info("factor_front") == front
    lam = _lams(2)
    xs = B.solve(lam)
    for g, gp in enumerate(gps):
        _check(gp, xs[g], lam[g], f"{rows} block rows, front {front}, graph {g}")


# ---- 6. stream group ---------------------------------------------------------------------------------------------------------------
def test_stream_group_solve_equals_the_single_stream_batch(gpu_lib):
    gps = []
    for i in range(70):
        g = make_graph(40 + 2 * i, 8 + (i % 5), seed=300 + i, noise_scale=0.0 if i == 11 else 1.0)
        gps.append(GraphProblem.from_synth(g, interleave=bool(i & 1)))
    _, B1 = _batch(gps)
    _, B2 = _batch(gps, streams=2)
    assert B2.info("streams") == 2
    lam = _lams(70)
    x1, x2 = B1.solve(lam), B2.solve(lam)
    for g in range(70):
        assert _same(x1[g], x2[g]), g
    for g in (3, 34, 69):                                # both parts, and the graph at their seam
        _check(gps[g], x2[g], lam[g], f"stream group graph {g}")
    # graphs sitting out in both parts: 8 of the first 35 and 9 of the last 35 take part -> every part compacts
    only = set(range(0, 70, 4)) - {0}
    m1, m2 = B1.solve(_lams(70, only)), B2.solve(_lams(70, only))
    assert B1.info("compact_rounds") == 1 and B2.info("compact_rounds") == 2   # summed over the parts
    for g in range(70):
        if g in only:
            assert _same(m1[g], x1[g]) and _same(m2[g], x1[g]), g
        else:
            assert m1[g] is None and m2[g] is None


# ---- 7. iterative solvers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [0, 2])
def test_iterative_solvers(gpu_lib, solver):
    sizes = [(60, 12), (45, 9), (80, 15)]
    gps = [GraphProblem.from_synth(make_graph(a, b, seed=20 + i), interleave=bool(i & 1)) for i, (a, b) in enumerate(sizes)]
    _, B = _batch(gps, solver=solver)
    lam = [1e-3, 0.7, 5.0]
    xs = B.solve(lam)
    for g, gp in enumerate(gps):
        assert B.last_solver_iterations[g] > 0
        _check(gp, xs[g], lam[g], f"solver {solver} graph {g}", iterative=True)
    xm = B.solve([-1.0, 0.7, -1.0])
    assert xm[0] is None and xm[2] is None and B.last_solver_iterations[0] == 0
    _check(gps[1], xm[1], 0.7, f"solver {solver} graph 1 alone", iterative=True)


# ---- 8. nothing is left behind -----------------------------------------------------------------------------------------------------
def test_solve_leaves_the_batch_as_it_found_it(gpu_lib):
    def fresh():
        return _batch(_ten())

    def stats(st):
        return [(s.status, s.iterations, s.trials, s.chi2_before, s.chi2_after, s.lambda_) for s in st]
    req = [(g, 3, 3) for g in range(10)] + [(g, 2, 7) for g in range(10)]
    g0, B0 = fresh()
    marg0 = B0.marginals(req)
    st0 = B0.optimize(6); B0.download()
    g1, B1 = fresh()
    B1.solve(_lams(10))
    B1.solve(_lams(10, {1, 4, 6, 9}))
    marg1 = B1.marginals(req)
    st1 = B1.optimize(6); B1.download()
    for a, b in zip(marg0, marg1):
        assert np.array_equal(a, b)
    assert stats(st0) == stats(st1)
    for a, b in zip(g0, g1):
        assert np.array_equal(a.estimates(), b.estimates())
    # and between two optimize calls: the LM states it borrows go back
    g2, B2 = fresh()
    B2.optimize(3)
    B2.solve(_lams(10, {0, 2}))
    st2 = B2.optimize(3); B2.download()
    g3, B3 = fresh()
    B3.optimize(3)
    st3 = B3.optimize(3); B3.download()
    assert stats(st2) == stats(st3)
    for a, b in zip(g2, g3):
        assert np.array_equal(a.estimates(), b.estimates())


# ---- 9. contract -------------------------------------------------------------------------------------------------------------------
def test_contract(gpu_lib):
    from semantic_slam_amd.graph_slam import SslamError, _dptr
    lib = gpu_lib
    gps = _ten()
    graphs, B = _batch(gps)
    dims = [GraphProblem.hessian_index(gp)[1] for gp in gps]
    n = int(lib.sslam_batch_solve(B._h, None, None, 0, None))      # x == NULL reports the size
    assert n == sum(dims)
    lam = np.array(_lams(10))
    x = np.full(n, 7.0)
    assert lib.sslam_batch_solve(B._h, _dptr(lam), _dptr(x), n - 1, None) == -1   # SSLAM_ERR_INVALID: too small a capacity
    assert np.all(x == 7.0)
    assert lib.sslam_batch_solve(B._h, None, _dptr(x), n, None) == -1
    bad = lam.copy(); bad[3] = np.nan
    assert lib.sslam_batch_solve(B._h, _dptr(bad), _dptr(x), n, None) == -1
    assert np.all(x == 7.0)
    # all lambdas negative: zeros, nothing launched, no error
    c0 = B.info("compact_rounds")
    none = np.full(10, -1.0)
    it = (C.c_int64 * 10)(*([5] * 10))
    assert lib.sslam_batch_solve(B._h, _dptr(none), _dptr(x), n, it) == n
    assert np.all(x == 0.0) and list(it) == [0] * 10
    assert B.solve(none) == [None] * 10 and B.info("compact_rounds") == c0
    # the layout: graph after graph, each in its own hessian-index order; zeros for a graph that sat out
    one = np.full(10, -1.0); one[4] = 0.7
    assert lib.sslam_batch_solve(B._h, _dptr(one), _dptr(x), n, None) == n
    o = sum(dims[:4])
    assert np.all(x[:o] == 0.0) and np.all(x[o + dims[4]:] == 0.0)
    _check(gps[4], x[o:o + dims[4]].copy(), 0.7, "graph 4 alone, C layout")
    # an edge-sharded batch refuses
    B.set_edge_shard(0, 2)
    with pytest.raises(SslamError) as e:
        B.solve(lam)
    assert e.value.code == -6                                      # SSLAM_ERR_UNSUPPORTED
    B.set_edge_shard(0, 1)
    # a graph that gained an edge after sslam_batch_create
    G = graphs[2]
    G.add_se3_edge(int(gps[2].pose_ids[0]), int(gps[2].pose_ids[1]), [1, 0, 0, 0, 0, 0, 1], np.eye(6))
    with pytest.raises(SslamError) as e:
        B.solve(lam)
    assert e.value.code == -1
    assert lib.sslam_batch_solve(B._h, None, None, 0, None) == -1
