"""The LDS budget of the front kernels (CholOpts::lds_budget) on the GPU: a batch of 34 graphs -- the throughput regime, k_front_pieces on
128 threads -- solved and optimised with no budget, with 20480 B and with 12288 B.  The budget only decides which components share a
workgroup, so the three plans give the same bits; each is held to the oracle's Cholesky solve and LM bookkeeping.

Damping of the solves: the cycle below, every value > 0.  The bar of 1e-9 compares two double-precision factorisations with different
elimination orders, whose difference grows with the condition number of H + lambda I; LM never solves the undamped system, and the
smallest lambda here (1e-3) is below what the optimiser reaches on these graphs."""
import numpy as np
import pytest

from semantic_slam_amd.synth import make_graph
from oracle.oracle import GraphProblem

pytestmark = pytest.mark.gpu

BUDGETS = (0, 20480, 12288)
LAMBDAS = (1e-3, 0.05, 0.7, 5.0)
N = 34


def _problems():
    return [GraphProblem.from_synth(make_graph(150 + 4 * k, 30, seed=200 + k), interleave=bool(k & 1)) for k in range(N)]


def _batch(gps):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    B = GraphBatch([GraphSLAM.from_problem(gp) for gp in gps])
    B.upload()
    return B


@pytest.fixture(scope="module")
def oracle_runs():
    """the oracle's solve of every graph at its lambda, then its five LM iterations: computed once, read by the tests"""
    gps = _problems()
    lam = [LAMBDAS[g % len(LAMBDAS)] for g in range(N)]
    xs = [gp.solve(lam[g]) for g, gp in enumerate(gps)]
    st = [gp.optimize(5) for gp in gps]
    return lam, xs, [(s.iterations, s.trials) for s in st]


@pytest.fixture(scope="module")
def gpu_runs(gpu_lib, oracle_runs):
    import os
    lam = oracle_runs[0]
    runs = {}
    old = os.environ.get("SSLAM_CHOL_OPTS")
    try:
        for budget in BUDGETS:
            os.environ["SSLAM_CHOL_OPTS"] = f"lds_budget={budget}"     # read when the plan is built
            B = _batch(_problems())
            assert B.info("factor_front") == 1
            per_cu = (B.info("front_groups_per_cu_leaf"), B.info("front_groups_per_cu_mid"))
            xs = B.solve(lam)
            st = B.optimize(5)
            runs[budget] = (xs, [(s.iterations, s.trials) for s in st], per_cu)
    finally:
        if old is None: os.environ.pop("SSLAM_CHOL_OPTS")
        else: os.environ["SSLAM_CHOL_OPTS"] = old
    return runs


def test_solutions_are_bitwise_equal_and_match_the_oracle(gpu_runs, oracle_runs):
    lam, x_or, _ = oracle_runs
    x0 = gpu_runs[0][0]
    for g in range(N):
        err = float(np.abs(x0[g] - x_or[g]).max() / np.abs(x_or[g]).max())
        print(f"graph {g}: dim {len(x_or[g])} lambda {lam[g]:g} error against the oracle {err:.3e} (bar 1e-9)")
        assert err <= 1e-9, g
        for budget in BUDGETS[1:]:
            assert np.array_equal(gpu_runs[budget][0][g], x0[g]), (budget, g)


def test_lm_bookkeeping_matches_the_oracle(gpu_runs, oracle_runs):
    for budget in BUDGETS:
        assert gpu_runs[budget][1] == oracle_runs[2], budget


def test_groups_per_cu_do_not_fall_with_the_budget(gpu_runs):
    per = [gpu_runs[b][2] for b in BUDGETS]       # no budget, 20480 B, 12288 B
    print("front workgroups per CU (leaf, mid):", dict(zip(BUDGETS, per)))
    for leaf, mid in per:
        assert leaf >= 1 and mid >= 1
    for k in (0, 1):
        assert per[0][k] <= per[1][k] <= per[2][k]


def test_failed_pivot_is_reported_with_the_budget_on(gpu_lib, monkeypatch):
    """one graph of the batch has a landmark whose edges carry a negative definite information matrix: its diagonal block of H + lambda I is
    negative at lambda = 0.05, the 3 x 3 factor of front_piece meets a pivot <= 0 and the solve reports the breakdown; the same batch
    without that graph taking part solves"""
    from semantic_slam_amd import SslamError
    monkeypatch.setenv("SSLAM_CHOL_OPTS", "lds_budget=12288")
    gs = [make_graph(150 + 4 * k, 30, seed=200 + k) for k in range(N)]
    bad = 7
    lm = int(gs[bad].lm_ij[0][1])
    gs[bad].lm_info[np.asarray(gs[bad].lm_ij)[:, 1] == lm] = -4.0 * np.eye(3) * abs(gs[bad].lm_info[0]).max()
    gps = [GraphProblem.from_synth(g, interleave=bool(k & 1)) for k, g in enumerate(gs)]
    B = _batch(gps)
    assert B.info("factor_front") == 1
    lam = [0.05] * N
    with pytest.raises(SslamError) as e:
        B.solve(lam)
    assert e.value.code == -4      # SSLAM_ERR_NUMERIC
    lam[bad] = -1.0                # the graph sits out: the others solve
    xs = B.solve(lam)
    assert xs[bad] is None and all(x is not None and np.isfinite(x).all() for g, x in enumerate(xs) if g != bad)
