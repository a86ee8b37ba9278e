"""The LDS budget of the front kernels (CholOpts::lds_budget, chol_plan.hpp) on the CPU: the plan is exported through the C-ABI and walked by
the numpy executor of tests/chol_plan_exec.py in the kernels' own order.  With a budget no group of a per-depth launch needs more LDS in
k_front_pieces than the budget says (a component above it alone stays a group of one), a launch reserves what its largest group needs, and
the factor is the one of the plan without a budget, bit for bit: grouping decides which components share a workgroup and where L lives,
never the order of a sum."""
import numpy as np
import pytest

from semantic_slam_amd.synth import make_graph
from chol_plan_exec import Plan
from test_chol_plan_cpu import _plan_and_system

# the batch regime forced onto one graph: the options of test_front_tables_are_a_fraction_of_the_record_tables
ENV = {"nt_leaf": 128, "group_cap": 2800, "cap_leaf": 700, "mid_width": 60, "tail_width": 6, "order_mul": 1.5, "order_add": 2, "ustage": 0, "flow": 0}
LAM = 1e-3
ARRAYS = ("col", "blk", "upd", "item", "mb", "ilv", "piece", "plv_ptr", "plv_pieces", "tail_ptr", "tail_pieces", "plv_lds_f", "plv_lds_b", "asrc", "usrc",
          "fwd", "uitem", "umb", "rcol", "rupd", "plv_nt", "plv_cls", "fblob", "fgrp", "plv_lds_ff")


def _front_lds(plan):
    """LDS doubles of k_front_pieces per piece: L, y, the blob and the derived tables (front_plan.hpp, FrontHost::lds)"""
    P, F = plan.piece, plan.fgrp
    return ((P["lsize"] + 1) & ~1) + ((P["ysize"] + 1) & ~1) + F["words"] // 2 + (F["dbytes"] + 7) // 8 + 2


def _components(plan, p):
    return int(plan.fblob[plan.fgrp[p]["blob"]] & 255)


def _solve(plan, H, b):
    """factor (the walk of the front kernels), forward and backward substitution; the dense factor and the solution in internal row order"""
    Lval, y, ok = plan.factor_front(plan.pack_H(H), b, LAM)
    assert ok
    Ld = plan.dense_L(Lval)
    assert np.abs(np.triu(Ld, 1)).max() == 0.0
    px, py = plan.perm_x_to_y()
    A = H + LAM * np.eye(plan.dim)
    Lx = np.zeros_like(Ld); Lx[np.ix_(px, px)] = Ld[np.ix_(py, py)]
    assert np.abs(Lx @ Lx.T - A).max() <= 1e-9 * np.abs(A).max()
    by = np.zeros(plan.dim); by[py] = b[px]
    yref = np.linalg.solve(Ld, by)
    assert np.abs(y[:plan.dim] - yref).max() <= 1e-9 * max(np.abs(yref).max(), 1e-30)
    x = plan.backward(Lval, y)
    xref = np.linalg.solve(A, b)
    assert np.abs(x - xref).max() <= 1e-7 * np.abs(xref).max()
    return Lx


def _budget_invariants(plan, budget):
    lds = _front_lds(plan)
    multi = 0
    for l in range(len(plan.plv_ptr) - 1):
        ps = plan.plv_pieces[plan.plv_ptr[l]:plan.plv_ptr[l + 1]]
        for p in ps:
            assert 8 * int(lds[p]) <= budget or _components(plan, int(p)) == 1, (l, int(p), 8 * int(lds[p]))
            multi += _components(plan, int(p)) > 1
        assert int(plan.plv_lds_ff[l]) == int(lds[ps].max())
    return multi


@pytest.fixture(scope="module")
def system(hip_lib):
    g = make_graph(600, 120, seed=11)
    plan, H, b = _plan_and_system(hip_lib, g, True, ENV)
    assert plan.front
    return g, plan, H, b, _solve(plan, H, b)


@pytest.mark.parametrize("budget", [20480, 12288])
def test_groups_stay_within_the_budget(hip_lib, system, budget):
    g, base, H, b, L0 = system
    plan, _, _ = _plan_and_system(hip_lib, g, True, dict(ENV, lds_budget=budget))
    assert plan.front and plan.lnz == base.lnz
    assert 8 * int(_front_lds(base)[base.plv_pieces].max()) > budget       # the plan without a budget has groups above it: the budget binds
    assert _budget_invariants(plan, budget) > 0                            # ... and still packs components side by side
    assert plan.npiece > base.npiece
    assert np.array_equal(_solve(plan, H, b), L0)


def test_budget_below_every_component(hip_lib, system):
    g, base, H, b, L0 = system
    plan, _, _ = _plan_and_system(hip_lib, g, True, dict(ENV, lds_budget=512))
    assert plan.front
    assert all(_components(plan, p) == 1 for p in range(plan.npiece))
    assert _budget_invariants(plan, 512) == 0
    assert np.array_equal(_solve(plan, H, b), L0)


def test_no_budget_is_the_plan_of_before(hip_lib, system):
    g, base, _, _, _ = system
    plan, _, _ = _plan_and_system(hip_lib, g, True, dict(ENV, lds_budget=0))
    for n in ARRAYS:
        a, c = getattr(base, n), getattr(plan, n)
        assert a.dtype == c.dtype and a.tobytes() == c.tobytes(), n


def test_mixed_batch_with_and_without_budget(hip_lib):
    """seven graphs of different sizes, one with plane landmarks, in one plan (B < 32: groups and front tables by option)"""
    import os
    from semantic_slam_amd import GraphSLAM
    from oracle.oracle import GraphProblem
    from test_chol_plan_cpu import _internal_order
    gs = [make_graph(40 + 5 * k, 8 + k, seed=70 + k) for k in range(6)] + [make_graph(150, 30, seed=5, landmark_kind="plane")]
    gps = [GraphProblem.from_synth(g, interleave=bool(i & 1)) for i, g in enumerate(gs)]
    handles = [GraphSLAM.from_problem(gp) for gp in gps]
    env = dict(ENV, front=1, cap_leaf=200, group_cap=1200, mid_width=4, tail_width=1)
    plans = []
    old = os.environ.get("SSLAM_CHOL_OPTS")
    try:
        for budget in (0, 6144):
            os.environ["SSLAM_CHOL_OPTS"] = ",".join(f"{k}={v}" for k, v in dict(env, lds_budget=budget).items())
            plans.append(Plan(hip_lib, handles))
    finally:
        if old is None: os.environ.pop("SSLAM_CHOL_OPTS")
        else: os.environ["SSLAM_CHOL_OPTS"] = old
    # block-diagonal system in the batch's internal row order: the pose rows of all graphs, then the landmark rows of all graphs
    Hs, bs, npose = [], [], []
    for gp in gps:
        U, bg = gp.linearize()
        Hg = (U + U.T).toarray() - np.diag(U.diagonal())
        idx, n = _internal_order(gp)
        Hs.append(Hg[np.ix_(idx, idx)]); bs.append(bg[idx])
        h, _ = gp.hessian_index()
        npose.append(6 * sum(1 for v in range(gp.nv) if gp.vtype[v] == 0 and h[v] >= 0))
    dim = sum(len(bg) for bg in bs)
    pos_p, pos_l = 0, sum(npose)
    H = np.zeros((dim, dim)); b = np.zeros(dim)
    for Hg, bg, npz in zip(Hs, bs, npose):
        w = np.concatenate([np.arange(pos_p, pos_p + npz), np.arange(pos_l, pos_l + len(bg) - npz)])
        pos_p += npz; pos_l += len(bg) - npz
        H[np.ix_(w, w)] = Hg; b[w] = bg
    a, c = plans
    assert a.front and c.front and a.dim == c.dim == dim and a.lnz == c.lnz
    assert c.npiece > a.npiece and _budget_invariants(c, 6144) >= 0
    assert np.array_equal(_solve(a, H, b), _solve(c, H, b))
