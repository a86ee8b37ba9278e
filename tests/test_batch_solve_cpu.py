"""The reference of the batch-solve tests itself (tests/solve_ref.py): iterative refinement with np.longdouble residuals against mpmath
at 50 digits, and its residual on a system of a few thousand unknowns.  tests/test_batch_solve_gpu.py compares the HIP solve with it."""
import numpy as np
import pytest

import solve_ref as R
from semantic_slam_amd.synth import make_graph
from oracle.oracle import GraphProblem


@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_refined_solve_matches_mpmath_at_50_digits(lam):
    import mpmath
    gp = GraphProblem.from_synth(make_graph(10, 2, seed=1), interleave=True)
    U, b = gp.linearize()
    n = U.shape[0]
    assert n == 60
    x, res = R.refined_solve(U, b, lam)
    assert x.dtype == np.longdouble and res.dtype == np.longdouble
    old = mpmath.mp.dps
    mpmath.mp.dps = 50
    try:
        Ud = U.toarray()
        Hd = Ud + np.triu(Ud, 1).T
        A = mpmath.matrix(n, n)
        for i in range(n):
            for j in range(n):
                if Hd[i, j] != 0.0:
                    A[i, j] = mpmath.mpf(float(Hd[i, j]))
            A[i, i] += mpmath.mpf(float(lam))
        xm = mpmath.lu_solve(A, mpmath.matrix([mpmath.mpf(float(v)) for v in b]))
        scale = max(abs(v) for v in xm)
        # a longdouble holds 64 bits: through (hi, lo) doubles it reaches mpmath without loss
        err = max(abs(mpmath.mpf(float(np.float64(v))) + mpmath.mpf(float(v - np.longdouble(np.float64(v)))) - m) for v, m in zip(x, xm))
        rel = float(err / scale)
    finally:
        mpmath.mp.dps = old
    print(f"lambda {lam}: refined_solve vs mpmath, relative {rel:.3g}")
    assert rel <= 1e-17


def test_refined_solve_residual_on_a_large_system():
    gp = GraphProblem.from_synth(make_graph(600, 120, seed=2), interleave=True)
    U, b = gp.linearize()
    for lam in (0.0, 1e-3, 5.0):
        x, res = R.refined_solve(U, b, lam)
        bound = 1e-17 * float(np.abs(b).max()) * U.shape[0]
        print(f"lambda {lam}: residual {float(np.abs(res).max()):.3g}, bound {bound:.3g}")
        assert float(np.abs(res).max()) <= bound
        assert np.array_equal(res, R.residual(U, b, lam, x))
        # and what a double factorisation does on it: orders of magnitude above the reference, orders below the project's 1e-9 bar
        de = R.double_error(gp, U, b, lam, x)
        assert 1e-17 < de < 1e-10, de
