"""Reference for linear-solve tests, CPU only: (H + lam I) x = b to extended precision.

refined_solve factors once in double (SuperLU) and refines three times with the residual accumulated in np.longdouble (x87 80-bit: 64-bit
mantissa), which takes the solution of these well-conditioned SLAM systems to ~1e-19 relative -- pinned against mpmath at 50 digits by
tests/test_batch_solve_cpu.py.  double_error is what an honest double factorisation does on the very same system: the yardstick the GPU
tests scale their bounds by, computed by the reference alone."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

_EPS = float(np.finfo(np.longdouble).eps)
assert _EPS < 2e-19, f"np.longdouble is not an extended-precision type here (eps {_EPS:.3g}): the solve reference needs a 64-bit mantissa"


def _triplets(H_upper, lam):
    """COO triplets (row, col, value) of the full symmetric H + lam I from its upper triangle"""
    U = sp.coo_matrix(H_upper)
    U.sum_duplicates()
    keep = U.row <= U.col
    r, c, v = U.row[keep], U.col[keep], U.data[keep]
    off = r != c
    n = U.shape[0]
    d = np.arange(n)
    rows = np.concatenate([r, c[off], d])
    cols = np.concatenate([c, r[off], d])
    vals = np.concatenate([v, v[off], np.full(n, float(lam))])
    return n, rows, cols, vals


def residual(H_upper, b, lam, x):
    """b - (H + lam I) x, products and sums in np.longdouble"""
    n, rows, cols, vals = _triplets(H_upper, lam)
    res = np.asarray(b, np.longdouble).copy()
    np.subtract.at(res, rows, vals.astype(np.longdouble) * np.asarray(x, np.longdouble)[cols])
    return res


def refined_solve(H_upper, b, lam, rounds=3):
    """-> (x as np.longdouble, final residual b - (H + lam I) x as np.longdouble)"""
    n, rows, cols, vals = _triplets(H_upper, lam)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsc()
    lu = spla.splu(A)
    vl = vals.astype(np.longdouble)
    bl = np.asarray(b, np.longdouble)
    x = lu.solve(np.asarray(b, np.float64)).astype(np.longdouble)
    for _ in range(rounds):
        res = bl.copy()
        np.subtract.at(res, rows, vl * x[cols])
        x = x + lu.solve(res.astype(np.float64)).astype(np.longdouble)
    res = bl.copy()
    np.subtract.at(res, rows, vl * x[cols])
    return x, res


def plain_splu(H_upper, b, lam):
    n, rows, cols, vals = _triplets(H_upper, lam)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsc()
    return spla.splu(A).solve(np.asarray(b, np.float64))


def rel_error(x, x_ref):
    """max |x - x_ref| / max |x_ref|, in np.longdouble"""
    xr = np.asarray(x_ref, np.longdouble)
    return float(np.abs(np.asarray(x, np.longdouble) - xr).max() / np.abs(xr).max())


def double_error(gp, H_upper, b, lam, x_ref, x_oracle=None):
    """What an honest double factorisation does on this system: the larger of the max-norm relative errors against x_ref of the oracle's
    own double Cholesky (gp.solve(lam): the oracle linearises the same graph itself) and of SuperLU without refinement."""
    return max(rel_error(gp.solve(lam) if x_oracle is None else x_oracle, x_ref), rel_error(plain_splu(H_upper, b, lam), x_ref))
