"""horn_rigid (csrc/sslam_math.hpp), the absolute-orientation solve of every scan-matching update, on its own and on the host:
tests/horn_check.cpp includes the header alone, reads the 16 sums k_reg_sums forms and prints T.  The reference is the same minimisation
in mpmath at 50 digits on the CENTRED data (the eigenvector of the largest eigenvalue of Horn's N, t = mean q - R mean p); the sums are
formed in float64 from points rounded to float32 first, as the device forms them.

Bounds, stated and not tuned:
* every case: |det R - 1| and |R^T R - I| within 1e-12, the bar of _proper in tests/test_registration_gpu.py, and every entry finite;
* mean offset 0: every entry of T within max(1e-13, 32 e_np) of the reference, e_np the error of the centred float64 NumPy Kabsch
  (registration_ref.kabsch) against the same reference on the same case -- two backward-stable solutions of one 3 x 3 problem;
* mean offsets of 30 m and 1000 m per axis: R within 32 * 2^-52 * (1 + |mean|^2 / spread^2) and t within that times max(1, |mean|),
  |mean| of the source points and spread^2 the smallest eigenvalue of their covariance: DESIGN section 4's model of the uncentred sums.
  At 30 m the flat 1e-9 of the GPU tests must hold too; at 1000 m it is not asked for (see the figures below);
* where the minimiser is not unique (collinear points) the residual sum |R p + t - q|^2 is compared with the reference's minimum, to
  1e-12 of sum |p'|^2 + |q'|^2 (centred): the residual is  that sum - 2 q^T N q,  |N| is below 1.5 times it, and an eigenvector of a
  matrix a few rounding errors from N misses the largest eigenvalue by as little: a few 2^-52 of that sum, a thousand times inside.

Figures measured with the clouds below (a 4 x 3 x 2 m box, 300 points, spread^2 about 0.3 m^2; largest over the 35 noisy cases):
  offset 0      R 7.3e-16, t 3.8e-16  (e_np up to 4.3e-15)
  offset 30 m   R 4.1e-13, t 1.5e-11  (model about 6e-11 and 3e-9; inside the flat 1e-9)
  offset 1000 m R 5.0e-10, t 5.1e-7   (model about 7e-8 and 1.2e-4; t is OUTSIDE 1e-9 -- the envelope include/sslam.h states for the call)"""
import math
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

from registration_ref import kabsch, motion_T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EPS = 2.0 ** -52
ANGLES = [("0", 0.0), ("1e-8", 1e-8), ("0.05", 0.05), ("pi/2", math.pi / 2), ("2pi/3", 2 * math.pi / 3), ("pi-1e-6", math.pi - 1e-6), ("pi", math.pi)]
AXES = [("z", (0, 0, 1)), ("x", (1, 0, 0)), ("y", (0, 1, 0)), ("g", (0.2, -0.3, 0.93)), ("d", (1, 1, 1))]
OFFSETS = [0.0, 30.0, 1000.0]
TRANSLATION = (3.0, -2.0, 1.5)
HALF = np.array([2.0, 1.5, 1.0])          # the half sides of the box the points are drawn from
NOISE = 0.002


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _pair(p, T, rng, noise, offset):
    """(p, q) in float32: q = R p + t, `noise` m of Gaussian noise on both, both shifted by `offset` on every axis, then rounded"""
    R, t = T[:9].reshape(3, 3), T[9:]
    q = p @ R.T + t
    if noise:
        p, q = p + rng.normal(0.0, noise, p.shape), q + rng.normal(0.0, noise, q.shape)
    return (p + offset).astype(np.float32), (q + offset).astype(np.float32)


def _noisy(angle, axis, offset, seed):
    rng = np.random.default_rng(seed)
    return _pair(rng.uniform(-HALF, HALF, (300, 3)), motion_T(angle, axis, TRANSLATION), rng, NOISE, offset)


def _lattice(turn, offset):
    """a full 10 x 6 x 5 integer grid (its covariance is exactly diagonal) and its image under a signed permutation matrix and an integer
    translation: every sum is an integer or a half, exact in float64"""
    g = np.stack(np.meshgrid(np.arange(10) - 5, np.arange(6) - 3, np.arange(5) - 2, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    R = {"I": np.diag([1.0, 1, 1]), "pi_z": np.diag([-1.0, -1, 1]), "pi_x": np.diag([1.0, -1, -1]), "pi_y": np.diag([-1.0, 1, -1]),
         "quarter_z": np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])}[turn]
    T = np.concatenate([R.reshape(-1), [3.0, -2.0, 1.0]])
    return _pair(g, T, None, 0.0, offset) + (T,)


def _slab(seed, thickness):
    """points of the plane z = 0 turned about z and moved inside it, noise inside the plane; `thickness` m of noise across it (0: the
    cross-covariance has rank 2 exactly)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-HALF, HALF, (300, 3)) * [1, 1, 0]
    q = p @ motion_T(0.7, (0, 0, 1), (3.0, -2.0, 0.0))[:9].reshape(3, 3).T + [3.0, -2.0, 0.0]
    p[:, :2] += rng.normal(0.0, NOISE, (300, 2)); q[:, :2] += rng.normal(0.0, NOISE, (300, 2))
    p[:, 2] += rng.normal(0.0, thickness, 300); q[:, 2] += rng.normal(0.0, thickness, 300)
    return p.astype(np.float32), q.astype(np.float32)


def _line(seed, noise):
    """source points exactly on a line (multiples of (1, 2, -1) / 8: exact in float32), the targets their image plus noise"""
    rng = np.random.default_rng(seed)
    p = rng.integers(-40, 41, (300, 1)) * np.array([[0.125, 0.25, -0.125]])
    T = motion_T(2.2, (0.2, -0.3, 0.93), TRANSLATION)
    q = p @ T[:9].reshape(3, 3).T + T[9:] + rng.normal(0.0, noise, (300, 3))
    return p.astype(np.float32), q.astype(np.float32)


def _point(seed):
    """every source point the same, on a 1/64 lattice like the targets: the sums and S = 0 are exact"""
    rng = np.random.default_rng(seed)
    p = np.tile(np.array([[0.375, -1.25, 0.734375]]), (300, 1))
    q = rng.integers(-256, 257, (300, 3)) / 64.0 + TRANSLATION
    return p.astype(np.float32), q.astype(np.float32)


def sums_of(p, q):
    """the 16 sums of k_reg_sums, in float64 from the float32 points (every product of two widened floats is exact)"""
    P, Q = p.astype(np.float64), q.astype(np.float64)
    M = [(P[:, a] * Q[:, b]).sum() for a in range(3) for b in range(3)]
    return np.array(list(P.sum(0)) + list(Q.sum(0)) + M + [float(len(P))])


# ---- the reference at 50 digits ----------------------------------------------------------------------------------------------------------
def _centred(p, q):
    P = [[mp.mpf(float(v)) for v in row] for row in p]
    Q = [[mp.mpf(float(v)) for v in row] for row in q]
    n = len(P)
    pm = [mp.fsum(r[a] for r in P) / n for a in range(3)]
    qm = [mp.fsum(r[a] for r in Q) / n for a in range(3)]
    Pc = [[r[a] - pm[a] for a in range(3)] for r in P]
    Qc = [[r[a] - qm[a] for a in range(3)] for r in Q]
    return Pc, Qc, pm, qm


def _rotation_of(w, x, y, z):
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def reference(p, q):
    """dict: T (12 mpf), S (3 x 3 mpf, centred), lam (eigenvalues of N, descending), minimum (the least residual), scale (sum |p'|^2 +
    |q'|^2), and residual(T) -> sum |R p + t - q|^2 of any T"""
    with mp.workdps(50):
        Pc, Qc, pm, qm = _centred(p, q)
        S = [[mp.fsum(a[r] * b[c] for a, b in zip(Pc, Qc)) for c in range(3)] for r in range(3)]
        N = mp.matrix([[S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]],
                       [S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]],
                       [S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]],
                       [S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]]])
        E, V = mp.eigsy(N)
        k = max(range(4), key=lambda i: E[i])
        v = [V[i, k] for i in range(4)]
        nv = mp.sqrt(mp.fsum(c * c for c in v))
        R = _rotation_of(*[c / nv for c in v])
        t = [qm[r] - mp.fsum(R[r][c] * pm[c] for c in range(3)) for r in range(3)]
        scale = mp.fsum(c * c for r in Pc for c in r) + mp.fsum(c * c for r in Qc for c in r)

        def residual(T):
            with mp.workdps(50):
                T = [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in T]
                Rm = [[T[3 * r + c] for c in range(3)] for r in range(3)]
                # R p + t - q = R p' - q' + (R pm + t - qm)
                d = [mp.fsum(Rm[r][c] * pm[c] for c in range(3)) + T[9 + r] - qm[r] for r in range(3)]
                return mp.fsum((mp.fsum(Rm[r][c] * a[c] for c in range(3)) - b[r] + d[r]) ** 2 for a, b in zip(Pc, Qc) for r in range(3))
        return dict(T=[R[r][c] for r in range(3) for c in range(3)] + t, S=S, lam=sorted((E[i] for i in range(4)), reverse=True),
                    minimum=scale - 2 * E[k], scale=scale, residual=residual, pm=pm, qm=qm)


def _error(T, ref):
    """(largest |entry| difference of R, of t) between 12 doubles and the reference"""
    with mp.workdps(50):
        d = [abs(mp.mpf(float(a)) - b) for a, b in zip(T, ref["T"])]
        return float(max(d[:9])), float(max(d[9:]))


def _numpy_error(p, q, ref):
    R, t, _ = kabsch(p.astype(np.float64), q.astype(np.float64))
    return max(_error(np.concatenate([R.reshape(-1), t]), ref))


# ---- the program -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def horn(tmp_path_factory):
    d = tmp_path_factory.mktemp("horn")
    exe = str(d / "horn_check")
    # the host half of a HIP compile (the header includes hip/hip_runtime.h), optimised and contracted as csrc/Makefile builds sslam_seg.hip
    subprocess.check_call([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O3", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                           os.path.join(ROOT, "tests", "horn_check.cpp"), "-o", exe])
    count = [0]

    def run(rows):
        count[0] += 1
        case = d / f"case{count[0]}.txt"
        case.write_text("".join(" ".join(float(v).hex() for v in r) + "\n" for r in rows))
        out = subprocess.run([exe, str(case)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        Ts = [np.array([float.fromhex(w) for w in line.split()]) for line in out.stdout.splitlines()]
        assert len(Ts) == len(rows) and all(len(T) == 12 for T in Ts)
        return Ts
    return run


def _proper(T, what):
    assert np.isfinite(T).all(), what
    R = T[:9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12, what
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, what


def _model(p):
    """(bound on R, bound on t) of DESIGN section 4's model for uncentred sums"""
    P = p.astype(np.float64)
    mean = np.linalg.norm(P.mean(0))
    spread2 = np.linalg.eigvalsh(np.cov(P.T, bias=True))[0]
    r = 32 * EPS * (1.0 + mean * mean / spread2)
    return r, r * max(1.0, mean)


def _check(T, p, q, offset, what, worst):
    """the assertions of a case whose minimiser is unique"""
    _proper(T, what)
    ref = reference(p, q)
    assert ref["lam"][0] - ref["lam"][1] > 1e-3 * ref["lam"][0], what          # the largest eigenvalue is simple: R is determined
    er, et = _error(T, ref)
    e_np = _numpy_error(p, q, ref)
    if offset == 0.0:
        br = bt = max(1e-13, 32 * e_np)
    else:
        br, bt = _model(p)
    print(f"{what}: e_np {e_np:.2e}  horn R {er:.2e} t {et:.2e}  bounds R {br:.2e} t {bt:.2e}")
    w = worst.setdefault(offset, [0.0, 0.0, 0.0])
    w[:] = [max(w[0], er), max(w[1], et), max(w[2], e_np)]
    assert er <= br and et <= bt, (what, er, et, br, bt)
    if offset == 30.0:
        assert max(er, et) <= 1e-9, (what, er, et)
    return ref


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis_name,axis", AXES)
def test_noisy_clouds_at_every_angle_and_offset(horn, axis_name, axis):
    cases = [(f"{an} about {axis_name} at {off:g} m", _noisy(a, axis, off, 1000 + 10 * i + j), off)
             for i, (an, a) in enumerate(ANGLES) for j, off in enumerate(OFFSETS)]
    Ts = horn([sums_of(p, q) for _, (p, q), _ in cases])
    worst = {}
    for (what, (p, q), off), T in zip(cases, Ts):
        _check(T, p, q, off, what, worst)
    for off, (er, et, e_np) in worst.items():
        print(f"envelope about {axis_name}, offset {off:g} m: R {er:.2e} t {et:.2e} (e_np {e_np:.2e})")


@pytest.mark.parametrize("turn", ["I", "pi_z", "pi_x", "pi_y", "quarter_z"])
def test_noise_free_lattice_is_solved_exactly(horn, turn):
    """integer points: every sum is exact, and for the half turns about the coordinate axes N is diagonal before the first sweep -- the
    loop ends at once and T is whatever the pick makes of V = I: exactly the signed permutation and the integer translation"""
    cases = [_lattice(turn, off) for off in OFFSETS]
    Ts = horn([sums_of(p, q) for p, q, _ in cases])
    for (p, q, T_true), T, off in zip(cases, Ts, OFFSETS):
        what = f"lattice {turn} at {off:g} m"
        ref = _check(T, p, q, off, what, {})
        if turn != "quarter_z":
            S = ref["S"]
            assert all(S[r][c] == 0 for r in range(3) for c in range(3) if r != c), what       # N is diagonal
            s = sums_of(p, q)
            assert all(s[6 + 3 * r + c] - s[r] * s[3 + c] / s[15] == 0 for r in range(3) for c in range(3) if r != c), what   # in float64 too
        R = T_true[:9].reshape(3, 3)
        want = np.concatenate([T_true[:9], T_true[9:] + off - R @ np.full(3, off)])
        if turn == "quarter_z":
            assert np.abs(T - want).max() <= (1e-13 if off == 0.0 else 1e-9 * off), what
        else:
            assert (T == want).all(), (what, T, want)                # +0 and -0 compare equal


def test_coplanar_points_both_signs_of_det_S(horn):
    """the plane z = 0 exactly (rank 2), and slabs 2 mm thick whose det S is positive and negative: with the negative one the SVD form
    needs its determinant correction, the quaternion form nothing"""
    cases = [("plane", _slab(5, 0.0))] + [(f"slab {s}", _slab(s, NOISE)) for s in range(20, 26)]
    Ts = horn([sums_of(p, q) for _, (p, q) in cases])
    signs = []
    for (what, (p, q)), T in zip(cases, Ts):
        ref = _check(T, p, q, 0.0, what, {})
        with mp.workdps(50):
            det = mp.det(mp.matrix(ref["S"]))
        signs.append(0 if det == 0 else (1 if det > 0 else -1))
        H = (p - p.mean(0)).astype(np.float64).T @ (q - q.mean(0)).astype(np.float64)
        U, _, Vt = np.linalg.svd(H)
        print(what, "det S", mp.nstr(det, 3), "det V U^T %.3f" % np.linalg.det(Vt.T @ U.T))
    assert signs[0] == 0 and 1 in signs[1:] and -1 in signs[1:], signs


@pytest.mark.parametrize("noise", [0.0, NOISE])
def test_collinear_points_reach_the_least_residual(horn, noise):
    p, q = _line(41, noise)
    (T,) = horn([sums_of(p, q)])
    _proper(T, "line")
    ref = reference(p, q)
    assert ref["lam"][0] - ref["lam"][1] <= 1e-40 * ref["scale"]                # the largest eigenvalue is double: R is not unique
    excess = float(ref["residual"](T) - ref["minimum"])
    print(f"line, noise {noise}: residual {mp.nstr(ref['residual'](T), 8)}, least {mp.nstr(ref['minimum'], 8)}, excess {excess:.2e}, scale {float(ref['scale']):.3e}")
    assert abs(float(ref["residual"](ref["T"]) - ref["minimum"])) <= 1e-30 * float(ref["scale"])   # the reference's two ways to its minimum agree
    # two-sided: an R a rounding error from orthogonal can undercut the least residual over rotations by as much
    assert -1e-12 * float(ref["scale"]) <= excess <= 1e-12 * float(ref["scale"])


@pytest.mark.parametrize("line,first", [(0, 2), (1, 1), (2, 1)])
def test_noise_free_half_turn_of_a_lattice_line(horn, line, first):
    """integer points on a coordinate axis and their half turn about another: N is diagonal with its largest eigenvalue TWICE (the half
    turns about both other axes are minimisers, residual 0).  No sweep runs, and the pick among equals decides: the header promises the
    first, and the bits of every degenerate registration hang on it"""
    other = [a for a in range(3) if a != line]
    p = np.zeros((300, 3))
    p[:, line] = np.arange(300) - 150
    R = np.diag([1.0 if a == other[0] else -1.0 for a in range(3)])             # the half turn about the lower of the two other axes
    t = np.array([3.0, -2.0, 1.0])
    p, q = p.astype(np.float32), (p @ R.T + t).astype(np.float32)
    s = sums_of(p, q)
    S = [[s[6 + 3 * r + c] - s[r] * s[3 + c] / s[15] for c in range(3)] for r in range(3)]
    assert all(S[r][c] == 0 for r in range(3) for c in range(3) if (r, c) != (line, line)) and S[line][line] < 0
    (T,) = horn([s])
    _proper(T, line)
    ref = reference(p, q)
    assert ref["lam"][0] == ref["lam"][1] and ref["minimum"] == 0 and ref["residual"](T) == 0
    want = np.diag([1.0 if a == first - 1 else -1.0 for a in range(3)])         # column `first` of V = I: order w, x, y, z
    assert (T[:9].reshape(3, 3) == want).all() and (T[9:] == t).all(), T         # on the line both half turns are p -> -p: the same t


def test_equal_source_points_give_the_identity(horn):
    p, q = _point(43)
    s = sums_of(p, q)
    assert all(s[6 + 3 * r + c] - s[r] * s[3 + c] / s[15] == 0 for r in range(3) for c in range(3))   # S = 0 exactly, in float64
    (T,) = horn([s])
    assert (T[:9] == np.eye(3).reshape(-1)).all(), T                            # the first among equals: w = 1
    want = q.astype(np.float64).mean(0) - p.astype(np.float64).mean(0)
    assert np.abs(T[9:] - want).max() <= 1e-13


def test_three_points(horn):
    cases = []
    for k, (an, a) in enumerate(ANGLES):
        rng = np.random.default_rng(70 + k)
        cases.append((f"n = 3, {an}", _pair(rng.uniform(-HALF, HALF, (3, 3)), motion_T(a, (0.2, -0.3, 0.93), TRANSLATION), rng, NOISE, 0.0)))
    Ts = horn([sums_of(p, q) for _, (p, q) in cases])
    for (what, (p, q)), T in zip(cases, Ts):
        _check(T, p, q, 0.0, what, {})
