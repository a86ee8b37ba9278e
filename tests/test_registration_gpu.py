"""sslam_seg_register_pairs (k_nn_pairs + k_reg_sums + k_reg_step, k_nn_finish at the end), its Python mirror and the C++ shim's ScanMatcher
on the GPU.  Reference: tests/registration_ref.py; tests/test_registration_cpu.py shows on the reference alone that the scenes used here
converge, are well conditioned, and that the bounded and coplanar cases bite.
Bounds, stated and not tuned: the device is driven ONE iteration at a time and each update is compared with step_ref from the SAME T_k,
every entry within 1e-9 -- the bar the point-to-plane ICP is held to against oracle/np_icp.py.  (The correspondences of the two are bitwise
equal, so what differs is the rounding of two double-precision solutions of one 3 x 3 problem: about 1e-15 in practice.)  Two free-running
trajectories are never compared: they may part at a float-rounding tie.  Everything else -- one call against many, the final pass against
sslam_seg_fitness_scores, a pair alone against the same pair in a batch, under another target split, and repeated -- is BITWISE.
The six scenes of CASES start from the identity and move by 0.05 rad; the scenes of FAR start from start_T(name), 0.05 rad from a relative
pose of 2.2 rad to a half turn about z, x, y or a skew axis, two of them with both clouds 30 m from the origin: what loop closing hands
the matcher when the robot comes back along its own track."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fitness_ref import DBL_MAX, IDENTITY_T, qmat, skew_T
from registration_ref import (BOUNDED_MAX_CORR2, ERR_NUMERIC, FAR_SCENES, HALF_TURNS, MAX_ITERATIONS, far_scene, fast_pair, scene, start_T, step_ref,
                              two_correspondences)

pytestmark = pytest.mark.gpu

# (scene, max_corr2): 1500 sources span two query blocks of 1024 and six runs of 256, the last partial; 300 x 257 is one block and two runs
CASES = [("large", None), ("small", None), ("small", BOUNDED_MAX_CORR2), ("mixed", None), ("wall", None), ("floor", None)]
FAR = list(FAR_SCENES)      # registered from start_T(name): relative rotations of 2.2 rad to a half turn, clouds 30 m from the origin


def _scene(name):
    return far_scene(name) if name in FAR_SCENES else scene(name)


@pytest.fixture(scope="module")
def seg(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    return PointCloudSegmentation()


def _with_chunk(chunk, f):
    old = os.environ.get("SSLAM_FITNESS_OPTS")
    os.environ["SSLAM_FITNESS_OPTS"] = f"chunk={chunk}"
    try:
        return f()
    finally:
        if old is None:
            os.environ.pop("SSLAM_FITNESS_OPTS")
        else:
            os.environ["SSLAM_FITNESS_OPTS"] = old


def _one(seg, tg, sr, T0=None, max_corr2=None, max_iterations=MAX_ITERATIONS, epsilon=0.0):
    """(Registration, nn index, nn d2) of one pair on its own"""
    res, nn = seg.register_pairs([tg, sr], [(0, 1, T0, max_corr2)], max_iterations=max_iterations, epsilon=epsilon, return_nn=True)
    return res[0], nn[0][0], nn[0][1]


def _same(a, b):
    """two (Registration, index, d2) triples, bit for bit"""
    return (a[0].T.tobytes() == b[0].T.tobytes() and a[0].score == b[0].score and a[0].used == b[0].used and a[0].iterations == b[0].iterations
            and a[0].converged == b[0].converged and a[0].status == b[0].status and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes())


def _proper(T, what):
    R = T[:9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12, what
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, what


_LOCKSTEP = {}


def _lockstep(seg, name, max_corr2, start=None):
    """the device driven one iteration at a time from `start` (the identity by default) until it reports convergence: [T_0, T_1, ...],
    each update checked against step_ref from the same T_k.  Computed once per case and shared."""
    cache = (name, max_corr2, None if start is None else np.asarray(start, np.float64).tobytes())
    if cache in _LOCKSTEP:
        return _LOCKSTEP[cache]
    key = (name, max_corr2)
    tg, sr, _ = _scene(name)
    Ts = [IDENTITY_T.copy() if start is None else np.array(start, np.float64)]
    worst = 0.0
    for k in range(MAX_ITERATIONS):
        r, _, _ = _one(seg, tg, sr, Ts[-1], max_corr2, max_iterations=1)
        ref, n = step_ref(tg, sr, Ts[-1], max_corr2)
        assert r.status == 0 and r.iterations == 1 and n >= 3, (key, k)
        err = float(np.abs(r.T - ref).max())
        worst = max(worst, err)
        assert err <= 1e-9, (key, k, err)
        _proper(r.T, (key, k))
        Ts.append(r.T)
        if r.converged:
            assert r.T.tobytes() == Ts[-2].tobytes(), (key, k)                  # epsilon = 0: converged means T repeated bit for bit
            break
        assert r.T.tobytes() != Ts[-2].tobytes(), (key, k)
    else:
        raise AssertionError(f"{key}: no convergence within {MAX_ITERATIONS} single iterations")
    print(f"{name} max_corr2 {max_corr2}: {len(Ts) - 1} iterations, largest |T_device - T_ref| per step {worst:.3e}")
    _LOCKSTEP[cache] = Ts
    return Ts


@pytest.mark.parametrize("name,max_corr2", CASES)
def test_lockstep_step_parity(seg, name, max_corr2):
    Ts = _lockstep(seg, name, max_corr2)
    assert 3 <= len(Ts) - 1 <= MAX_ITERATIONS
    assert np.abs(Ts[-1] - IDENTITY_T).max() > 1e-2                             # the loop went somewhere


@pytest.mark.parametrize("name", FAR)
def test_lockstep_step_parity_far_from_the_identity(seg, name):
    """every update from start_T on: T0 = inverse(new) o old of a robot that comes back along its own track is nowhere near the identity"""
    T0 = start_T(name)
    Ts = _lockstep(seg, name, None, T0)
    assert 3 <= len(Ts) - 1 <= MAX_ITERATIONS
    assert np.abs(Ts[-1] - T0).max() > 1e-3                                     # the loop went somewhere
    if name in HALF_TURNS:
        assert np.trace(Ts[-1][:9].reshape(3, 3)) < 0


def _one_call_equals_many(seg, name, max_corr2, T0):
    Ts = _lockstep(seg, name, max_corr2, T0)
    tg, sr, _ = _scene(name)
    n = len(Ts) - 1
    r, _, _ = _one(seg, tg, sr, T0, max_corr2)
    assert r.T.tobytes() == Ts[-1].tobytes() and r.iterations == n and r.converged == 1 and r.status == 0
    for cap in (1, n - 1, 9):                                                   # stopped by the cap, across a chunk of 8 iterations too
        if cap < n:
            c, _, _ = _one(seg, tg, sr, T0, max_corr2, max_iterations=cap)
            assert c.T.tobytes() == Ts[cap].tobytes() and c.iterations == cap and c.converged == 0 and c.status == 0, cap
    e, _, _ = _one(seg, tg, sr, T0, max_corr2, epsilon=1e-4)                     # a real epsilon ends the same trajectory earlier
    moved = [np.abs(Ts[k + 1] - Ts[k]).max() for k in range(n)]
    first = next(k for k, m in enumerate(moved) if m <= 1e-4)
    assert e.converged == 1 and e.iterations == first + 1 and e.T.tobytes() == Ts[first + 1].tobytes()


@pytest.mark.parametrize("name,max_corr2", CASES)
def test_one_call_equals_many(seg, name, max_corr2):
    _one_call_equals_many(seg, name, max_corr2, None)


@pytest.mark.parametrize("name", FAR)
def test_one_call_equals_many_far_from_the_identity(seg, name):
    _one_call_equals_many(seg, name, None, start_T(name))


def test_mixed_batch_independence(seg):
    """a half-turn pair, a pair 30 m from the origin, a small motion from the identity and a pair with too few correspondences in one
    call: each bitwise what it is alone, repeated, and under another target split"""
    htg, hsr, _ = far_scene("half_y")
    ftg, fsr, _ = far_scene("far")
    stg, ssr, _ = scene("small")
    ttg, tsr, tmc = two_correspondences()
    clouds = [htg, hsr, ftg, fsr, stg, ssr, ttg, tsr]
    pairs = [(0, 1, start_T("half_y"), None), (2, 3, start_T("far"), None), (4, 5, None, None), (6, 7, None, tmc)]
    res, nn = seg.register_pairs(clouds, pairs, max_iterations=MAX_ITERATIONS, return_nn=True)
    again = seg.register_pairs(clouds, pairs, max_iterations=MAX_ITERATIONS, return_nn=True)
    split = _with_chunk(256, lambda: seg.register_pairs(clouds, pairs, max_iterations=MAX_ITERATIONS, return_nn=True))
    for k, (t, s, T0, mc) in enumerate(pairs):
        got = (res[k], nn[k][0], nn[k][1])
        if k < 3:
            assert res[k].status == 0 and res[k].converged == 1 and res[k].iterations >= 3, k
        else:
            assert res[k].status == ERR_NUMERIC and res[k].iterations == 0 and res[k].T.tobytes() == IDENTITY_T.tobytes()
        assert _same(got, _one(seg, clouds[t], clouds[s], T0, mc)), k
        assert _same(got, (again[0][k], again[1][k][0], again[1][k][1])), k
        assert _same(got, (split[0][k], split[1][k][0], split[1][k][1])), k
        assert _same(got, _with_chunk(256, lambda: _one(seg, clouds[t], clouds[s], T0, mc))), k
    assert np.trace(res[0].T[:9].reshape(3, 3)) < -0.9 and np.abs(res[1].T[9:]).max() > 1.0    # a half turn; a lever arm of 30 m
    assert len({r.iterations for r in res}) >= 3                                 # the pairs finish at different times


def test_sign_of_the_start_quaternion_is_not_seen(seg):
    """T0 is a matrix: the same rotation built from q and from -q is the same twelve doubles, and nothing on the way to the result goes
    through a quaternion whose sign could matter -- at a half turn, where w is about 0 and its sign arbitrary"""
    from loop_ref import measurement_of_T
    for name in ("half_z", "half_g"):
        tg, sr, _ = far_scene(name)
        z = measurement_of_T(start_T(name))
        q = z[3:] / np.linalg.norm(z[3:])
        assert abs(q[3]) < 0.2
        plus, minus = np.array(list(qmat(q)) + list(z[:3])), np.array(list(qmat(-q)) + list(z[:3]))
        assert plus.tobytes() == minus.tobytes() and np.abs(plus - start_T(name)).max() < 1e-12
        a, b = _one(seg, tg, sr, plus), _one(seg, tg, sr, minus)
        assert _same(a, b) and a[0].status == 0 and a[0].converged == 1 and np.trace(a[0].T[:9].reshape(3, 3)) < -0.9


@pytest.mark.parametrize("name,max_corr2", CASES)
def test_final_pass_is_the_fitness_pass(seg, name, max_corr2):
    tg, sr, _ = scene(name)
    r, idx, d2 = _one(seg, tg, sr, None, max_corr2)
    score, used, nn = seg.fitness_scores([tg, sr], [(0, 1, r.T, max_corr2)], return_nn=True)
    assert r.score == score[0] and r.used == used[0] and np.array_equal(idx, nn[0][0]) and d2.tobytes() == nn[0][1].tobytes()
    assert 0 < r.score < DBL_MAX and (r.used == len(sr) if max_corr2 is None else 3 <= r.used < len(sr))
    T0 = skew_T(0.03, (0.1, 0.9, -0.2), (0.02, 0.01, -0.03))                     # max_iterations = 0: the fitness pass at T0
    z, zidx, zd2 = _one(seg, tg, sr, T0, max_corr2, max_iterations=0)
    score, used, nn = seg.fitness_scores([tg, sr], [(0, 1, T0, max_corr2)], return_nn=True)
    assert z.T.tobytes() == T0.tobytes() and (z.iterations, z.converged, z.status) == (0, 0, 0)
    assert z.score == score[0] and z.used == used[0] and np.array_equal(zidx, nn[0][0]) and zd2.tobytes() == nn[0][1].tobytes()


def test_batch_independence_and_repeatability(seg):
    ltg, lsr, _ = scene("large")
    stg, ssr, _ = scene("small")
    _, msr, _ = scene("mixed")
    clouds = [ltg, lsr, stg, ssr, msr]
    Tg = skew_T(0.02, (0.3, -0.5, 0.8), (0.01, -0.02, 0.01))
    pairs = [(0, 1, None, None), (2, 3, None, None), (2, 3, None, BOUNDED_MAX_CORR2), (2, 4, Tg, None), (0, 3, Tg, 0.02)]   # clouds 0, 2, 3 serve several pairs
    res, nn = seg.register_pairs(clouds, pairs, max_iterations=MAX_ITERATIONS, return_nn=True)
    again = seg.register_pairs(clouds, pairs, max_iterations=MAX_ITERATIONS, return_nn=True)
    split = _with_chunk(256, lambda: seg.register_pairs(clouds, pairs, max_iterations=MAX_ITERATIONS, return_nn=True))
    assert len({r.iterations for r in res}) >= 3                                 # the pairs finish at different times
    for k, (t, s, T0, mc) in enumerate(pairs):
        got = (res[k], nn[k][0], nn[k][1])
        assert res[k].status == 0 and res[k].converged == 1 and res[k].iterations >= 3, k
        assert _same(got, _one(seg, clouds[t], clouds[s], T0, mc)), k
        assert _same(got, (again[0][k], again[1][k][0], again[1][k][1])), k
        assert _same(got, (split[0][k], split[1][k][0], split[1][k][1])), k
        assert _same(got, _with_chunk(256, lambda: _one(seg, clouds[t], clouds[s], T0, mc))), k
    assert seg.last_registration_ms > 0


def test_non_finite_points_take_no_part(seg):
    tg, sr, _ = scene("small")
    tg, sr = tg.copy(), sr.copy()
    rng = np.random.default_rng(31)
    for a in (tg, sr):
        bad = rng.choice(len(a), len(a) // 20, replace=False)
        a[bad, rng.integers(0, 3, len(bad))] = np.nan
        a[rng.choice(len(a), 3, replace=False), 1] = np.inf
        a[rng.choice(len(a), 2, replace=False), 2] = -np.inf
    sbad, tbad = ~np.isfinite(sr).all(1), ~np.isfinite(tg).all(1)
    assert sbad.sum() >= 15 and tbad.sum() >= 12
    T = IDENTITY_T
    for k in range(3):                                                          # three updates in lockstep with the reference
        r, idx, d2 = _one(seg, tg, sr, T, None, max_iterations=1)
        ref, n = step_ref(tg, sr, T, None)
        assert n == (~sbad).sum() and r.status == 0 and np.isfinite(r.T).all()
        assert np.abs(r.T - ref).max() <= 1e-9, k
        T = r.T
    assert r.used == (~sbad).sum() and (idx[sbad] == -1).all() and (d2[sbad] == -1.0).all() and (idx[~sbad] >= 0).all()
    assert not tbad[idx[~sbad]].any()                                           # a non-finite target is never chosen
    nan_src = np.full((40, 3), np.nan, np.float32)
    empty = np.zeros((0, 3), np.float32)
    for t, s, what in ((tg, nan_src, "all-NaN source"), (tg, empty, "empty source"), (empty, sr, "empty target"), (empty, empty, "both empty")):
        r, idx, d2 = _one(seg, t, s, None, None)
        assert r.status == ERR_NUMERIC and r.iterations == 0 and r.converged == 0 and r.T.tobytes() == IDENTITY_T.tobytes(), what
        assert r.score == DBL_MAX and r.used == 0 and len(idx) == len(s) and (idx == -1).all(), what
        z, _, _ = _one(seg, t, s, None, None, max_iterations=0)
        assert z.status == 0 and z.used == 0 and z.score == DBL_MAX, what


def test_two_correspondences_are_too_few(seg):
    tg, src, mc = two_correspondences()
    stg, ssr, _ = scene("small")
    T0 = skew_T(1e-4, (0, 0, 1), (1e-4, 0, 0))                                    # not the identity: T must come back as it went in
    res, nn = seg.register_pairs([tg, src, stg, ssr], [(2, 3, None, None), (0, 1, T0, mc), (2, 3, None, BOUNDED_MAX_CORR2)], max_iterations=MAX_ITERATIONS,
                                 return_nn=True)
    few = res[1]
    assert few.status == ERR_NUMERIC and few.iterations == 0 and few.converged == 0 and few.T.tobytes() == T0.tobytes()
    assert few.used == 2 and 0 < few.score <= mc                                # the final pass still reports what it found at T0
    score, used = seg.fitness_scores([tg, src], [(0, 1, T0, mc)])
    assert few.score == score[0] and used[0] == 2
    for k, mcs in ((0, None), (2, BOUNDED_MAX_CORR2)):                           # the other pairs of the call are unaffected, bitwise
        assert _same((res[k], nn[k][0], nn[k][1]), _one(seg, stg, ssr, None, mcs)), k
        assert res[k].status == 0 and res[k].converged == 1


def test_finished_pairs_stay_frozen(seg):
    ftg, fsr = fast_pair()
    ltg, lsr, _ = scene("large")
    res, nn = seg.register_pairs([ftg, fsr, ltg, lsr], [(0, 1, None, None), (2, 3, None, None)], max_iterations=MAX_ITERATIONS, return_nn=True)
    fast, slow = res
    print(f"fast pair {fast.iterations} iterations, slow pair {slow.iterations}")
    assert fast.converged == 1 and slow.converged == 1 and fast.iterations <= 4 and slow.iterations >= fast.iterations + 8
    assert _same((fast, nn[0][0], nn[0][1]), _one(seg, ftg, fsr))
    assert _same((slow, nn[1][0], nn[1][1]), _one(seg, ltg, lsr))
    assert np.abs(fast.T[9:] - [0.01, -0.005, 0.0025]).max() < 1e-6 and np.abs(fast.T[:9] - IDENTITY_T[:9]).max() < 1e-6


@pytest.mark.parametrize("name,max_corr2", CASES)
def test_converged_T_is_a_fixed_point_of_the_reference(seg, name, max_corr2):
    T = _lockstep(seg, name, max_corr2)[-1]
    tg, sr, _ = scene(name)
    ref, _ = step_ref(tg, sr, T, max_corr2)
    assert np.abs(ref - T).max() <= 1e-9


def _raw(lib, seg, xyz, start, n_clouds, pairs, n_pairs, max_iterations, epsilon, out, idx=None, d2=None, ms=None):
    return lib.sslam_seg_register_pairs(seg._h, xyz.ctypes.data, start.ctypes.data, n_clouds, C.cast(pairs, C.c_void_p), n_pairs, max_iterations,
                                        C.c_double(epsilon), C.cast(out, C.c_void_p), None if idx is None else idx.ctypes.data,
                                        None if d2 is None else d2.ctypes.data, ms)


def test_python_mirror_returns_the_c_values(gpu_lib, seg):
    from semantic_slam_amd.segmentation import RegPair, RegResult
    from semantic_slam_amd.synth import make_frame
    tg, sr, _ = scene("small")
    T0 = skew_T(0.01, (0.1, 0.2, 0.9), (0.01, 0.0, -0.01))
    xyz = np.ascontiguousarray(np.concatenate([tg, sr]))
    start = np.array([0, len(tg), len(tg) + len(sr)], np.int32)
    rec = (RegPair * 2)()
    for k, (mc, T) in enumerate(((DBL_MAX, IDENTITY_T), (BOUNDED_MAX_CORR2, T0))):
        rec[k].target, rec[k].source, rec[k].max_corr2 = 0, 1, mc
        for q in range(12):
            rec[k].T0[q] = T[q]
    out = (RegResult * 2)()
    idx, d2 = np.zeros(2 * len(sr), np.int32), np.zeros(2 * len(sr), np.float32)
    ms = C.c_double(0)
    assert _raw(gpu_lib, seg, xyz, start, 2, rec, 2, MAX_ITERATIONS, 1e-7, out, idx, d2, C.byref(ms)) == 2 and ms.value > 0
    res, nn = seg.register_pairs([tg, sr], [(0, 1, None, None), (0, 1, T0, BOUNDED_MAX_CORR2)], max_iterations=MAX_ITERATIONS, epsilon=1e-7, return_nn=True)
    for k in range(2):
        assert np.array(out[k].T[:]).tobytes() == res[k].T.tobytes()
        assert (out[k].score, out[k].used, out[k].iterations, out[k].converged, out[k].status) == \
               (res[k].score, res[k].used, res[k].iterations, res[k].converged, res[k].status)
        assert res[k].converged == 1 and res[k].iterations >= 3
        assert np.array_equal(idx[k * len(sr):(k + 1) * len(sr)], nn[k][0]) and d2[k * len(sr):(k + 1) * len(sr)].tobytes() == nn[k][1].tobytes()
    plain = seg.register_pairs([tg, sr], [(0, 1, np.eye(4), None)], max_iterations=MAX_ITERATIONS, epsilon=1e-7)   # a 4 x 4 guess, no nn arrays
    assert plain[0].T.tobytes() == res[0].T.tobytes()
    assert _raw(gpu_lib, seg, xyz, start, 2, rec, 0, 5, 0.0, out) == 0
    # the call refuses while a pipelined batch is in flight, and works again once it is collected
    seg.submit_frames([make_frame(seed=3, n_boxes=2)])
    assert _raw(gpu_lib, seg, xyz, start, 2, rec, 2, 5, 0.0, out) == -1 and b"in flight" in gpu_lib.sslam_last_error()
    seg.collect_frames()
    assert _raw(gpu_lib, seg, xyz, start, 2, rec, 2, 5, 0.0, out) == 2


# ---- the C++ shim -------------------------------------------------------------------------------------------------------------------

def _shim_clouds():
    """the clouds of tests/shim_registration_check.cpp: keep the two in step"""
    i = np.arange(300)
    tg = np.stack([np.float32(0.125) * (i % 20).astype(np.float32), np.float32(0.25) * (i // 20).astype(np.float32),
                   np.float32(0.0625) * ((i * 7) % 11).astype(np.float32)], 1).astype(np.float32)
    sr = (tg[2 * np.arange(130) + 3] + np.array([-0.03125, 0.015625, -0.0078125], np.float32)).astype(np.float32)
    sr[17, 1] = np.nan
    return tg, sr


def test_cpp_shim_scan_matcher_end_to_end(seg, tmp_path):
    from semantic_slam_amd import library_path
    tg, sr = _shim_clouds()
    r, _, _ = _one(seg, tg, sr, None, 0.2 * 0.2, max_iterations=30)              # ScanMatcher squares its distance the same way
    assert r.status == 0 and r.converged == 1 and r.used == 129
    assert np.abs(r.T[9:] - [0.03125, -0.015625, 0.0078125]).max() < 1e-6 and np.abs(r.T[:9] - IDENTITY_T[:9]).max() < 1e-6
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_registration")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_registration_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    args = [repr(float(v)) for v in r.T] + [repr(float(r.score)), str(r.converged), str(r.iterations)]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shim registration ok" in out.stdout and re.search(r"converged 1 iterations \d+ status 0", out.stdout), out.stdout
