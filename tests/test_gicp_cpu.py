"""Generalized ICP without a GPU: the NumPy reference (tests/gicp_ref.py) on its own -- what tests/test_gicp_gpu.py relies on when it
holds the device to it -- and the parts of the C-ABI and the shim that need no device.
Scenes: those of tests/registration_ref.py; `half_z` and `far_half` start from start_T(name), the others from the identity."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gicp_ref as G
from fitness_ref import DBL_MAX, IDENTITY_T
from registration_ref import FAR_SCENES, MAX_ITERATIONS, far_pose_error, icp_ref, pose_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def _run(name):
    """the reference loop on a scene, once: dict with the clouds, covariances, gaps, T, the trace of every step and ICP's fixed point"""
    if name not in _RUNS:
        tg, sr, Tt, T0 = G.load_scene(name)
        Ct, gt, _ = G.cov_ref(tg)
        Cs, gs, _ = G.cov_ref(sr)
        trace = []
        T, it, conv, st = G.gicp_ref(tg, sr, Ct, Cs, T0, None, MAX_ITERATIONS, 1e-10, trace=trace)
        Ti, iti, convi, sti = icp_ref(tg, sr, T0, None, MAX_ITERATIONS, 0.0)
        _RUNS[name] = dict(tg=tg, sr=sr, Tt=Tt, T0=T0, Ct=Ct, Cs=Cs, gt=gt, gs=gs, T=T, it=it, conv=conv, st=st, trace=trace, Ti=Ti, convi=convi)
    return _RUNS[name]


def _err(name, T, Tt):
    return far_pose_error(name, T) if name in FAR_SCENES else pose_error(T, Tt)


@pytest.mark.parametrize("name", G.SCENE_NAMES)
def test_reference_reaches_a_fixed_point(name):
    """no entry of T moves by more than 1e-10 within MAX_ITERATIONS, plain Gauss-Newton, and T stays a proper rotation"""
    r = _run(name)
    print(name, "iterations", r["it"], "last move", r["trace"][-1][3])
    assert r["st"] == 0 and r["conv"] == 1 and 3 <= r["it"] <= MAX_ITERATIONS
    assert r["trace"][-1][3] <= 1e-10
    R = r["T"][:9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12


@pytest.mark.parametrize("name", G.SCENE_NAMES)
def test_pose_error_is_no_worse_than_1_5_times_icp(name):
    """rotation and translation error at the fixed point against icp_ref's on the same scene and start.  Measured (rad, m): GICP is 2 to
    14 times nearer to the truth than ICP on the room scenes and on `floor`, and lands on ICP's fixed point to 1e-12 on `wall` (ratio 1)."""
    r = _run(name)
    assert r["convi"] == 1
    (ga, gd), (ia, idist) = _err(name, r["T"], r["Tt"]), _err(name, r["Ti"], r["Tt"])
    print(name, "gicp", ga, gd, "icp", ia, idist)
    assert ga <= 1.5 * ia and gd <= 1.5 * idist


@pytest.mark.parametrize("name", G.SCENE_NAMES)
def test_conditioning_of_every_step(name):
    """cond2(H) <= 1e5 everywhere but on far_half, whose clouds lie 30 m from the origin: there it is between 1e6 and 1e9, which is what
    exercises the relative bar of the lockstep test"""
    conds = [c for c, _, _, _ in _run(name)["trace"]]
    print(name, "cond2(H) %.3g .. %.3g" % (min(conds), max(conds)))
    if name == "far_half":
        assert all(1e6 <= c <= 1e9 for c in conds)
    else:
        assert all(c <= 1e5 for c in conds)


@pytest.mark.parametrize("name", G.SCENE_NAMES)
def test_gap_ratio_cap(name):
    """the covariance comparison on the GPU leaves out points with (l1 - l0) / l2 < 1e-2: at most 1 % of any cloud"""
    r = _run(name)
    for g in (r["gt"], r["gs"]):
        assert np.isfinite(g).all() and (g >= G.GAP_MIN).mean() >= 0.99


def test_the_method_bites():
    r = _run("small")
    assert np.abs(r["T"] - r["Ti"]).max() > 1e-6


def test_covariances_are_the_plane_regularisation():
    r = _run("small")
    for c in r["Ct"][::17]:
        lam = np.linalg.eigvalsh(G.mat6(c))
        assert np.abs(lam - [G.EPS_DEFAULT, 1.0, 1.0]).max() <= 1e-12
    # a flat cloud: the normal is the axis the cloud has no extent along
    w = _run("floor")
    assert np.abs(w["Ct"] - G.sym6(np.diag([1.0, 1.0, G.EPS_DEFAULT]))).max() <= 1e-12


def test_degenerate_inputs():
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    cov, gap, m = G.cov_ref(two)
    assert list(m) == [2, 2] and np.array_equal(cov, np.tile(G.sym6(np.eye(3)), (2, 1)))
    rng = np.random.default_rng(5)
    c19 = rng.normal(size=(19, 3)).astype(np.float32)
    knn = G.knn_ref(c19, 20)
    cov, gap, m = G.cov_ref(c19, 20)
    assert (m == 19).all() and (knn[:, 19] == -1).all() and (np.sort(knn[:, :19], 1) == np.arange(19)).all()
    assert (knn[:, 0] == np.arange(19)).all()                                   # a point is its own nearest neighbour
    assert np.abs(cov - cov[0]).max() <= 1e-9                                   # all 19 use the same 19 points: one covariance
    c19[4] = np.nan
    knn = G.knn_ref(c19, 20)
    assert (knn[4] == -1).all() and not (knn == 4).any() and ((knn >= 0).sum(1) == np.where(np.arange(19) == 4, 0, 18)).all()
    assert not G.cov_ref(c19, 20)[0][4].any()


def test_ties_go_to_the_lowest_index():
    base = np.random.default_rng(6).normal(size=(40, 3)).astype(np.float32)
    c = np.concatenate([base, base[:10]])                                        # points 40 .. 49 repeat 0 .. 9
    knn = G.knn_ref(c, 3)
    assert list(knn[45, :2]) == [5, 45] and list(knn[5, :2]) == [5, 45]


# ---- the C-ABI without a device ----------------------------------------------------------------------------------------------------------
def _cov_raw(lib, h, xyz, start, n_clouds, k, eps, cov):
    return lib.sslam_seg_cloud_covariances(h, None if xyz is None else xyz.ctypes.data, None if start is None else start.ctypes.data, n_clouds, k,
                                           C.c_double(eps), None if cov is None else cov.ctypes.data, None, None)


def test_covariance_argument_checks_come_before_the_device(hip_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    seg = PointCloudSegmentation()
    xyz = np.random.default_rng(0).normal(size=(90, 3)).astype(np.float32)
    start = np.array([0, 40, 90], np.int32)
    cov = np.zeros((90, 6))
    bad = [dict(h=None), dict(start=None), dict(n_clouds=-1), dict(xyz=None), dict(cov=None), dict(start=np.array([0, 50, 40], np.int32)),
           dict(start=np.array([-1, 40, 90], np.int32)), dict(k=2), dict(k=33), dict(k=-1), dict(eps=0.0), dict(eps=-1e-3), dict(eps=1.5),
           dict(eps=float("nan")), dict(eps=float("inf"))]
    for kw in bad:
        a = dict(h=seg._h, xyz=xyz, start=start, n_clouds=2, k=20, eps=1e-3, cov=cov)
        a.update(kw)
        assert _cov_raw(hip_lib, **a) == -1, kw
    assert not cov.any()
    for k, eps in ((3, 1e-3), (32, 1.0), (20, 1e-300)):
        assert _cov_raw(hip_lib, seg._h, xyz, start, 2, k, eps, cov) == (90 if hip_lib.sslam_device_count() > 0 else -2)


def test_gicp_argument_checks_come_before_the_device(hip_lib):
    from semantic_slam_amd.segmentation import GicpParams, PointCloudSegmentation, RegPair, RegResult
    seg = PointCloudSegmentation()
    xyz = np.random.default_rng(0).normal(size=(90, 3)).astype(np.float32)
    start = np.array([0, 40, 90], np.int32)
    out = (RegResult * 1)()

    def pair(t, s):
        p = (RegPair * 1)()
        p[0].target, p[0].source, p[0].max_corr2 = t, s, DBL_MAX
        for q in range(12):
            p[0].T0[q] = IDENTITY_T[q]
        return p

    def raw(h=seg._h, xyz=xyz, start=start, n_clouds=2, pairs=pair(0, 1), n_pairs=1, gp=None, max_iterations=5, epsilon=0.0, out=out):
        return hip_lib.sslam_seg_register_pairs_gicp(h, None if xyz is None else xyz.ctypes.data, None if start is None else start.ctypes.data, n_clouds,
                                                     None if pairs is None else C.cast(pairs, C.c_void_p), n_pairs, None,
                                                     None if gp is None else C.byref(gp), max_iterations, C.c_double(epsilon),
                                                     None if out is None else C.cast(out, C.c_void_p), None, None, None)
    bad = [dict(h=None), dict(start=None), dict(xyz=None), dict(pairs=None), dict(out=None), dict(n_pairs=-1), dict(n_clouds=-1),
           dict(pairs=pair(0, 2)), dict(pairs=pair(-1, 0)), dict(start=np.array([0, 50, 40], np.int32)), dict(max_iterations=-1), dict(epsilon=-1.0),
           dict(epsilon=float("nan")), dict(gp=GicpParams(2, 1e-3)), dict(gp=GicpParams(33, 1e-3)), dict(gp=GicpParams(20, 0.0)),
           dict(gp=GicpParams(20, 2.0)), dict(gp=GicpParams(20, float("nan")))]
    for kw in bad:
        assert raw(**kw) == -1, kw
    assert out[0].iterations == 0 and out[0].T[0] == 0.0
    assert raw() == raw(gp=GicpParams(3, 1.0)) == (1 if hip_lib.sslam_device_count() > 0 else -2)


def test_set_loop_registration_checks(hip_lib):
    from semantic_slam_amd.segmentation import GicpParams
    from semantic_slam_amd.semantic_graph_slam import REG_GICP, REG_ICP, SemanticGraphSLAM
    S = SemanticGraphSLAM()
    f = hip_lib.sslam_slam_set_loop_registration
    assert f(None, REG_ICP, None) == -1
    for method, gp in ((2, None), (-1, None), (REG_GICP, GicpParams(2, 1e-3)), (REG_GICP, GicpParams(33, 1e-3)), (REG_GICP, GicpParams(20, 0.0)),
                       (REG_GICP, GicpParams(20, 1.0001)), (REG_ICP, GicpParams(20, float("nan")))):
        assert f(S._h, method, None if gp is None else C.byref(gp)) == -1, (method, gp)
    assert f(S._h, REG_GICP, None) == 0 and f(S._h, REG_ICP, None) == 0 and f(S._h, REG_GICP, C.byref(GicpParams(3, 1.0))) == 0
    S.set_loop_registration("FAST_GICP", k=10)
    S.set_loop_registration("ICP")
    with pytest.raises(ValueError):
        S.set_loop_registration("NDT")
    assert S.loop_covariance_passes() == 0


def test_default_parameters(hip_lib):
    from semantic_slam_amd.segmentation import GicpParams
    p = GicpParams(0, 0.0)
    hip_lib.sslam_gicp_default_params(C.byref(p))
    assert (p.k, p.plane_epsilon) == (G.K_DEFAULT, G.EPS_DEFAULT)
    assert C.sizeof(GicpParams) == 16


def test_symbols_are_exported_and_declared(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "sslam.h")).read()
    for name, n_args in (("sslam_seg_cloud_covariances", 9), ("sslam_seg_register_pairs_gicp", 14), ("sslam_slam_set_loop_registration", 3),
                         ("sslam_slam_loop_covariance_passes", 2)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        fn = getattr(hip_lib, name)                                             # AttributeError if the library does not export it
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    assert "typedef struct sslam_gicp_params" in hdr and "#define SSLAM_REG_GICP 1" in hdr and "DEVIATION" in hdr


def test_cpp_shim_set_method(hip_lib, tmp_path):
    """ScanMatcher::setMethod takes hdl's three names and refuses "NDT"; the check program runs its device part only with a GPU"""
    from semantic_slam_amd import library_path
    exe = str(tmp_path / "shim_gicp")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "shim_gicp_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "names"], capture_output=True, text=True)
    assert out.returncode == 0 and "shim gicp names ok" in out.stdout, out.stdout + out.stderr
