"""Scan-matching odometry without a GPU: the boundary (symbols, struct layouts, defaults, every SSLAM_ERR_INVALID case, the refusal without
a device, the C++ shim's parameter mapping) and, on the NumPy reference alone, the conditions that keep tests/test_odometry_gpu.py
honest: the 45-frame run of odom_scene.py makes no keyframe decision near its threshold, tracks the truth, and is the run recorded in
tests/golden/odom_ref45.npz; the outlier stages remove something but not much; the rejection sequence rejects with a margin; point-to-point
ICP slides on these clouds, which is why the accuracy test is generalized ICP's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gicp_ref
import odom_ref as R
import odom_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_NO_DEVICE = -1, -2
SYMBOLS = (("int", "sslam_seg_radius_outlier_removal", 8), ("void", "sslam_prefilter_default_params", 1), ("int", "sslam_seg_prefilter", 8),
           ("void", "sslam_odom_default_params", 1), ("sslam_odom*", "sslam_odom_create", 2), ("void", "sslam_odom_destroy", 1),
           ("int", "sslam_odom_reset", 1), ("int", "sslam_odom_push", 7), ("int", "sslam_odom_keyframe", 4))


def test_symbols_are_exported_and_declared(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "sslam.h")).read()
    for ret, name, n_args in SYMBOLS:
        assert re.search(re.escape(ret) + r"\s+" + name + r"\s*\(", hdr), name
        fn = getattr(hip_lib, name)                                             # AttributeError if the library does not export it
        assert len(fn.argtypes) == n_args, name
    for text in ("typedef struct sslam_prefilter_params", "typedef struct sslam_odom_params", "typedef struct sslam_odom_stats",
                 "#define SSLAM_OUTLIER_RADIUS 2", "#define SSLAM_DOWNSAMPLE_VOXELGRID 1", "HALF the rotation angle", "[UPSTREAM, quoted from memory]"):
        assert text in hdr, text
    assert "#define SSLAM_REG_ICP 0" in hdr and "#define SSLAM_REG_GICP 1" in hdr          # the pinned values of the loop scan matcher


def test_struct_sizes_and_defaults(hip_lib):
    from semantic_slam_amd.odometry import OdomParams, OdomStats, PrefilterParams
    assert (C.sizeof(PrefilterParams), C.sizeof(OdomParams), C.sizeof(OdomStats)) == (64, 160, 208)
    assert (PrefilterParams.distance_near.offset, PrefilterParams.leaf.offset, PrefilterParams.min_neighbors.offset) == (8, 28, 56)
    assert (OdomParams.method.offset, OdomParams.gicp.offset, OdomParams.epsilon.offset, OdomParams.max_acceptable_angle.offset) == (64, 72, 96, 152)
    assert (OdomStats.covariance_passes.offset, OdomStats.T.offset, OdomStats.total_ms.offset) == (40, 56, 200)
    # the C side writes exactly the struct: the guard bytes behind it stay
    for name, size in (("sslam_prefilter_default_params", 64), ("sslam_odom_default_params", 160)):
        buf = (C.c_ubyte * (size + 16))(*([0xAB] * (size + 16)))
        getattr(hip_lib, name)(C.addressof(buf))
        assert bytes(buf[size:]) == b"\xab" * 16, name
        getattr(hip_lib, name)(None)                                            # a NULL pointer is ignored
    p = OdomParams()
    hip_lib.sslam_odom_default_params(C.byref(p))
    f = p.prefilter
    got = dict(use_distance_filter=f.use_distance_filter, distance_near=f.distance_near, distance_far=f.distance_far, downsample=f.downsample,
               leaf=f.leaf, outlier=f.outlier, mean_k=f.mean_k, stddev_mul=f.stddev_mul, radius=f.radius, min_neighbors=f.min_neighbors)
    want = dict(R.PREFILTER_DEFAULTS); want["leaf"] = float(np.float32(0.1))
    assert got == want
    got = {k: getattr(p, k) for k in R.ODOM_DEFAULTS if k not in ("k", "plane_epsilon")}
    got.update(k=p.gicp.k, plane_epsilon=p.gicp.plane_epsilon)
    assert got == R.ODOM_DEFAULTS
    assert p.method == R.REG_GICP == 1                                           # hdl's default is FAST_GICP


def _raises_invalid(fn):
    from semantic_slam_amd.graph_slam import SslamError
    with pytest.raises(SslamError) as e:
        fn()
    assert e.value.code == ERR_INVALID, e.value


def test_invalid_arguments_are_refused_before_any_device_call(hip_lib):
    """every SSLAM_ERR_INVALID case of the three entry points comes back as such with or without a device; a valid call without one is
    SSLAM_ERR_NO_DEVICE; create succeeds without a device and push fails"""
    from semantic_slam_amd.odometry import OdomStats, ScanMatchingOdometry, default_odom_params, default_prefilter_params, prefilter_params
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    seg = PointCloudSegmentation()
    pts = np.ascontiguousarray(S.frames()[1][0][:200])
    keep = np.zeros(200, np.int32)
    nan, inf = float("nan"), float("inf")
    no_gpu = hip_lib.sslam_device_count() < 1

    def radius(h=seg._h, xyz=pts, n=200, radius=0.8, min_neighbors=2, out=keep, max_out=200):
        return hip_lib.sslam_seg_radius_outlier_removal(h, None if xyz is None else xyz.ctypes.data, n, radius, min_neighbors,
                                                        None if out is None else out.ctypes.data, max_out, None)
    for kw in (dict(h=None), dict(xyz=None), dict(n=-1), dict(out=None), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf),
               dict(min_neighbors=-1)):
        assert radius(**kw) == ERR_INVALID, kw

    out = np.zeros((200, 3), np.float32)

    def prefilter(h=seg._h, xyz=pts, n=200, p=default_prefilter_params(), out=out, max_out=200):
        return hip_lib.sslam_seg_prefilter(h, None if xyz is None else xyz.ctypes.data, n, None if p is None else C.addressof(p),
                                           None if out is None else out.ctypes.data, max_out, None, None)
    bad_filters = [dict(distance_near=nan), dict(distance_far=nan), dict(downsample=2), dict(downsample=-1), dict(leaf=0.0), dict(leaf=-0.1), dict(leaf=nan),
                   dict(leaf=inf), dict(outlier=3), dict(outlier=-1), dict(mean_k=0), dict(mean_k=64), dict(stddev_mul=nan),
                   dict(outlier=R.OUTLIER_RADIUS, radius=0.0), dict(outlier=R.OUTLIER_RADIUS, radius=nan), dict(outlier=R.OUTLIER_RADIUS, radius=inf),
                   dict(outlier=R.OUTLIER_RADIUS, min_neighbors=-1)]
    for kw in (dict(h=None), dict(xyz=None), dict(n=-1), dict(p=None), dict(out=None), dict(max_out=-1)):
        assert prefilter(**kw) == ERR_INVALID, kw
    for kw in bad_filters:
        assert prefilter(p=prefilter_params(**kw)) == ERR_INVALID, kw
    # parameters of a stage that is off are not read
    ok = [prefilter_params(use_distance_filter=0, distance_near=nan), prefilter_params(downsample=0, leaf=0.0),
          prefilter_params(outlier=R.OUTLIER_RADIUS, mean_k=0), prefilter_params(outlier=0, radius=-1.0, mean_k=99)]

    # the odometry: create refuses bad parameters (NULL, the reason in sslam_last_error), push refuses bad arguments
    bad_odom = bad_filters + [dict(method=2), dict(method=-1), dict(k=2), dict(k=33), dict(plane_epsilon=0.0), dict(plane_epsilon=1.5),
                              dict(plane_epsilon=nan), dict(max_iterations=-1)]
    for name in ("epsilon", "max_correspondence_distance", "keyframe_delta_trans", "keyframe_delta_angle", "keyframe_delta_time",
                 "max_acceptable_trans", "max_acceptable_angle"):
        bad_odom += [{name: -1e-9}, {name: nan}, {name: inf}]
    for kw in bad_odom:
        _raises_invalid(lambda: ScanMatchingOdometry(seg, **kw))
    assert not hip_lib.sslam_odom_create(None, None)
    assert b"bad argument" in hip_lib.sslam_last_error()
    h = hip_lib.sslam_odom_create(seg._h, None)                                  # NULL params: the defaults
    assert h
    hip_lib.sslam_odom_destroy(h)
    hip_lib.sslam_odom_destroy(None)
    od = ScanMatchingOdometry(seg, method="ICP", k=2)                              # ICP does not read the generalized-ICP parameters
    pose = np.full(12, 7.0)
    st = OdomStats()

    def push(h=od._h, xyz=pts, n=200, pose=pose):
        return hip_lib.sslam_odom_push(h, None if xyz is None else xyz.ctypes.data, n, 0, 0, None if pose is None else pose.ctypes.data, C.addressof(st))
    for kw in (dict(h=None), dict(xyz=None), dict(n=-1), dict(pose=None)):
        assert push(**kw) == ERR_INVALID, kw
    assert (pose == 7.0).all() and st.n_raw == 0
    assert hip_lib.sslam_odom_reset(None) == ERR_INVALID and hip_lib.sslam_odom_reset(od._h) == 0
    assert hip_lib.sslam_odom_keyframe(None, None, 0, None) == ERR_INVALID
    assert hip_lib.sslam_odom_keyframe(od._h, None, 5, None) == ERR_INVALID and hip_lib.sslam_odom_keyframe(od._h, None, -1, None) == ERR_INVALID
    assert hip_lib.sslam_odom_keyframe(od._h, None, 0, None) == 0                  # no keyframe yet
    cloud, kf_pose = od.keyframe()
    assert len(cloud) == 0 and kf_pose is None
    if no_gpu:
        assert radius() == ERR_NO_DEVICE and prefilter() == ERR_NO_DEVICE and push() == ERR_NO_DEVICE
        assert all(prefilter(p=p) == ERR_NO_DEVICE for p in ok)
        assert hip_lib.sslam_odom_keyframe(od._h, None, 0, None) == 0            # the failed push left the handle without a keyframe
    else:
        assert radius() >= 0 and prefilter() >= 0 and all(prefilter(p=p) >= 0 for p in ok)
    assert default_odom_params().max_iterations == 64


def test_loop_scan_matcher_surface_is_unchanged(hip_lib):
    from semantic_slam_amd.semantic_graph_slam import REG_GICP, REG_ICP, SemanticGraphSLAM
    assert (REG_ICP, REG_GICP) == (0, 1)
    assert hip_lib.sslam_slam_set_loop_registration(SemanticGraphSLAM()._h, 2, None) == ERR_INVALID


def test_cpp_shim_parameters_and_refusal(hip_lib, tmp_path):
    """hdl's parameter names map onto the C defaults, unknown method names throw, the structs have the sizes the mirror assumes; without a
    GPU matching() throws"""
    from semantic_slam_amd import library_path
    exe = str(tmp_path / "shim_odometry")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "shim_odometry_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "params"], capture_output=True, text=True)
    assert out.returncode == 0 and "shim odometry params ok" in out.stdout, out.stdout + out.stderr
    if hip_lib.sslam_device_count() < 1:
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and "no GPU: params and the refusal only" in out.stdout, out.stdout + out.stderr


# ---- the reference alone ------------------------------------------------------------------------------------------------------------------
def test_products_and_angle():
    rng = np.random.default_rng(5)
    for _ in range(20):
        A = np.concatenate([gicp_ref.exp_so3(rng.normal(size=3)).reshape(-1), rng.normal(size=3)])
        B = np.concatenate([gicp_ref.exp_so3(rng.normal(size=3)).reshape(-1), rng.normal(size=3)])
        Ra, Rb = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
        assert np.abs(R.mul(A, B) - np.concatenate([(Ra @ Rb).reshape(-1), Ra @ B[9:] + A[9:]])).max() < 1e-14
        assert np.abs(R.mul(A, R.inverse(A)) - gicp_ref.IDENTITY_T).max() < 1e-14
        full = np.arccos(np.clip((np.trace(Ra) - 1) / 2, -1, 1))
        assert abs(R.angle(A) - min(full, 2 * np.pi - full) / 2) < 1e-9            # HALF the rotation angle
    assert R.angle(gicp_ref.IDENTITY_T) == 0.0 and R.trans(gicp_ref.IDENTITY_T) == 0.0
    assert R.delta_time((3, 100000000), (1, 900000000)) == 2.0 + 1e-9 * -800000000.0 and abs(R.delta_time((3, 100000000), (1, 900000000)) - 1.2) < 1e-12


def test_cloud_at_a_time_gicp_is_gicp_ref():
    """odom_ref's generalized ICP evaluates gicp_ref's statements for all points at once: the same neighbours, covariances and step"""
    _, cl = S.frames()
    a, b = (R.prefilter(c, use_distance_filter=0, leaf=0.4, outlier=0)[0] for c in (cl[0], cl[1]))
    assert 150 < len(a) < 600
    Ca, Cb = R.covariances(a), R.covariances(b)
    ref_a, gap, m = gicp_ref.cov_ref(a)
    assert (m == 20).all() and (gicp_ref.knn_ref(a, 20) == R.knn(a, 20)).all()
    sure = gap > gicp_ref.GAP_MIN
    assert sure.sum() > 0.8 * len(a) and np.abs(Ca[sure] - ref_a[sure]).max() < 1e-6
    ref_b = gicp_ref.cov_ref(b)[0]
    T_ref, n_ref, _, _ = gicp_ref.gicp_step_ref(a, b, ref_a, ref_b, gicp_ref.IDENTITY_T, 2.5 ** 2)
    T, n = R.gicp_step(a, b, ref_a, ref_b, gicp_ref.IDENTITY_T, 2.5 ** 2)
    assert n == n_ref and np.abs(T - T_ref).max() < 1e-10


@pytest.fixture(scope="module")
def run45():
    _, cl = S.frames()
    return R.reference_run(cl, [S.stamp(k) for k in range(len(cl))])


def test_reference_run_makes_no_decision_near_a_threshold_and_tracks_the_truth(run45):
    """condition (a): the GPU test may demand equal keyframe flags only if no decision of the reference is a near thing.  Largest pose error
    here: 0.0113 m and 0.0069 rad (0.0111 / 0.0068 with gicp_ref's own loops, which stop some matches an iteration apart)."""
    tr, _ = S.frames()
    P = R.ODOM_DEFAULTS
    thr = np.array([P["keyframe_delta_trans"], P["keyframe_delta_angle"], P["keyframe_delta_time"]])
    assert (run45["status"] == 0).all() and (run45["accepted"] == 1).all()
    assert run45["new_keyframe"].sum() == 15 and (np.nonzero(run45["new_keyframe"])[0] == np.arange(0, 45, 3)).all()
    assert run45["iterations"][1:].min() >= 3 and run45["iterations"].max() <= 6 < P["max_iterations"]
    for k in range(1, S.N_FRAMES):
        d = np.array([run45["delta_trans"][k], run45["delta_angle"][k], run45["delta_time"][k]])
        if run45["new_keyframe"][k]:
            assert (d > thr).any() and not ((d > thr) & (d < thr + 1e-3)).any() and (d - thr).max() > 1e-3, (k, d)
        else:
            assert (d < thr - 1e-3).all(), (k, d)
    err = np.array([S.pose_error(run45["pose"][k], S.truth_T(tr, k)) for k in range(S.N_FRAMES)])
    print("largest pose error of the reference: %.4f m, %.4f rad" % (err[:, 0].max(), err[:, 1].max()))
    assert err[:, 0].max() < 0.02 and err[:, 1].max() < 0.012
    assert abs(err[:, 0].max() - 0.0111) < 0.05 * 0.0111 and abs(err[:, 1].max() - 0.0068) < 0.05 * 0.0068


def test_recorded_run_is_the_reference_run(run45):
    """tests/golden/odom_ref45.npz is what the GPU test compares with (python tests/odom_ref.py records it): the flags exactly, the poses to
    what another LAPACK may move them"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", R.GOLDEN))
    for k in ("new_keyframe", "accepted", "status"):
        assert (gold[k] == run45[k]).all(), k
    assert np.abs(gold["pose"] - run45["pose"]).max() < 1e-6 and np.abs(gold["T"] - run45["T"]).max() < 1e-6


def test_outlier_stages_remove_some_points_but_few():
    """condition (b), on the frames the GPU tests filter: each outlier stage removes at least one point and fewer than 20 %"""
    _, cl = S.frames()
    for cloud in [S.holed_frame(0)] + [cl[k] for k in range(1, 8)]:
        for kw in (dict(outlier=R.OUTLIER_STATISTICAL), dict(outlier=R.OUTLIER_RADIUS, **R.RADIUS_KW)):
            _, counts = R.prefilter(cloud, **kw)
            assert counts[0] <= len(cloud) and counts[1] < counts[0]
            assert 1 <= counts[1] - counts[2] < 0.2 * counts[1], (kw, counts)


def test_rejection_sequence_rejects_with_a_margin():
    """condition (c): frames 0, 1, 2, 12, 3, 4 under max_acceptable_trans = 0.3"""
    _, cl = S.frames()
    o = R.Odometry(prefilter_kw=R.RUN_PREFILTER, transform_thresholding=1, max_acceptable_trans=0.3, **R.RUN_KW)
    recs = [o.push(cl[k], S.stamp(k))[1] for k in (0, 1, 2, 12, 3, 4)]
    assert [r["accepted"] for r in recs] == [1, 1, 1, 0, 1, 1] and all(r["status"] == 0 for r in recs)
    assert recs[3]["thresholding"][0] > 0.35 and recs[3]["thresholding"][1] < 1.0 - 0.05
    for r in recs[1:3] + recs[4:]:
        assert r["thresholding"][0] < 0.25 and r["thresholding"][1] < 0.95


def test_point_to_point_icp_leaves_the_truth():
    """condition (d): on the first 8 frames the point-to-point matcher slides on the ray-cast samples (DESIGN, the GICP section), by 0.4 m --
    so the accuracy test is generalized ICP's and ICP is tested for parity with the device primitives only"""
    tr, cl = S.frames()
    run = R.reference_run(cl[:8], [S.stamp(k) for k in range(8)], method=R.REG_ICP)
    err = max(S.pose_error(run["pose"][k], S.truth_T(tr, k))[0] for k in range(8))
    assert (run["status"] == 0).all() and err > 0.1
