"""Fitness-score information matrices, the parts that need no GPU: the NumPy reference of tests/fitness_ref.py pinned against an
independent nearest-neighbour search, sslam_information_from_fitness against the plain-Python restatement, and the contract of the new
entry points on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

from fitness_ref import DBL_MAX, DEFAULT_INF, information_ref, nearest_f32, skew_T, transform_f32


def test_reference_against_an_independent_search():
    """scipy's k-d tree on the float64 images of the same transformed float32 points.  The float32 d2 of the reference differs from the
    exact one by its own rounding: three subtractions, three products and two sums, each 2^-24 relative -> at most 4 * 2^-24 * d2 to first
    order, plus the issue's cancellation allowance 2 * d * 2^-24 * |p| (|p| = the largest coordinate norm in play).  The reference's
    nearest point may be another one than the tree's when two are that close: distances are compared, not indices."""
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(7)
    worst = 0.0
    for nt, ns in ((700, 333), (257, 1025), (64, 65)):
        tg = (rng.normal(size=(nt, 3)) * [3.0, 2.0, 0.5]).astype(np.float32)
        sr = (rng.normal(size=(ns, 3)) * [3.0, 2.0, 0.5]).astype(np.float32)
        T = skew_T()
        idx, d2 = nearest_f32(tg, sr, T)
        q = transform_f32(sr, T).astype(np.float64)
        dist, _ = spatial.cKDTree(tg.astype(np.float64)).query(q, k=1)
        pmax = max(np.linalg.norm(q, axis=1).max(), np.linalg.norm(tg.astype(np.float64), axis=1).max())
        bound = 4 * 2.0 ** -24 * dist ** 2 + 2 * dist * 2.0 ** -24 * pmax
        err = np.abs(d2.astype(np.float64) - dist ** 2)
        worst = max(worst, float((err / bound).max()))
        assert (idx >= 0).all() and (idx < nt).all()
        assert (err <= bound).all(), (err.max(), bound[err.argmax()])
        # the index the reference reports is the one whose distance it reports
        back = ((q - tg[idx].astype(np.float64)) ** 2).sum(1)
        assert (np.abs(back - d2) <= bound).all()
    print(f"largest error / bound: {worst:.3f}")


def test_reference_tie_rule_and_non_finite_points():
    tg = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    sr = np.array([[1, 0, 0], [0.1, 0, 0], [np.inf, 0, 0], [0, np.nan, 0]], np.float32)
    idx, d2 = nearest_f32(tg, sr, np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]))
    assert idx.tolist() == [1, 0, -1, -1] and d2[2] == -1.0 and d2[3] == -1.0 and d2[0] == 0.0


SCORES = [0.0, 1e-4, 0.05, 0.5, 5.0, DBL_MAX]


def test_information_from_fitness_equals_the_restatement(hip_lib):
    from semantic_slam_amd.segmentation import InfParams, default_inf_params, information_from_fitness
    d = default_inf_params()
    assert (d.var_gain_a, d.min_stddev_x, d.max_stddev_x, d.min_stddev_q, d.max_stddev_q, d.fitness_score_thresh) == DEFAULT_INF
    other = InfParams(7.5, 0.2, 3.0, 0.01, 0.4, 1.25)
    prev = None
    for sc in SCORES:
        got = information_from_fitness(sc)
        want = information_ref(sc)
        assert got.shape == (6, 6) and got.tobytes() == want.tobytes(), (sc, np.diag(got), np.diag(want))
        assert np.isfinite(got).all() and (np.diag(got) > 0).all()
        assert information_from_fitness(sc, other).tobytes() == information_ref(sc, (7.5, 0.2, 3.0, 0.01, 0.4, 1.25)).tobytes()
        if prev is not None:                                          # a worse score never gives more information
            assert (np.diag(got) <= np.diag(prev)).all()
        prev = got
    # no clamp: above the threshold y > 1 and the variance exceeds max_stddev^2
    assert 1.0 / information_from_fitness(5.0)[0, 0] > 5.0 ** 2 * (1 - 1e-6) and 1.0 / information_from_fitness(0.0)[0, 0] == float(np.float32(0.1 * 0.1))
    assert hip_lib.sslam_information_from_fitness(None, C.c_double(0.1), None) == -1


def _pairs(n, target=0, source=0):
    from semantic_slam_amd.segmentation import FitnessPair
    rec = (FitnessPair * max(n, 1))()
    for k in range(n):
        rec[k].target, rec[k].source, rec[k].max_range = target, source, DBL_MAX
        for q, v in enumerate(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])):
            rec[k].T[q] = v
    return rec


def test_contract_without_a_device(hip_lib):
    if hip_lib.sslam_device_count() > 0:
        pytest.skip("a GPU is visible here; the loud-failure path is for CPU-only boxes")
    from semantic_slam_amd import SslamError
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    seg = PointCloudSegmentation()
    pts = np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32)
    with pytest.raises(SslamError) as ei:
        seg.fitness_scores([pts, pts], [(0, 1, np.eye(4), None)])
    assert ei.value.code == -2 and "no CPU fallback" in str(ei.value)
    # argument errors are reported before the device is looked for
    start = np.array([0, 50], np.int32)
    score, used = np.zeros(1), np.zeros(1, np.int32)
    rc = hip_lib.sslam_seg_fitness_scores(seg._h, pts.ctypes.data, start.ctypes.data, 1, C.cast(_pairs(1, 0, 1), C.c_void_p), 1,
                                          score.ctypes.data, used.ctypes.data, None, None, None)
    assert rc == -1
    # the orchestrator: the setter needs no device, and keyframes without clouds still get constant-matrix edges
    S = SemanticGraphSLAM(default_slam_params())
    S.set_fitness_information()
    for k in range(3):
        assert S.VIOCallback((k, 0), [0.6 * k, 0, 0, 0, 0, 0, 1])
    assert S.run() and S.last_stats.keyframes_added == 3 and not S.last_stats.optimized
    assert len(S.getKeyframes()[0]) == 3 and S.num_edges() == 2
    score, used = S.last_fitness()
    assert score.tolist() == [-1.0, -1.0] and used.tolist() == [-1, -1]
    S.set_fitness_information(None)
    assert S.VIOCallback((3, 0), [1.8, 0, 0, 0, 0, 0, 1]) and S.run() and S.num_edges() == 3
    assert len(S.last_fitness()[0]) == 0


def test_setter_arguments(hip_lib):
    from semantic_slam_amd.segmentation import default_inf_params
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    S = SemanticGraphSLAM(default_slam_params())
    p = default_inf_params()
    f = hip_lib.sslam_slam_set_fitness_information
    assert f(S._h, C.byref(p), C.c_float(0.0), C.c_double(0.0)) == 0
    assert f(S._h, None, C.c_float(0.2), C.c_double(-1.0)) == 0
    assert f(None, C.byref(p), C.c_float(0.1), C.c_double(1.0)) == -1
    assert f(S._h, C.byref(p), C.c_float(-0.1), C.c_double(1.0)) == -1
    assert f(S._h, C.byref(p), C.c_float(float("nan")), C.c_double(1.0)) == -1
    assert f(S._h, C.byref(p), C.c_float(0.1), C.c_double(float("nan"))) == -1
    assert hip_lib.sslam_slam_last_fitness(None, None, None, 0) == -1
