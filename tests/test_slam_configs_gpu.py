"""GPU parity of the orchestrator tick and of data association away from the constructor defaults: the three configurations the
reference ships, every parameter alone off its default, a tilted robot, a slow one, Mahalanobis distances on the
covariances a real graph produces, detections exactly on a threshold, the first landmark of ~add_first_lan, and the handle after a
failed tick.  The inputs come from tests/slam_configs.py; tests/test_slam_configs_cpu.py asserts on the oracle alone that each of
them reaches the branch it is made for.

Bars: those of tests/test_slam_gpu.py for the replays (decisions and ids exact, estimates 1e-6, covariances 1e-4 relative, chi2 1e-6
relative).  Distances on real covariances: |d - d64| <= 8 eps32 cond(S + qI) d64 against a float64 solve on the float32 inputs -- the
float32 restatement of the oracle is within 2 of these units (0.89 measured), the factor 8 leaves room for fused multiply-adds and
the device's order of operations; 0.89 was measured on an MI355X."""
import time

import numpy as np
import pytest

from oracle import np_slam as S
from semantic_slam_amd.synth import make_replay
from tests import slam_configs as K
from tests.slam_replay import feed, oracle_instance, planes_of, product_instance
from tests.test_slam_gpu import _compare_state, _run_both

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(autouse=True)
def _print_seconds(request):
    t0 = time.perf_counter()
    yield
    print(f"{request.node.name}: {time.perf_counter() - t0:.2f} s")


def _map_is_true(P, lms):
    tr = np.array([p for p, _, _ in lms])
    for l in P.getMappedLandmarks():
        assert np.linalg.norm(tr - P.graph_vertex(l.vertex), axis=1).min() < 0.25


# ---- a. replay parity, tick by tick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", [("bucket_detector", 0), ("bucket_detector", 1), ("bucket_detector_workspace", 0), ("yolo_detector", 0)])
def test_shipped_configuration_matches_oracle_tick_by_tick(gpu_lib, name, seed):
    kw = dict(K.SHIPPED[name], **(K.BUCKET_FIRST_LAN if name == "bucket_detector" else {}))
    events, lms = K.events_for(kw, seed=seed, n_samples=300, detect_every=3)
    P, Or, ticks = _run_both(events, **kw)
    assert ticks > 20 and len(Or.assoc.landmarks) >= 8
    if "add_first_lan" not in kw:      # the known bucket is no landmark of the synthetic world
        _map_is_true(P, lms)
    else:
        tr = np.array([p for p, _, _ in lms])
        for l in P.getMappedLandmarks()[1:]:
            assert np.linalg.norm(tr - P.graph_vertex(l.vertex), axis=1).min() < 0.25


@pytest.mark.parametrize("name", list(K.SINGLES))
def test_single_parameter_matches_oracle_tick_by_tick(gpu_lib, name):
    kw = K.SINGLES[name]
    events, lms = K.single_events(name)
    iters = []
    P, Or, ticks = _run_both(events, on_tick=lambda p, o: iters.append((p.last_stats.opt.iterations, o.last_stats["opt"].iterations))
                             if o.last_stats["optimized"] else None, **kw)
    assert ticks >= 8 and len(Or.assoc.landmarks) >= 3
    if "camera_angle_deg" in kw:
        _map_is_true(P, lms)
    if "max_iterations" in kw:         # graph_slam.cpp:205: the cap counts LM iterations, as g2o's optimize(n) does
        print("iterations (product, oracle) per tick:", iters)
        assert iters and all(a == b <= kw["max_iterations"] for a, b in iters) and max(b for _, b in iters) == kw["max_iterations"]


def test_slow_replay_matches_oracle_tick_by_tick(gpu_lib):
    events, _ = K.slow_replay()
    P, Or, ticks = _run_both(events)
    assert ticks >= 20 and len(Or.keyframes) >= 25


@pytest.mark.parametrize("kw", [{}, dict(use_rtab_map_odom=1, camera_angle_deg=33.93)], ids=["level_camera", "rtab_offset_pitched_camera"])
def test_tilted_world_matches_oracle_tick_by_tick(gpu_lib, kw):
    events, _ = K.events_for(kw, n_samples=220)
    P, Or, ticks = _run_both(K.tilt_world(events), **kw)
    rpy = np.array([S.matrix2vector(k["robot_pose"])[3:] for k in Or.keyframes])
    assert ticks >= 10 and np.abs(rpy[:, 0]).max() >= 0.3 and np.abs(rpy[:, 1]).max() >= 0.3


# ---- b. mahalanobis3 on real covariances -------------------------------------------------------------------------------------------
def test_mahalanobis_on_the_covariances_of_a_real_graph(gpu_lib):
    """k_associate / mahalanobis3 on the product's own table after anisotropic_run (condition numbers up to 1e3, every row-swap pattern of
    the 3 x 3 partial-pivot LU): decisions equal to the float64 replay and to the oracle, distances within the bar of the module
    docstring of the float64 value -- never of the oracle's float32 one"""
    P = product_instance(**K.ANISO_KW)
    assert K.anisotropic_run(P, True) == 4 and P.last_stats.optimized and P.last_stats.marginals_ok
    table = K.product_table(P)
    assert len(table[0]) >= 30
    frames, expect, dropped = K.make_probes(table)
    assert dropped <= 0.05 and len(expect) >= 1500
    D = K.seeded_association(table)
    k, worst = 0, 0.0
    for objs in frames:
        got = P.find_matches(planes_of(objs), K.PROBE_POSE)
        ref = D.find_matches(objs, K.PROBE_POSE, F(0.0), lambda l: l["pose"])
        for g, r in zip(got, ref):
            new, lid, d64, cond = expect[k]
            k += 1
            assert (g.is_new, g.id) == (new, lid) == (int(r["is_new"]), r["id"])
            assert np.array_equal(np.array(g.pose[:]), r["pose"])
            ratio = abs(float(g.distance) - d64) / (K.EPS32 * cond * d64)
            worst = max(worst, ratio)
            assert ratio <= K.PROBE_FACTOR, (k, g.distance, d64, cond)
    assert k == len(expect) and len(P.getMappedLandmarks()) == len(D.landmarks)
    print("mahalanobis3 against float64, worst |d - d64| / (eps32 cond d64):", worst)


def test_tick_after_the_association_hook_keeps_the_covariances(gpu_lib):
    """sslam_slam_find_matches appends landmarks without graph vertices; a tick after it optimises, finds no marginal for them and leaves
    every covariance as it was: marginals_ok == 0, no error (include/sslam.h, next to the hook)"""
    P = product_instance(**K.ANISO_KW)
    K.anisotropic_run(P, True)
    before = [np.array(l.covariance[:]) for l in P.getMappedLandmarks()]
    far = dict(pose=np.array([0, 0, 200], F), normal=np.array([0, 0, 1, 0], F), class_id=5, plane_type=0)
    got = P.find_matches(planes_of([far]), K.PROBE_POSE)
    assert (got[0].is_new, got[0].id, got[0].vertex) == (1, len(before), -1)
    assert P.VIOCallback((28, 0), np.array([14, 4.2, 1.4, 0, 0, np.sin(1.75), np.cos(1.75)])) and P.run()
    st = P.last_stats
    assert (st.keyframes_added, st.landmark_edges_added, st.optimized, st.marginals_ok) == (1, 0, 1, 0)
    after = P.getMappedLandmarks()
    assert len(after) == len(before) + 1 and after[-1].vertex == -1
    for l, c in zip(after, before):
        assert np.array_equal(np.array(l.covariance[:]), c)


# ---- c. exact thresholds -----------------------------------------------------------------------------------------------------------
def test_detections_exactly_on_the_threshold_match_and_one_step_past_it_do_not(gpu_lib):
    for kw, frames, expect in K.threshold_frames():
        P = product_instance(**kw)
        got = [P.find_matches(planes_of(objs), pose)[0] for pose, objs in frames]
        assert (got[0].is_new, got[0].id) == (1, 0) and np.array_equal(np.array(got[0].pose[:]), K.C_THRES)
        for g, (new, lid, dist) in zip(got[1:], expect):
            assert (g.is_new, g.id) == (new, lid)
            if dist is not None:
                assert g.distance == F(dist)                 # bit-equal: every operand and every result is exact in float32
        assert got[2].distance > F(expect[0][2])


# ---- d. first landmark -------------------------------------------------------------------------------------------------------------
def test_first_landmark_right_after_create(gpu_lib):
    """addFirstPoseAndLandmark (semantic_graph_slam.cpp:289-329), addFirstLandmark (data_association.h:70-73)"""
    kw = dict(K.SHIPPED["bucket_detector"], **K.BUCKET_FIRST_LAN)
    lan = np.array(K.BUCKET_FIRST_LAN["first_lan"])

    def fresh():
        P = product_instance(**kw)
        ids, est = P.getKeyframes()
        assert list(ids) == [0] and np.array_equal(est[0], [0, 0, 0, 0, 0, 0, 1])
        lm = P.getMappedLandmarks()
        assert len(lm) == 1
        l = lm[0]
        assert (l.id, l.vertex, l.class_id, l.plane_type) == (0, 1, K.CLASS_BUCKET, 1)
        assert np.array_equal(np.array(l.covariance[:]).reshape(3, 3), np.diag([F(0.1)] * 3))
        assert np.array_equal(np.array(l.normal[:]), np.array([-0.4, 0.86, 0, 0], F))
        assert np.array_equal(np.array(l.pose[:]), lan.astype(F)) and np.array_equal(P.graph_vertex(1), lan.astype(F).astype(float))
        assert P.num_edges() == 1 and gpu_lib.sslam_graph_num_vertices(gpu_lib.sslam_slam_graph(P._h)) == 2
        Or = oracle_instance(**kw)
        _compare_state(P, Or)
        return P
    # seen from the identity through the camera pitched by 33.93 degrees: a detection 10 cm from first_lan, inside eq_dist_thres = 1.5
    Tw = S.transform_normals_to_world(np.zeros(6, F), F(kw["camera_angle_deg"] * np.pi / 180))[:3, :3].astype(float)
    pc = (np.linalg.inv(Tw) @ (lan + [0.1, 0, 0])).astype(F)
    det = lambda cls, pt: [dict(pose=pc, normal=np.array([0, 0, 1, 0], F), class_id=cls, plane_type=pt)]
    # first_object is already cleared: the very first detection is associated, not blindly mapped
    g = fresh().find_matches(planes_of(det(K.CLASS_BUCKET, 1)), np.zeros(6, F))[0]
    assert (g.is_new, g.id, g.vertex) == (0, 0, 1) and abs(g.distance - 0.1) < 1e-5
    g = fresh().find_matches(planes_of(det(1, 1)), np.zeros(6, F))[0]
    assert (g.is_new, g.id, g.vertex) == (1, 1, -1) and g.distance == -1.0


# ---- e. a failed tick leaves a usable handle ---------------------------------------------------------------------------------------
def test_failed_tick_leaves_a_usable_handle(gpu_lib):
    """A keyframe with boxes and a cloud on a handle without a frontend: run() fails with SSLAM_ERR_INVALID after the keyframe reached
    the graph.  The keyframe stays, once; its objects are lost; nothing is optimised in that tick; the next ticks associate against a
    table uploaded again and agree with an oracle in which that tick did exactly this much."""
    from semantic_slam_amd.graph_slam import SslamError
    from semantic_slam_amd.synth import make_frame
    events, _ = make_replay(0, n_samples=220)
    dry, bad = oracle_instance(), None
    for k, ev in enumerate(events):
        kf, _ = feed(dry, ev, False)
        if bad is None and k >= 160 and kf and ev.objects:
            bad = k
    assert bad is not None
    fr = make_frame(seed=20, n_boxes=4)
    P, Or = product_instance(), oracle_instance()
    ticks_after = matched_after = 0
    for k, ev in enumerate(events):
        if k == bad:
            P.setPointCloudData(fr); P.setDetectedObjectInfo(fr.boxes)
            Or.set_segmented_objects([])
            assert P.VIOCallback(ev.stamp, ev.odom) and Or.vio(ev.stamp[0], ev.stamp[1], ev.odom)
            edges = P.num_edges()
            with pytest.raises(SslamError) as err:
                P.run()
            assert err.value.code == -1 and "frontend" in str(err.value)
            assert len(Or.queue) == 1 and Or._empty_keyframe_queue()       # the oracle's side of that tick: the keyframe and its odometry edge
            Or.keyframes += Or.new_keyframes
            Or.new_keyframes = []
            assert P.num_edges() == edges + 1 == len(Or.etype)
            _compare_state(P, Or)
            continue
        kp, rp = feed(P, ev, True)
        ko, ro = feed(Or, ev, False)
        assert kp == ko and rp == ro
        if not rp:
            continue
        st, so = P.last_stats, Or.last_stats
        assert (st.keyframes_added, st.landmarks_added, st.landmarks_matched, st.landmark_edges_added, bool(st.optimized), bool(st.marginals_ok)) == \
               (so["keyframes_added"], so["landmarks_added"], so["landmarks_matched"], so["landmark_edges_added"], so["optimized"], so["marginals_ok"])
        if so["optimized"]:
            assert abs(st.opt.chi2_after - so["opt"].chi2_after) <= 1e-6 * max(1.0, so["opt"].chi2_after)
        _compare_state(P, Or)
        if k > bad:
            ticks_after += 1
            matched_after += st.landmarks_matched
    ids, _ = P.getKeyframes()
    assert len(set(ids)) == len(ids) == len(Or.keyframes) and P.num_edges() == len(Or.etype)
    assert ticks_after >= 5 and matched_after >= 5
