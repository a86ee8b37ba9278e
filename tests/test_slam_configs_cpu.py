"""The tick and the association at the configurations the reference ships and one parameter at a time off its default, on the
oracle alone: oracle/np_slam.py against oracle/oracle_slam.c at the bars of test_oracle_slam.py, and the conditions that keep
tests/test_slam_configs_gpu.py honest -- every input there must reach the branch it is made for, which is asserted here on the
oracle, where no product code runs."""
import functools
import math

import numpy as np
import pytest

from oracle import np_slam as S
from oracle.oracle import SlamTickC
from semantic_slam_amd.synth import make_replay
from tests import slam_configs as K
from tests.slam_replay import ODOM_STDDEV_X, ODOM_STDDEV_Q, oracle_instance

F = np.float32


def _cross_check(events, kw):
    """np_slam and the C driver through the same events, compared tick by tick (the bars of test_c_tick_driver_equals_the_numpy_tick);
    -> (the np_slam instance, ticks)"""
    o = oracle_instance(**kw)
    c = SlamTickC(**dict(dict(const_stddev_x=ODOM_STDDEV_X, const_stddev_q=ODOM_STDDEV_Q), **kw))
    ticks = 0
    for ev in events:
        if ev.objects is not None:
            o.set_segmented_objects(ev.objects); c.set_segmented_objects(ev.objects)
        assert o.vio(ev.stamp[0], ev.stamp[1], ev.odom) == c.vio(ev.stamp[0], ev.stamp[1], ev.odom)
        if not ev.run_after:
            continue
        ran = o.run()
        assert c.run() == ran
        if not ran:
            continue
        ticks += 1
        so, sc = o.last_stats, c.last_stats
        assert (so["keyframes_added"], so["landmarks_added"], so["landmarks_matched"], so["landmark_edges_added"]) == \
               (sc.keyframes_added, sc.landmarks_added, sc.landmarks_matched, sc.landmark_edges_added)
        g = c.graph()
        assert list(g["vtype"]) == list(o.vtype) and list(g["etype"]) == list(o.etype)
        assert list(g["evi"]) == list(o.evi) and list(g["evj"]) == list(o.evj)
        if o.etype:      # a first tick of one keyframe adds no edge
            assert np.abs(g["meas"] - np.array(o.meas)).max() <= 1e-12 and np.abs(g["info"] - np.array(o.info)).max() <= 1e-9 * np.abs(g["info"]).max()
        if so["optimized"]:
            assert sc.optimized and abs(sc.chi2_after - so["opt"].chi2_after) <= 1e-7 * max(1.0, so["opt"].chi2_after)
            assert bool(sc.marginals_ok) == so["marginals_ok"]
            if "max_iterations" in kw:              # a cap that binds is reached on both sides; free-running LM may end a step apart
                assert sc.iterations <= kw["max_iterations"] and so["opt"].iterations <= kw["max_iterations"]
            assert np.abs(g["est"] - np.array(o.est)).max() <= 1e-7
            lm = c.landmarks()
            assert list(lm["vertex"]) == [l["vertex"] for l in o.assoc.landmarks]
            cov = np.array([l["covariance"] for l in o.assoc.landmarks]).reshape(-1, 3, 3)
            assert len(cov) == 0 or np.abs(lm["covariance"] - cov).max() <= 1e-5 * np.abs(cov).max()
            assert np.abs(c.robot_pose() - o.robot_pose).max() <= 1e-7
    assert c.counts()[2] == len(o.keyframes) and c.counts()[3] == len(o.assoc.landmarks)
    return o, ticks


def _signature(o):
    """what a parameter has to move to count as read: keyframe ids, landmarks, the bits of their poses, the last chi2"""
    return ([k["node"] for k in o.keyframes], len(o.assoc.landmarks), b"".join(l["pose"].tobytes() for l in o.assoc.landmarks),
            o.last_stats["opt"].chi2_after if o.last_stats["optimized"] else None)


def _map_error(o, lms):
    tr = np.array([p for p, _, _ in lms])
    return max(np.linalg.norm(tr - o.est[l["vertex"]][:3], axis=1).min() for l in o.assoc.landmarks)


def _plain_run(events):
    """the default configuration on the events of a SINGLES entry"""
    o = oracle_instance()
    for ev in events:
        if ev.objects is not None:
            o.set_segmented_objects(ev.objects)
        o.vio(ev.stamp[0], ev.stamp[1], ev.odom)
        if ev.run_after:
            o.run()
    return _signature(o)


@pytest.mark.parametrize("first_lan", [0, 1])
@pytest.mark.parametrize("name", list(K.SHIPPED))
def test_shipped_configurations_on_both_cpu_drivers(name, first_lan):
    kw = dict(K.SHIPPED[name], **(K.BUCKET_FIRST_LAN if first_lan else {}))
    events, lms = K.events_for(kw, n_samples=300, detect_every=3)
    o, ticks = _cross_check(events, kw)
    assert ticks > 20 and len(o.assoc.landmarks) >= 8
    if first_lan:       # the known landmark hangs on the identity keyframe, and the first real keyframe on that one
        l0 = o.assoc.landmarks[0]
        assert (l0["vertex"], l0["class_id"], l0["plane_type"]) == (1, K.CLASS_BUCKET, 1) and o.keyframes[0]["node"] == 0
        assert (o.etype[0], o.evi[0], o.evj[0]) == (S.O.ET_SE3_POINT, 0, 1) and (o.etype[1], o.evi[1], o.evj[1]) == (S.O.ET_SE3, 0, 2)


@pytest.mark.parametrize("name", list(K.SINGLES))
def test_single_parameters_on_both_cpu_drivers_and_each_one_is_read(name):
    kw = K.SINGLES[name]
    events, _ = K.single_events(name)
    o, ticks = _cross_check(events, kw)
    assert ticks >= 8 and len(o.assoc.landmarks) >= 3 and o.last_stats["optimized"]
    # the same events at the defaults end elsewhere: a side that ignored the parameter could not agree with one that reads it
    assert _signature(o) != _plain_run(events)


def test_first_landmark_state_right_after_construction():
    o = oracle_instance(**K.BUCKET_FIRST_LAN)
    c = SlamTickC(**K.BUCKET_FIRST_LAN)
    assert [k["node"] for k in o.keyframes] == [0] and np.array_equal(o.est[0], [0, 0, 0, 0, 0, 0, 1]) and not o.queue
    assert len(o.assoc.landmarks) == 1 and not o.assoc.first_object and not o.first_key_added and o.is_first
    l = o.assoc.landmarks[0]
    assert (l["id"], l["vertex"], l["class_id"], l["plane_type"]) == (0, 1, K.CLASS_BUCKET, 1)
    assert np.array_equal(l["covariance"], np.diag([F(0.1)] * 3)) and np.array_equal(l["normal"], np.array([-0.4, 0.86, 0, 0], F))
    assert np.array_equal(l["pose"], np.array(K.BUCKET_FIRST_LAN["first_lan"], F))
    assert (list(o.vtype), list(o.etype), o.evi, o.evj) == ([S.O.VT_SE3, S.O.VT_POINT], [S.O.ET_SE3_POINT], [0], [1])
    assert np.allclose(o.info[0][:9].reshape(3, 3), 10 * np.eye(3), rtol=1e-6)
    g = c.graph()
    assert c.counts() == (2, 1, 1, 1) and np.array_equal(g["est"], np.array(o.est)) and np.array_equal(g["meas"], np.array(o.meas))
    assert np.array_equal(g["info"], np.array(o.info))


def test_threshold_frames_decide_as_stated_on_the_oracle():
    for kw, frames, expect in K.threshold_frames():
        D = S.DataAssociation(**kw)
        got = [D.find_matches(objs, pose, F(0.0), lambda l: l["pose"])[0] for pose, objs in frames]
        assert got[0]["is_new"] and got[0]["id"] == 0 and np.array_equal(got[0]["pose"], K.C_THRES)
        for g, (new, lid, dist) in zip(got[1:], expect):
            assert (int(g["is_new"]), g["id"]) == (new, lid)
            if dist is not None:
                assert g["distance"] == dist
        assert got[2]["distance"] > expect[0][2]              # the second probe is past the threshold by rounding-proof arithmetic


# ---- the conditions of the GPU file ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _anisotropic_table():
    o = oracle_instance(**K.ANISO_KW)
    assert K.anisotropic_run(o, False) == 4 and o.last_stats["optimized"] and o.last_stats["marginals_ok"]
    return K.oracle_table(o), o.last_stats["opt"].chi2_after


def test_anisotropic_run_reaches_every_pivot_pattern():
    (est, cov, kinds), chi2 = _anisotropic_table()
    assert len(est) >= 30 and chi2 < 1e-20
    A = [c + F(0.5) * np.eye(3, dtype=F) for c in cov]
    pat = [K.pivot_pattern(a) for a in A]
    for first in (False, True):
        for second in (False, True):
            assert pat.count((first, second)) >= 3, (first, second, pat.count((first, second)))
    assert max(np.linalg.cond(a.astype(float)) for a in A) >= 100


def test_probes_keep_their_margins_and_the_float32_restatement_is_within_its_bound():
    """of the probes of the GPU file's distance test at most 5 % fall to the margin filter, the float32 oracle takes every decision
    the float64 replay takes, and its distance is within 2 eps32 cond(S + qI) d of the float64 value: the reference error that the
    device bar of PROBE_FACTOR = 8 is a multiple of"""
    table, _ = _anisotropic_table()
    frames, expect, dropped = K.make_probes(table)
    assert dropped <= 0.05 and len(expect) >= 1500 and max(len(f) for f in frames) <= 40
    new = sum(e[0] for e in expect)
    assert 200 <= new <= len(expect) - 200                   # both decisions are taken often
    D = K.seeded_association(table)
    got = [r for objs in frames for r in D.find_matches(objs, K.PROBE_POSE, F(0.0), lambda l: l["pose"])]
    assert [(int(r["is_new"]), r["id"]) for r in got] == [e[:2] for e in expect]
    worst = max(abs(r["distance"] - e[2]) / (K.EPS32 * e[3] * e[2]) for r, e in zip(got, expect))
    print("np_slam.mahalanobis against float64, worst |d - d64| / (eps32 cond d64):", worst)
    assert worst <= 2.0
    roll, pitch = float(K.PROBE_POSE[3]), float(K.PROBE_POSE[4])
    assert abs(roll) > 0.1 and abs(pitch) > 0.1


def test_slow_replay_is_decided_by_the_whole_second_clause():
    events, _ = K.slow_replay()
    o = oracle_instance()
    by_time = borrowed = ticks = 0
    for ev in events:
        first, pre, (psec, pnsec) = o.is_first, o.prev_keypose, o.prev_stamp
        if ev.objects is not None:
            o.set_segmented_objects(ev.objects)
        kf = o.vio(ev.stamp[0], ev.stamp[1], ev.odom)
        if not first:
            delta = S.iso_inv(pre) @ S.tq_to_iso(ev.odom)
            dx, da = np.linalg.norm(delta[:3, 3]), math.acos(min(1.0, S.iso_to_tq(delta)[6]))
            by_time += kf and dx < o.dt and da < o.da_
            # a full second by the seconds field alone, not yet one with the nanoseconds: rejected only because of the borrow
            borrowed += (not kf) and ev.stamp[0] - psec == 1 and ev.stamp[1] < pnsec
        if ev.run_after:
            ticks += o.run()
    assert by_time >= 20 and borrowed >= 20 and ticks >= 20 and len(o.assoc.landmarks) >= 3


def test_tilt_world_rolls_and_pitches_the_robot():
    events, _ = make_replay(0, n_samples=220)
    o = oracle_instance()
    for ev in K.tilt_world(events):
        if ev.objects is not None:
            o.set_segmented_objects(ev.objects)
        o.vio(ev.stamp[0], ev.stamp[1], ev.odom)
        if ev.run_after:
            o.run()
    rpy = np.array([S.matrix2vector(k["robot_pose"])[3:] for k in o.keyframes])
    assert np.abs(rpy[:, 0]).max() >= 0.3 and np.abs(rpy[:, 1]).max() >= 0.3
    assert len(o.assoc.landmarks) >= 8


@pytest.mark.parametrize("seed", [0, 1])
def test_pitched_detections_map_the_true_landmarks(seed):
    kw = K.SHIPPED["bucket_detector"]
    events, lms = K.events_for(kw, seed=seed, n_samples=300, detect_every=3)
    o = oracle_instance(**kw)
    for ev in events:
        if ev.objects is not None:
            o.set_segmented_objects(ev.objects)
        o.vio(ev.stamp[0], ev.stamp[1], ev.odom)
        if ev.run_after:
            o.run()
    assert len(o.assoc.landmarks) >= 8 and _map_error(o, lms) < 0.25
