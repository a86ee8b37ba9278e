"""Loop closing in the tick, the host side: defaults and argument checks of sslam_slam_set_loop_closure (no device needed), and the
conditions the replay of tests/loop_scene.py must meet for tests/test_loop_closure_gpu.py to mean something, asserted on the reference
chain alone (loop_ref + registration_ref.icp_ref + fitness_ref on oracle/np_slam.py's tick).

Figures of the reference chain on the replay (53 keyframes, two laps of 14.5 m, drift of the odometry 0.26 m rms): 6 loops added, 2
refused on their score, rms position error with the loop edges 0.51 of that without."""
import functools
import math

import numpy as np
import pytest

import loop_ref as LR
import loop_scene as LS
from fitness_ref import DBL_MAX
from oracle.np_filters import voxel_grid
from registration_ref import pose_error


# ---- the setter -----------------------------------------------------------------------------------------------------------------------
def test_defaults(hip_lib):
    from semantic_slam_amd.semantic_graph_slam import default_loop_params
    from semantic_slam_amd.segmentation import default_inf_params
    p = default_loop_params()
    assert (p.distance_thresh, p.accum_distance_thresh, p.distance_from_last_edge_thresh) == (5.0, 8.0, 5.0)
    assert (p.fitness_score_max_range, p.fitness_score_thresh) == (DBL_MAX, 0.5)
    assert (p.max_iterations, p.epsilon, p.max_candidates, p.gate_chi2) == (64, 0.01, 0, 0.0)
    assert p.voxel_leaf == np.float32(0.1)
    assert (p.robust_kernel, p.robust_delta) == (1, 1.0)                      # SSLAM_ROBUST_HUBER
    d = default_inf_params()
    assert all(getattr(p.inf, f) == getattr(d, f) for f, _ in d._fields_)
    ref = LR.loop_params()                                                    # the plain restatement the reference chain starts from
    for f, _ in p._fields_:
        if f == "inf":
            assert tuple(getattr(p.inf, g) for g, _ in d._fields_) == ref.inf
        else:
            assert getattr(p, f) == (np.float32(ref.voxel_leaf) if f == "voxel_leaf" else getattr(ref, f)), f


def _systems():
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    return SemanticGraphSLAM(), SemanticGraphSLAM(segmentation=PointCloudSegmentation())


BAD = [("distance_thresh", -1.0), ("distance_thresh", math.nan), ("accum_distance_thresh", -0.5), ("accum_distance_thresh", math.inf),
       ("distance_from_last_edge_thresh", -1.0), ("distance_from_last_edge_thresh", math.nan), ("fitness_score_max_range", -1.0),
       ("fitness_score_max_range", math.inf), ("fitness_score_thresh", -0.1), ("fitness_score_thresh", math.nan), ("gate_chi2", -1.0),
       ("gate_chi2", math.inf), ("voxel_leaf", -0.1), ("voxel_leaf", math.nan), ("max_candidates", -1), ("max_candidates", 65),
       ("max_iterations", -1), ("epsilon", -1e-9), ("epsilon", math.nan), ("robust_kernel", -1), ("robust_kernel", 8), ("robust_delta", 0.0),
       ("robust_delta", math.nan)]


def test_setter_refuses_bad_arguments(hip_lib):
    from semantic_slam_amd import SslamError
    from semantic_slam_amd.semantic_graph_slam import default_loop_params
    bare, full = _systems()
    full.set_loop_closure(default_loop_params())
    full.set_loop_closure(None)
    bare.set_loop_closure(None)                                               # off needs no frontend handle
    with pytest.raises(SslamError) as ei:
        bare.set_loop_closure(default_loop_params())
    assert ei.value.code == -1 and "frontend handle" in str(ei.value)
    for field, value in BAD:
        p = default_loop_params()
        setattr(p, field, value)
        with pytest.raises(SslamError) as ei:
            full.set_loop_closure(p)
        assert ei.value.code == -1, (field, value)
    for field, value in [("max_candidates", 64), ("max_iterations", 0), ("epsilon", 0.0), ("robust_kernel", 0), ("robust_kernel", 7),
                         ("gate_chi2", 12.59), ("voxel_leaf", 0.0), ("distance_thresh", 0.0)]:
        p = default_loop_params()
        setattr(p, field, value)
        full.set_loop_closure(p)
    p = default_loop_params()
    p.robust_kernel, p.robust_delta = 0, math.nan                             # no kernel: its width is not read
    full.set_loop_closure(p)
    assert full.last_loops() == []
    assert hip_lib.sslam_slam_set_loop_closure(None, None) == -1 and hip_lib.sslam_slam_last_loops(None, None, 0) == -1


# ---- the replay on the reference chain ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chains():
    events = LS.make_events()
    P = LR.loop_params(**LS.LOOP_KW)
    down = lambda xyz, leaf: voxel_grid(xyz, leaf)[0]
    return events, P, LR.oracle_replay(events, P, True, down), LR.oracle_replay(events, P, False, down)


def test_scene_is_a_room_seen_from_inside():
    ev = LS.make_events(30)
    for e in ev[::7]:
        xyz = e.cloud.xyz().astype(np.float64)
        assert xyz.shape == (LS.WIDTH * LS.HEIGHT, 3) and np.isfinite(xyz).all()
        c, s = math.cos(e.truth[3]), math.sin(e.truth[3])
        w = xyz @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + e.truth[:3]
        assert (w > -1e-4).all() and (w < np.array(LS.ROOM) + 1e-4).all()      # every point lies in the room ...
        inside = ((w > np.array(LS.BOX[0]) + 1e-3) & (w < np.array(LS.BOX[1]) - 1e-3)).all(1)
        assert not inside.any()                                                # ... and none inside the box
        on_box = ((w > np.array(LS.BOX[0]) - 1e-3) & (w < np.array(LS.BOX[1]) + 1e-3)).all(1)
        assert on_box.sum() > 20                                               # the box is in view
    steps = [np.linalg.norm(b.odom[:3] - a.odom[:3]) for a, b in zip(ev, ev[1:])]
    assert min(steps) > 0.5                                                    # every sample passes the keyframe gate


def test_replay_meets_the_conditions_of_the_gpu_test():
    events, P, on, off = _chains()
    records = [r for _, recs, _ in on.ticks for r in recs]
    added = [r for r in records if r["outcome"] == LR.ADDED]
    print("records", [(r["new_vertex"], r["cand_vertex"], r["n_candidates"], r["outcome"], round(r["score"], 5)) for r in records])
    assert len(added) >= 3
    # a new keyframe the tick's starting last_edge_accum let through and the running one passed over: a loop accepted earlier in the tick
    assert any(skipped > 0 and any(r["outcome"] == LR.ADDED for r in recs) for _, recs, skipped in on.ticks)
    assert any(r["n_candidates"] > 1 for r in records)
    assert any(r["outcome"] == LR.SCORE for r in records)
    assert all(r["margin"] > 1e-6 for r in records), [r["margin"] for r in records]
    # every accepted T within the scan matcher's reach of the truth: the grid of the clouds is voxel_leaf wide, so a translation is known
    # to within a cell and a rotation to within a cell over the 3 m to the nearest surfaces
    truth = [k["truth"] for k in on.replay.keyframes]
    for r in added:
        rot, tra = pose_error(r["T"], LS.truth_T(truth[r["new_vertex"]], truth[r["cand_vertex"]]))
        print("loop", r["new_vertex"], r["cand_vertex"], "score %.5f" % r["score"], "error %.4f rad %.4f m" % (rot, tra))
        assert tra < P.voxel_leaf and rot < P.voxel_leaf / 3.0
    print("rms position error: %.4f m with the loop edges, %.4f m without, ratio %.3f" % (on.rms, off.rms, on.rms / off.rms))
    assert on.rms < off.rms
    assert len(on.oracle.etype) == len(off.oracle.etype) + len(added)


# ---- the half-turn replay on the reference chain -----------------------------------------------------------------------------------------
# One lap and the same lap back (loop_scene, path "out_and_back"): the candidate search looks at positions alone, so every revisit on the
# way back pairs keyframes a half turn apart, T0 = inverse(new) o old is nowhere near the identity, and the loop edge's quaternion has
# w near 0.  Figures of the chain (52 keyframes): 7 loop records, 5 added -- one at the end of the way out, heading as at the start, and 4
# on the way back with trace(R) from -1.000 to -0.904 -- 2 refused on their score, smallest margin 0.11, rms 0.125 m against 0.294 m.
@functools.lru_cache(maxsize=None)
def _half_turn_chain(mount, loops=True):
    events = LS.make_events(path="out_and_back", fov_h=LS.FOV_PANORAMA, mount=LS.MOUNTS[mount])
    P = LR.loop_params(**LS.LOOP_KW)
    return P, LR.oracle_replay(events, P, loops, lambda xyz, leaf: voxel_grid(xyz, leaf)[0])


def _branch(T):
    """which branch of measurement_of_T (csrc/sslam_slam.hip) a T takes, by the branch conditions themselves: "w", or the index of the pivot"""
    R = [float(x) for x in T[:9]]
    if R[0] + R[4] + R[8] > 0:
        return "w"
    if R[0] > R[4] and R[0] > R[8]:
        return 0
    return 4 if R[4] > R[8] else 8


def test_default_arguments_are_the_replay_of_before():
    a, b = LS.make_events(12), LS.make_events(12, path="laps", fov_h=LS.FOV_H, mount=None)
    for x, y in zip(a, b):
        assert x.odom.tobytes() == y.odom.tobytes() and x.cloud.cloud.tobytes() == y.cloud.cloud.tobytes() and x.truth.tobytes() == y.truth.tobytes()
    assert LS.cast(a[3].truth).cloud.tobytes() == a[3].cloud.cloud.tobytes()
    # the identity mount changes nothing but the sign of a zero; the others permute the coordinates of the cloud and turn the pose
    e0 = LS.make_events(6, path="out_and_back", fov_h=LS.FOV_PANORAMA)
    for name, C in LS.MOUNTS.items():
        assert abs(np.linalg.det(C) - 1) < 1e-15 and (C.T @ C == np.eye(3)).all()
        e = LS.make_events(6, path="out_and_back", fov_h=LS.FOV_PANORAMA, mount=C)
        for x, y in zip(e0, e):
            assert (y.cloud.xyz() == (x.cloud.xyz().astype(np.float64) @ C).astype(np.float32)).all()
            assert np.abs(np.array(LR.qmat(y.odom[3:])).reshape(3, 3) - np.array(LR.qmat(x.odom[3:])).reshape(3, 3) @ C).max() < 1e-15
    z = np.array([0.0, 0.0, 1.0])
    assert (LS.MOUNTS["z->x"].T @ z == [1, 0, 0]).all() and (LS.MOUNTS["z->y"].T @ z == [0, 1, 0]).all()


def test_out_and_back_is_a_lap_and_the_same_lap_back():
    ev = LS.make_events(path="out_and_back", fov_h=LS.FOV_PANORAMA)
    tr = np.array([e.truth for e in ev])
    assert len(ev) == 54 and sum(e.run_after for e in ev) == 13
    out, back = tr[:27], tr[27:]
    assert np.abs(np.diff(tr[:, 3])).max() <= math.pi + 1e-9                    # the yaw is continuous but for the turn on the spot
    # a half turn, less what the tangent turns over 0.3 of a step: the curvature is SEMI[0] / SEMI[1]^2 = 0.97 / m at most
    assert abs(abs(back[0, 3] - out[-1, 3]) - math.pi) <= LS.RETURN_OFFSET * LS.STEP * LS.SEMI[0] / LS.SEMI[1] ** 2
    d = np.linalg.norm(back[:, None, :2] - out[None, :, :2], axis=2)
    assert (d.min(1) > 0.25 * LS.STEP * LS.RETURN_OFFSET).all() and (d.min(1) < LS.STEP).all()      # between the samples of the way out, not on them
    for e in ev[::9]:                                                          # the panorama sees the room all the way round
        c, s = math.cos(e.truth[3]), math.sin(e.truth[3])
        w = e.cloud.xyz().astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + e.truth[:3]
        assert (w > -1e-4).all() and (w < np.array(LS.ROOM) + 1e-4).all()
        az = np.arctan2(e.cloud.xyz()[:, 1], e.cloud.xyz()[:, 0])
        assert az.max() - az.min() > 6.0


@pytest.mark.parametrize("mount", list(LS.MOUNTS))
def test_half_turn_replay_meets_the_conditions_of_the_gpu_test(mount):
    P, on = _half_turn_chain(mount)
    C = LS.MOUNTS[mount]
    records = [r for _, recs, _ in on.ticks for r in recs]
    added = [r for r in records if r["outcome"] == LR.ADDED]
    print("records", [(r["new_vertex"], r["cand_vertex"], r["n_candidates"], r["outcome"], round(r["score"], 5)) for r in records])
    half = [r for r in added if r["T"][0] + r["T"][4] + r["T"][8] < -0.9]
    assert len(half) >= 3
    assert any(r["outcome"] == LR.SCORE for r in records)
    assert all(r["margin"] > 1e-6 for r in records), [r["margin"] for r in records]
    truth = [k["truth"] for k in on.replay.keyframes]
    for r in added:
        rot, tra = pose_error(r["T"], LS.truth_T(truth[r["new_vertex"]], truth[r["cand_vertex"]], C))
        print("loop", r["new_vertex"], r["cand_vertex"], "score %.5f" % r["score"], "trace %.4f" % (r["T"][0] + r["T"][4] + r["T"][8]),
              "error %.4f rad %.4f m" % (rot, tra), "branch", _branch(r["T"]), "q", r["z"][3:])
        assert tra < P.voxel_leaf and rot < P.voxel_leaf / 3.0
        # the measurement is the rotation it was taken from, whichever branch made it
        assert np.abs(np.array(LR.qmat(r["z"][3:])) - r["T"][:9]).max() < 1e-12 and abs(np.linalg.norm(r["z"][3:]) - 1) < 1e-12
    # the three mounts put the pivot of the half turn on R[8], R[0] and R[4]: the three branches no other replay reaches
    assert {_branch(r["T"]) for r in half} == {{"I": 8, "z->x": 0, "z->y": 4}[mount]}
    assert sum(abs(r["z"][6]) < 0.1 for r in half) >= 3                         # w near 0: its sign is arbitrary
    assert any(_branch(r["T"]) == "w" for r in added)
    if mount == "I":
        _, off = _half_turn_chain(mount, False)
        print("rms position error: %.4f m with the loop edges, %.4f m without, ratio %.3f" % (on.rms, off.rms, on.rms / off.rms))
        assert on.rms < off.rms
        assert len(on.oracle.etype) == len(off.oracle.etype) + len(added)


def test_mounts_decide_alike():
    """the mount permutes coordinates and nothing else: the same records, decisions, iteration counts and scores under all three"""
    runs = {m: [r for _, recs, _ in _half_turn_chain(m)[1].ticks for r in recs] for m in LS.MOUNTS}
    key = lambda recs: [(r["new_vertex"], r["cand_vertex"], r["n_candidates"], r["outcome"], r["used"], r["iterations"], r["converged"]) for r in recs]
    assert key(runs["I"]) == key(runs["z->x"]) == key(runs["z->y"])
    # the float32 squared distances add their three terms in another order: a few 2^-24 each, and so their mean
    for a, b in zip(runs["I"], runs["z->y"]):
        assert abs(a["score"] - b["score"]) <= 1e-6 * a["score"]


def test_candidates_ref_on_a_hand_made_table():
    keys = np.array([[0, 0, 0], [3, 4, 1], [0, 5, 2], [3, 4, 2.5], [0, 0, 9.5], [math.nan, 0, 0], [1, 1, math.inf]], np.float64)
    news = np.array([[0, 0, 10.0], [0, 0, math.nan]])
    cand, count = LR.candidates_ref(keys, news, 8.0, 5.0)
    assert list(count) == [3, 0] and list(cand[0, :3]) == [0, 1, 2]            # 3 is too recent (7.5 < 8), 4 much too recent
    cand, count = LR.candidates_ref(keys, news, 7.5, 5.0, max_candidates=3)
    assert list(count) == [3, 0] and list(cand[0]) == [0, 1, 2]                # d2 0, then 25 three times: the two lowest indices of them
    cand, count = LR.candidates_ref(keys, news, 7.5, 5.0, max_candidates=4, cap=2)
    assert list(count) == [4, 0] and list(cand[0]) == [0, 1]
