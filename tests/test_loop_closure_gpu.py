"""Loop closing in the tick on the GPU: the candidate kernel (k_loop_candidates) against loop_ref.candidates_ref by integer equality, and
the tick with loop closure on against a prediction made from the same device primitives (voxel grid, register_pairs -- both repeat their
bits) and against oracle/np_slam.py's tick with the reported loop edges injected (tests/loop_ref.py).  The replay is tests/loop_scene.py's;
tests/test_loop_closure_cpu.py checks on the reference chain alone that it has loops to close, a refused match, a tick where an accepted
loop makes the next keyframe skip, and margins that keep a last-bit difference from flipping a decision.

Tick parity uses the tolerances of tests/test_slam_gpu.py as they are: estimates 1e-6 absolute, chi2 1e-6 relative."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import loop_ref as LR
import loop_scene as LS

pytestmark = pytest.mark.gpu


def _loop_struct(**kw):
    from semantic_slam_amd.semantic_graph_slam import default_loop_params
    p = default_loop_params()
    for k, v in dict(LS.LOOP_KW, **kw).items():
        if k == "inf":
            for (f, _), x in zip(p.inf._fields_, v):
                setattr(p.inf, f, x)
        else:
            setattr(p, k, v)
    return p


def _product(seg):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    p = default_slam_params()
    p.const_stddev_x, p.const_stddev_q = LS.ODOM_STDDEV_X, LS.ODOM_STDDEV_Q
    return SemanticGraphSLAM(p, seg)


@pytest.fixture(scope="module")
def seg(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    return PointCloudSegmentation()


@pytest.fixture(scope="module")
def events():
    return LS.make_events()


# ---- the candidate kernel --------------------------------------------------------------------------------------------------------------
def _table(n_keys, n_new, seed):
    """keys on an integer lattice (many exactly equal d2, equal positions 64 and more indices apart), travelled distance rising with the
    index; queries on the lattice too, half of the keys old enough for them; a NaN and an infinity in both"""
    rng = np.random.default_rng(seed)
    keys = np.zeros((n_keys, 3))
    keys[:, :2] = rng.integers(-6, 7, (n_keys, 2))
    keys[:, 2] = 0.125 * np.arange(n_keys)
    news = np.zeros((n_new, 3))
    news[:, :2] = rng.integers(-2, 3, (n_new, 2))
    news[:, 2] = 8.0 + 0.125 * (n_keys // 2) + 0.125 * np.arange(n_new)
    if n_keys >= 3:
        keys[1, 0] = math.nan; keys[n_keys - 1, 2] = math.inf; keys[n_keys // 2, 1] = -math.inf
    if n_new >= 3:
        news[1, 1] = math.nan; news[2, 0] = math.inf
    return keys, news


@pytest.mark.parametrize("n_keys", [0, 1, 63, 64, 65, 129, 1000])
def test_candidate_kernel_matches_the_reference(gpu_lib, n_keys):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_loop_params
    S = SemanticGraphSLAM()
    for n_new in (0, 1, 10):
        keys, news = _table(n_keys, n_new, 100 * n_keys + n_new)
        for m in (0, 1, 8, 64):
            p = default_loop_params()
            p.max_candidates = m
            _, full = LR.candidates_ref(keys, news, p.accum_distance_thresh, p.distance_thresh, m)
            top = int(full.max()) if n_new else 0
            if n_keys >= 63 and n_new == 10:
                assert top >= min(m, 8) if m else top > 8                     # the table does have candidates to choose among
            for cap in sorted({top // 2, top + 3, 0}):
                cand, count = S.loop_candidates(keys, news, p, cap)
                rc, rn = LR.candidates_ref(keys, news, p.accum_distance_thresh, p.distance_thresh, m, cap)
                assert cand.shape == rc.shape == (n_new, cap)
                assert np.array_equal(count, rn) and np.array_equal(cand, rc), (n_keys, n_new, m, cap)
    if n_keys == 1000:   # repeating a call repeats its answer; a second handle gives it too
        again, _ = SemanticGraphSLAM().loop_candidates(keys, news, p, cap)
        assert np.array_equal(again, cand)


def test_candidate_kernel_at_its_thresholds(gpu_lib):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_loop_params
    S = SemanticGraphSLAM()
    p = default_loop_params()                                                 # 5 m, 8 m
    up = lambda v: math.nextafter(v, math.inf)
    under = 10.0 - math.nextafter(8.0, 0.0)     # the travelled distance that leaves the largest double below 8
    keys = np.array([[0, 0, 2.0],               # travelled difference exactly 8: passes
                     [0, 0, under],             # one double step under it: fails
                     [3, 4, 0.0],               # d2 = 9 + 16 = 25 exactly: passes
                     [up(3.0), 4, 0.0],         # one double step over it: fails
                     [-4, -up(3.0), 0.0],       # fails
                     [-3, -4, 1.0]])            # passes
    news = np.array([[0, 0, 10.0]])
    assert 10.0 - under == math.nextafter(8.0, 0.0) and up(3.0) * up(3.0) + 4.0 * 4.0 == up(25.0) == 4.0 * 4.0 + up(3.0) * up(3.0)
    cand, count = S.loop_candidates(keys, news, p)
    assert list(count) == [3] and list(cand[0]) == [0, 2, 5, -1, -1, -1]
    rc, rn = LR.candidates_ref(keys, news, 8.0, 5.0)
    assert np.array_equal(cand, rc) and np.array_equal(count, rn)
    # groups of equal d2 that straddle the M-th place, their members 64 and more indices apart: the lowest indices win, in (d2, index) order
    keys = np.zeros((300, 3))
    keys[:, 0] = 4.0                                                          # d2 = 16 everywhere ...
    for i in (3, 70, 140, 260):
        keys[i, :2] = (1.0, 0.0)                                              # ... but for a group at d2 = 1 ...
    keys[100, :2] = (0.0, 0.0)                                                # ... and one at 0
    keys[200, :2] = (0.0, -1.0)                                               # the group at 1 again, another place
    for m, want in [(1, [100]), (3, [100, 3, 70]), (4, [100, 3, 70, 140]), (6, [100, 3, 70, 140, 200, 260]), (8, [100, 3, 70, 140, 200, 260, 0, 1])]:
        p.max_candidates = m
        cand, count = S.loop_candidates(keys, news, p)
        assert list(count) == [m] and list(cand[0]) == want
        rc, _ = LR.candidates_ref(keys, news, 8.0, 5.0, m)
        assert np.array_equal(cand, rc)
    p.max_candidates = 64
    cand, count = S.loop_candidates(keys, news, p, 70)
    assert list(count) == [64] and list(cand[0, :8]) == [100, 3, 70, 140, 200, 260, 0, 1] and list(cand[0, 64:]) == [-1] * 6
    assert list(cand[0, 6:64]) == [k for k in range(300) if k not in (3, 70, 100, 140, 200, 260)][:58]


# ---- the tick ------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _compare_with_oracle(Sp, Or, tol=1e-6):
    """the checks of tests/test_slam_gpu.py's tick parity for a replay without landmarks, at its tolerances"""
    from oracle import np_slam as NS
    st, so = Sp.last_stats, Or.last_stats
    assert (st.keyframes_added, bool(st.optimized), bool(st.marginals_ok)) == (so["keyframes_added"], so["optimized"], so["marginals_ok"])
    if so["optimized"]:
        print("chi2", st.opt.chi2_after, so["opt"].chi2_after)
        assert abs(st.opt.chi2_after - so["opt"].chi2_after) <= 1e-6 * max(1.0, so["opt"].chi2_after)
    ids, est = Sp.getKeyframes()
    assert list(ids) == [k["node"] for k in Or.keyframes]
    for v, e in zip(ids, est):
        eo = Or.est[v]
        s = 1.0 if np.dot(e[3:], eo[3:]) >= 0 else -1.0
        assert np.abs(e[:3] - eo[:3]).max() <= tol and np.abs(e[3:] - s * eo[3:]).max() <= tol
    assert np.abs(Sp.getRobotPose()[:3] - NS.iso_to_tq(Or.robot_pose)[:3]).max() <= tol
    assert np.abs(Sp.getMap2OdomTrans()[:3] - NS.iso_to_tq(Or.map2odom)[:3]).max() <= 10 * tol


def _replay_off(seg, events):
    Sp = _product(seg)
    for ev in events:
        Sp.setPointCloudData(ev.cloud)
        Sp.VIOCallback(ev.stamp, ev.odom)
        if ev.run_after:
            assert Sp.run() and Sp.last_loops() == []
    return Sp


def _tick_matches_prediction_and_oracle(seg, events):
    """a replay with loop closure on, every tick against the prediction from the device primitives and against the oracle tick with the
    reported edges injected; returns the (record, measurement) of every loop edge added"""
    from semantic_slam_amd.segmentation import InfParams, information_from_fitness
    P = LR.loop_params(**LS.LOOP_KW)
    struct = _loop_struct()
    Sp = _product(seg)
    Sp.set_loop_closure(struct)
    Or = LR.LoopOracle(const_stddev_x=LS.ODOM_STDDEV_X, const_stddev_q=LS.ODOM_STDDEV_Q)
    R = LR.Replay(P, lambda xyz, leaf: seg.downsamplePointcloud(xyz, leaf)[0])
    register = lambda clouds, pairs, mi, eps: seg.register_pairs(clouds, pairs, max_iterations=mi, epsilon=eps)
    outcomes, first_tick, all_loops = [], True, []
    for ev in events:
        Sp.setPointCloudData(ev.cloud)
        kp = Sp.VIOCallback(ev.stamp, ev.odom)
        assert kp == R.sample(ev) == bool(Or.vio(ev.stamp[0], ev.stamp[1], ev.odom))
        if not ev.run_after:
            continue
        ids, est = Sp.getKeyframes()
        news = R.begin_tick(est)
        want, _ = R.predict(news, register)
        edges = Sp.num_edges()
        assert Sp.run()
        got = Sp.last_loops()
        odometry_edges = len(news) - (1 if first_tick else 0)
        first_tick = False
        assert [(g.new_vertex, g.cand_vertex, g.n_candidates, g.outcome, g.used, g.iterations, g.converged) for g in got] == \
               [(w["new_vertex"], w["cand_vertex"], w["n_candidates"], w["outcome"], w["used"], w["iterations"], w["converged"]) for w in want]
        added = 0
        loops = []
        for g, w in zip(got, want):
            assert _bits(g.T[:]) == _bits(w["T"]) and _bits(g.score) == _bits(w["score"]) and math.isnan(g.d2)
            if g.outcome == LR.ADDED:
                assert g.edge_id == edges + odometry_edges + added
                added += 1
                info = information_from_fitness(g.score, struct.inf)
                assert np.abs(info - w["info"]).max() <= 1e-12 * np.abs(w["info"]).max()
                loops.append((g.new_vertex, g.cand_vertex, LR.measurement_of_T(g.T[:]), info))
                all_loops.append((g, loops[-1][2]))
            else:
                assert g.edge_id == -1
        assert Sp.num_edges() == edges + odometry_edges + added
        outcomes += [g.outcome for g in got]
        Or.pending_loops = loops
        assert Or.run()
        R.end_tick(news)
        assert list(Sp.getKeyframes()[0]) == [k["node"] for k in R.keyframes]
        _compare_with_oracle(Sp, Or)
    assert outcomes.count(LR.ADDED) >= 3 and LR.SCORE in outcomes
    truth = np.array([k["truth"] for k in R.keyframes])
    on = LS.rms_position_error(Sp.getKeyframes()[1], truth)
    off = LS.rms_position_error(_replay_off(seg, events).getKeyframes()[1], truth)
    print("rms position error: %.4f m with loop closure, %.4f m without" % (on, off))
    assert on < off
    return all_loops


def test_tick_with_loop_closure_matches_prediction_and_oracle(seg, events):
    _tick_matches_prediction_and_oracle(seg, events)


# ---- the half-turn replay: one lap and the same lap back ----------------------------------------------------------------------------------
_HALF_TURN_EVENTS = {}


def _half_turn_events(mount):
    if mount not in _HALF_TURN_EVENTS:
        _HALF_TURN_EVENTS[mount] = LS.make_events(path="out_and_back", fov_h=LS.FOV_PANORAMA, mount=LS.MOUNTS[mount])
    return _HALF_TURN_EVENTS[mount]


@pytest.mark.parametrize("mount", list(LS.MOUNTS))
def test_tick_closes_loops_at_a_half_turn(seg, mount):
    """T0 = inverse(new) o old a half turn from the identity, the matcher's T with its pivot on R[8], R[0] or R[4] (the mount decides), and
    loop edges whose quaternion has w near 0: the three other branches of measurement_of_T and the SE3 edge far from the identity, in the
    tick, against the oracle.  tests/test_loop_closure_cpu.py shows on the reference chain that the replay has such loops."""
    loops = _tick_matches_prediction_and_oracle(seg, _half_turn_events(mount))
    for g, z in loops:
        print("loop", g.new_vertex, g.cand_vertex, "trace %.4f" % (g.T[0] + g.T[4] + g.T[8]), "q", z[3:])
    half = [(g, z) for g, z in loops if abs(z[6]) < 0.1]
    assert len(half) >= 3
    pivot = {"I": 5, "z->x": 3, "z->y": 4}[mount]                               # the half turn is about the sensor's z, x or y
    assert all(abs(z[pivot]) > 0.99 for _, z in half)


def _until_tick(seg, events, last, gate_chi2):
    """the half-turn replay (no mount) with the gate wide open (its distance is reported, nothing is refused) up to the tick after
    events[last], which runs with `gate_chi2`; returns (records of that tick, edges the tick added, its new keyframes)"""
    Sp = _product(seg)
    Sp.set_loop_closure(_loop_struct(gate_chi2=1e300))
    pending = 0
    for ev in events[:last + 1]:
        Sp.setPointCloudData(ev.cloud)
        pending += Sp.VIOCallback(ev.stamp, ev.odom)
        if not ev.run_after:
            continue
        if ev is events[last]:
            Sp.set_loop_closure(_loop_struct(gate_chi2=gate_chi2))
        edges = Sp.num_edges()
        assert Sp.run()
        if ev is events[last]:
            return Sp.last_loops(), Sp.num_edges() - edges, pending
        assert all(r.outcome != LR.GATE for r in Sp.last_loops())
        pending = 0
    raise AssertionError("no tick")


def test_gate_decides_on_the_reported_distance_at_a_half_turn(seg):
    """test_gate_decides_on_the_reported_distance for the first two loops of the way back: the error of the candidate edge is taken
    between poses a half turn apart, where a quaternion difference formed with the wrong sign would be a full turn"""
    events = _half_turn_events("I")
    assert events[35].run_after and events[39].run_after
    for last in (35, 39):
        A, edges_a, n_a = _until_tick(seg, events, last, 1e300)
        first = next(k for k, r in enumerate(A) if r.outcome == LR.ADDED and r.T[0] + r.T[4] + r.T[8] < 0)
        d = A[first].d2
        print("tick after event", last, "loop", A[first].new_vertex, A[first].cand_vertex, "d2", d)
        assert math.isfinite(d) and d > 0
        assert edges_a == n_a + sum(r.outcome == LR.ADDED for r in A)
        B, edges_b, n_b = _until_tick(seg, events, last, d / 2)
        assert (B[first].new_vertex, B[first].cand_vertex) == (A[first].new_vertex, A[first].cand_vertex)
        assert _bits(B[first].T[:]) == _bits(A[first].T[:]) and _bits(B[first].score) == _bits(A[first].score) and _bits(B[first].d2) == _bits(d)
        assert B[first].outcome == LR.GATE and B[first].edge_id == -1
        assert edges_b == n_b + sum(r.outcome == LR.ADDED for r in B)
        assert all(r.d2 < d / 2 for r in B if r.outcome == LR.ADDED) and all(not r.d2 < d / 2 for r in B if r.outcome == LR.GATE)
        Cc, edges_c, n_c = _until_tick(seg, events, last, 2 * d)
        assert Cc[first].outcome == LR.ADDED and _bits(Cc[first].d2) == _bits(d) and Cc[first].edge_id == A[first].edge_id
        assert edges_c == edges_a
        for k in range(first):                                                  # what came before it in the tick is the same in all three
            assert A[k].outcome == B[k].outcome == Cc[k].outcome and _bits(A[k].d2) == _bits(B[k].d2) == _bits(Cc[k].d2)


def test_off_is_off(seg, events):
    """a handle that never called the setter and one that called it with NULL (after having had it on before any keyframe): bitwise the
    same ticks, clouds and detections fed to both, and no loop records"""
    from semantic_slam_amd.synth import make_replay
    from tests.slam_replay import feed
    plain, nulled = _product(seg), _product(seg)
    nulled.set_loop_closure(_loop_struct())
    nulled.set_loop_closure(None)
    replay, _ = make_replay(0, n_samples=220)
    ticks = 0
    for k, ev in enumerate(replay):
        states = []
        for Sp in (plain, nulled):
            Sp.setPointCloudData(events[k % len(events)].cloud)
            kf, ran = feed(Sp, ev, True)
            if ran:
                assert Sp.last_loops() == [] and not Sp.last_loop_timing().any()
                ids, est = Sp.getKeyframes()
                lms = [(l.id, l.vertex, tuple(l.pose), tuple(l.covariance)) for l in Sp.getMappedLandmarks()]
                states.append((kf, ids.tobytes(), est.tobytes(), lms, Sp.num_edges(), Sp.getRobotPose().tobytes()))
            else:
                states.append((kf,))
        assert states[0] == states[1]
        ticks += len(states[0]) > 1
    assert ticks >= 5 and len(plain.getMappedLandmarks()) >= 1 and plain.num_edges() >= 10


@pytest.mark.parametrize("kernel", [None, 0])
def test_loop_edges_carry_the_robust_kernel(gpu_lib, seg, events, kernel):
    """the default parameters' kernel (Huber, 1.0) on every loop edge; none with robust_kernel = 0"""
    from semantic_slam_amd.semantic_graph_slam import default_loop_params
    import ctypes as C
    d = default_loop_params()
    struct = _loop_struct(robust_kernel=d.robust_kernel if kernel is None else kernel, robust_delta=d.robust_delta)
    Sp = _product(seg)
    Sp.set_loop_closure(struct)
    g = gpu_lib.sslam_slam_graph(Sp._h)
    seen = 0
    for ev in events[:36]:
        Sp.setPointCloudData(ev.cloud)
        Sp.VIOCallback(ev.stamp, ev.odom)
        if not ev.run_after:
            continue
        assert Sp.run()
        for L in Sp.last_loops():
            if L.outcome != LR.ADDED:
                continue
            kind, delta = C.c_int(-1), C.c_double(-1.0)
            assert gpu_lib.sslam_graph_get_edge_robust_kernel(g, L.edge_id, C.byref(kind), C.byref(delta)) == 0
            assert (kind.value, delta.value) == ((1, 1.0) if kernel is None else (0, 0.0))
            seen += 1
    assert seen >= 2


def _until_first_loop(seg, events, gate_chi2):
    """the replay up to the tick of replay A's first loop; returns (records of that tick, edges the tick added, its new keyframes)"""
    Sp = _product(seg)
    Sp.set_loop_closure(_loop_struct(gate_chi2=gate_chi2))
    pending = 0
    for ev in events[:28]:
        Sp.setPointCloudData(ev.cloud)
        pending += Sp.VIOCallback(ev.stamp, ev.odom)
        if not ev.run_after:
            continue
        edges = Sp.num_edges()
        assert Sp.run()
        recs = Sp.last_loops()
        if ev is events[27]:
            return recs, Sp.num_edges() - edges, pending
        assert all(r.outcome == LR.SCORE for r in recs)
        pending = 0
    raise AssertionError("no tick")


def test_gate_decides_on_the_reported_distance(seg, events):
    A, edges_a, n_a = _until_first_loop(seg, events, 1e300)
    first = next(k for k, r in enumerate(A) if r.outcome == LR.ADDED)
    d = A[first].d2
    print("d2 of the first loop", d)
    assert math.isfinite(d) and d > 0
    assert edges_a == n_a + sum(r.outcome == LR.ADDED for r in A)
    B, edges_b, n_b = _until_first_loop(seg, events, d / 2)
    assert (B[first].new_vertex, B[first].cand_vertex) == (A[first].new_vertex, A[first].cand_vertex)
    assert _bits(B[first].T[:]) == _bits(A[first].T[:]) and _bits(B[first].score) == _bits(A[first].score) and _bits(B[first].d2) == _bits(d)
    assert B[first].outcome == LR.GATE and B[first].edge_id == -1
    assert edges_b == n_b + sum(r.outcome == LR.ADDED for r in B)
    assert all(r.d2 < d / 2 for r in B if r.outcome == LR.ADDED) and all(not r.d2 < d / 2 for r in B if r.outcome == LR.GATE)
    Cc, edges_c, n_c = _until_first_loop(seg, events, 2 * d)
    assert Cc[first].outcome == LR.ADDED and _bits(Cc[first].d2) == _bits(d) and Cc[first].edge_id == A[first].edge_id
    assert edges_c == edges_a
    for k in range(first):                                                    # what came before the first loop never reached the gate
        assert A[k].outcome == B[k].outcome == Cc[k].outcome == LR.SCORE and math.isnan(A[k].d2)


# ---- the C++ shim --------------------------------------------------------------------------------------------------------------------
def test_cpp_shim_loop_end_to_end(gpu_lib, seg, events, tmp_path):
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, rec = str(tmp_path / "shim_loop"), str(tmp_path / "replay.bin")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_loop_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    with open(rec, "wb") as f:
        for ev in events[:32]:
            f.write(np.array([ev.stamp[0], ev.stamp[1], int(ev.run_after)], np.int32).tobytes())
            f.write(np.asarray(ev.odom, np.float64).tobytes())
            f.write(ev.cloud.cloud.tobytes())
    out = subprocess.run([exe, rec], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"shim loop ok: new (\d+) cand (\d+) candidates (\d+) edge (\d+) used (\d+) iterations (\d+) score (\S+) T((?: \S+){12})", out.stdout)
    assert m, out.stdout
    Sp = _product(seg)
    Sp.set_loop_closure(_loop_struct())
    mine = None
    for ev in events[:32]:
        Sp.setPointCloudData(ev.cloud)
        Sp.VIOCallback(ev.stamp, ev.odom)
        if ev.run_after and mine is None:
            assert Sp.run()
            mine = next((L for L in Sp.last_loops() if L.outcome == LR.ADDED), None)
    assert mine is not None
    # the shim hands the odometry over as a matrix, so its quaternions differ from the mirror's in the last bits: integers exactly, the
    # scan match to the bar of the gate shim's comparison
    assert [int(v) for v in m.groups()[:6]] == [mine.new_vertex, mine.cand_vertex, mine.n_candidates, mine.edge_id, mine.used, mine.iterations]
    print("shim", m.group(7), "mirror", mine.score)
    assert abs(float(m.group(7)) - mine.score) <= 1e-9 * mine.score
    assert np.abs(np.array([float(v) for v in m.group(8).split()]) - np.array(mine.T[:])).max() <= 1e-9
