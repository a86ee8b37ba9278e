"""sslam_seg_fitness_scores (k_nn_pairs + k_nn_finish), sslam_slam_set_fitness_information and the C++ shim's
InformationMatrixCalculator on the GPU.  Reference: tests/fitness_ref.py, the float32 arithmetic of include/sslam.h restated in NumPy
(pinned against scipy's k-d tree in tests/test_fitness_cpu.py).
Bounds, derived and not tuned: the nearest-neighbour index and squared distance are BITWISE the reference's; `used` is equal; the score
is the library's fixed-order double sum against math.fsum of the same addends, which any summation order of n non-negative doubles
meets within n * 2^-52 relative."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from fitness_ref import DBL_MAX, IDENTITY_T, fitness_ref, information_ref, qmat, skew_T

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def seg(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    return PointCloudSegmentation()


def _cloud(rng, n, scale=(3.0, 2.0, 0.5)):
    return (rng.normal(size=(n, 3)) * scale).astype(np.float32)


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


def _check_pair(got, ref, what):
    """got = (score, used, idx, d2) of the library, ref the same of fitness_ref"""
    score, used, idx, d2 = got
    rscore, rused, ridx, rd2 = ref
    assert idx.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(idx, ridx), what
    assert d2.tobytes() == rd2.tobytes(), what
    assert used == rused, what
    if rused == 0:
        assert score == DBL_MAX, what
    else:
        err = abs(score - rscore) / rscore if rscore > 0 else abs(score - rscore)
        print(f"{what}: score {score:.17g} ref {rscore:.17g} rel err {err:.3e} (bound {rused * 2.0 ** -52:.3e}), used {used}")
        assert err <= rused * 2.0 ** -52, what


def _one(seg, tg, sr, T, max_range=None):
    score, used, nn = seg.fitness_scores([tg, sr], [(0, 1, T, max_range)], return_nn=True)
    return float(score[0]), int(used[0]), nn[0][0], nn[0][1]


def test_nn_arrays_bit_exact(seg):
    from semantic_slam_amd.segmentation import NN_Q, NN_TILE
    rng = np.random.default_rng(11)
    T = skew_T()
    clouds, pairs, refs, names = [], [], [], []
    for nt in (NN_TILE - 1, NN_TILE, NN_TILE + 1, 700):
        tg = _cloud(rng, nt)
        ti = len(clouds)
        clouds.append(tg)
        for ns in (1, NN_Q - 1, NN_Q, NN_Q + 1, 333):
            sr = _cloud(rng, ns)
            clouds.append(sr)
            pairs.append((ti, len(clouds) - 1, T, 0.1))
            refs.append(fitness_ref(tg, sr, T, 0.1))
            names.append(f"{nt} targets x {ns} sources")
    score, used, nn = seg.fitness_scores(clouds, pairs, return_nn=True)
    assert len(nn) == len(pairs) and sum(r[1] for r in refs) > 100 and any(r[1] < len(r[2]) for r in refs)   # max_range bites, and not always
    for k, ref in enumerate(refs):
        _check_pair((float(score[k]), int(used[k]), nn[k][0], nn[k][1]), ref, names[k])
    # one pair on its own: the same bits as inside the batch, with and without a bound
    for k in (3, 17):
        tg, sr = clouds[pairs[k][0]], clouds[pairs[k][1]]
        alone = _one(seg, tg, sr, T, 0.1)
        assert alone[0] == score[k] and alone[1] == used[k] and np.array_equal(alone[2], nn[k][0]) and alone[3].tobytes() == nn[k][1].tobytes()
        _check_pair(_one(seg, tg, sr, T), fitness_ref(tg, sr, T), names[k] + ", no bound")


def test_ties_go_to_the_lowest_index(seg):
    rng = np.random.default_rng(12)
    half = _cloud(rng, 350)
    for tg in (np.concatenate([half, half]), np.repeat(half, 2, axis=0)):     # the twin 350 places later, and the twin next door
        sr = np.concatenate([_cloud(rng, 200), half[::7]])                      # the last 50 sit exactly on a target
        got = _one(seg, tg, sr, IDENTITY_T)
        _check_pair(got, fitness_ref(tg, sr, IDENTITY_T), "ties")
        idx = got[2]
        twin_first = np.array_equal(tg[0], tg[1])
        assert ((idx % 2 == 0) if twin_first else (idx < 350)).all()
        assert (got[3][200:] == 0).all()
        for chunk in (1, 256):                                                  # the twins on either side of a chunk boundary
            split = _with_chunk(chunk, lambda: _one(seg, tg, sr, IDENTITY_T))
            assert split[0] == got[0] and split[1] == got[1] and np.array_equal(split[2], idx) and split[3].tobytes() == got[3].tobytes()


def test_non_finite_points(seg):
    rng = np.random.default_rng(13)
    tg, sr = _cloud(rng, 700), _cloud(rng, 333)
    for a in (tg, sr):
        bad = rng.choice(len(a), len(a) // 20, replace=False)
        a[bad, rng.integers(0, 3, len(bad))] = np.nan
        a[rng.choice(len(a), 3, replace=False), 1] = np.inf
        a[rng.choice(len(a), 2, replace=False), 2] = -np.inf
    T = skew_T()
    got = _one(seg, tg, sr, T)
    _check_pair(got, fitness_ref(tg, sr, T), "5 % NaN, a few inf")
    sbad, tbad = ~np.isfinite(sr).all(1), ~np.isfinite(tg).all(1)
    assert sbad.sum() >= 16 and tbad.sum() >= 35
    assert (got[2][sbad] == -1).all() and (got[3][sbad] == -1.0).all() and (got[2][~sbad] >= 0).all()
    assert not tbad[got[2][~sbad]].any()                                        # a non-finite target is never chosen
    assert got[1] == (~sbad).sum()
    nan_src = np.full((40, 3), np.nan, np.float32)
    empty = np.zeros((0, 3), np.float32)
    for t, s, what in ((tg, nan_src, "all-NaN source"), (tg, empty, "empty source"), (empty, sr, "empty target"), (empty, empty, "both empty"),
                       (np.full((300, 3), np.nan, np.float32), sr, "all-NaN target")):
        score, used, idx, d2 = _one(seg, t, s, T)
        assert score == DBL_MAX and used == 0 and len(idx) == len(s) and (idx == -1).all() and (d2 == -1.0).all(), what


def test_max_range(seg):
    rng = np.random.default_rng(14)
    tg, sr = _cloud(rng, 257), _cloud(rng, 333)
    T = skew_T()
    _, _, ridx, rd2 = fitness_ref(tg, sr, T)
    order = np.argsort(rd2)
    d = float(rd2[order[100]])                                                   # one query's d2 as a double
    n_le, n_lt = int((rd2.astype(np.float64) <= d).sum()), int((rd2.astype(np.float64) < d).sum())
    assert n_le > n_lt >= 100
    at = _one(seg, tg, sr, T, d)
    below = _one(seg, tg, sr, T, float(np.nextafter(d, -np.inf)))
    assert at[1] == n_le and below[1] == n_lt                                    # accepted at the bound (<=), rejected just below it
    _check_pair(at, fitness_ref(tg, sr, T, d), "max_range == a d2")
    _check_pair(below, fitness_ref(tg, sr, T, float(np.nextafter(d, -np.inf))), "max_range just below")
    same = _one(seg, tg, tg, IDENTITY_T, 0.0)                                    # identical clouds, identity: every point at distance 0
    assert same[0] == 0.0 and same[1] == len(tg) and (same[3] == 0).all() and np.array_equal(same[2], np.arange(len(tg)))


def test_target_split_is_bitwise_the_unsplit_run(seg):
    rng = np.random.default_rng(15)
    T = skew_T()
    for nt, ns, chunk in ((700, 333, 256), (700, 1025, 256), (65, 129, 1), (700, 333, 100)):
        tg, sr = _cloud(rng, nt), _cloud(rng, ns)
        tg[5], tg[nt - 1] = np.nan, tg[3]                                        # a non-finite target and a duplicate across chunks
        whole = _with_chunk(1 << 20, lambda: _one(seg, tg, sr, T, 0.5))              # one chunk: no split
        auto = _one(seg, tg, sr, T, 0.5)                                         # the heuristic's own choice
        assert auto[0] == whole[0] and auto[1] == whole[1] and np.array_equal(auto[2], whole[2]) and auto[3].tobytes() == whole[3].tobytes()
        split = _with_chunk(chunk, lambda: _one(seg, tg, sr, T, 0.5))
        assert split[0] == whole[0] and split[1] == whole[1] and np.array_equal(split[2], whole[2]) and split[3].tobytes() == whole[3].tobytes()
        _check_pair(split, fitness_ref(tg, sr, T, 0.5), f"{nt} targets in chunks of {chunk}")


def test_batch_independence_and_repeatability(seg):
    rng = np.random.default_rng(16)
    clouds = [_cloud(rng, n) for n in (700, 333, 1025, 64)]
    Ta, Tb = skew_T(), skew_T(-0.4, (0.9, 0.1, -0.2), (-0.2, 0.3, 0.0))
    pairs = [(0, 1, Ta, None), (1, 0, Tb, 0.3), (2, 2, Ta, 0.05), (0, 3, Tb, None), (3, 2, Ta, 1.0), (1, 3, IDENTITY_T, 0.2)]   # cloud 1: target and source; cloud 2 against itself
    score, used, nn = seg.fitness_scores(clouds, pairs, return_nn=True)
    again = seg.fitness_scores(clouds, pairs, return_nn=True)
    assert score.tobytes() == again[0].tobytes() and np.array_equal(used, again[1])
    for k, (t, s, T, mr) in enumerate(pairs):
        alone = _one(seg, clouds[t], clouds[s], T, mr)
        assert alone[0] == score[k] and alone[1] == used[k], k
        assert np.array_equal(alone[2], nn[k][0]) and alone[3].tobytes() == nn[k][1].tobytes(), k
        assert np.array_equal(again[2][k][0], nn[k][0]) and again[2][k][1].tobytes() == nn[k][1].tobytes()
        _check_pair((float(score[k]), int(used[k]), nn[k][0], nn[k][1]), fitness_ref(clouds[t], clouds[s], T, mr), f"pair {k}")
    assert seg.last_fitness_ms > 0


def _raw(lib, seg, xyz, start, n_clouds, pairs, n_pairs, score, used):
    return lib.sslam_seg_fitness_scores(seg._h, None if xyz is None else xyz.ctypes.data, None if start is None else start.ctypes.data, n_clouds,
                                        None if pairs is None else C.cast(pairs, C.c_void_p), n_pairs,
                                        None if score is None else score.ctypes.data, None if used is None else used.ctypes.data, None, None, None)


def test_argument_errors(gpu_lib, seg):
    from semantic_slam_amd.segmentation import FitnessPair
    from semantic_slam_amd.synth import make_frame
    xyz = _cloud(np.random.default_rng(17), 90)
    start = np.array([0, 40, 90], np.int32)
    score, used = np.full(2, -7.0), np.full(2, -7, np.int32)

    def pairs(*ts):
        rec = (FitnessPair * len(ts))()
        for k, (t, s) in enumerate(ts):
            rec[k].target, rec[k].source, rec[k].max_range = t, s, DBL_MAX
            for q in range(12):
                rec[k].T[q] = IDENTITY_T[q]
        return rec

    good = pairs((0, 1), (1, 0))
    assert _raw(gpu_lib, seg, xyz, start, 2, good, 2, score, used) == 2 and (used == [50, 40]).all()
    assert _raw(gpu_lib, seg, xyz, start, 2, good, 0, None, None) == 0
    score[:], used[:] = -7.0, -7
    for bad in (pairs((0, 2)), pairs((2, 0)), pairs((-1, 0)), pairs((0, 1), (0, -1))):              # a cloud index out of range
        assert _raw(gpu_lib, seg, xyz, start, 2, bad, len(bad), score, used) == -1
    assert _raw(gpu_lib, seg, xyz, np.array([0, 50, 40], np.int32), 2, good, 2, score, used) == -1   # cloud_start decreases
    assert _raw(gpu_lib, seg, xyz, np.array([-1, 40, 90], np.int32), 2, good, 2, score, used) == -1  # ... or starts below 0
    assert _raw(gpu_lib, seg, xyz, start, 2, good, -1, score, used) == -1                            # n_pairs < 0
    assert _raw(gpu_lib, seg, xyz, start, -1, good, 2, score, used) == -1
    assert _raw(gpu_lib, seg, None, start, 2, good, 2, score, used) == -1                            # null required pointers
    assert _raw(gpu_lib, seg, xyz, None, 2, good, 2, score, used) == -1
    assert _raw(gpu_lib, seg, xyz, start, 2, None, 2, score, used) == -1
    assert _raw(gpu_lib, seg, xyz, start, 2, good, 2, None, used) == -1
    assert _raw(gpu_lib, seg, xyz, start, 2, good, 2, score, None) == -1
    assert gpu_lib.sslam_seg_fitness_scores(None, xyz.ctypes.data, start.ctypes.data, 2, C.cast(good, C.c_void_p), 2, score.ctypes.data,
                                            used.ctypes.data, None, None, None) == -1
    assert (score == -7.0).all() and (used == -7).all()                                               # nothing was written
    # the call refuses while a pipelined batch is in flight, and works again once it is collected
    f = make_frame(seed=3, n_boxes=2)
    seg.submit_frames([f])
    assert _raw(gpu_lib, seg, xyz, start, 2, good, 2, score, used) == -1 and b"in flight" in gpu_lib.sslam_last_error()
    seg.collect_frames()
    assert _raw(gpu_lib, seg, xyz, start, 2, good, 2, score, used) == 2


# ---- the tick ----------------------------------------------------------------------------------------------------------------------

def _tick_inputs():
    """five odometry poses 0.6 m apart with a little yaw, and the 96 x 72 golden patch (its NaNs included) seen from each of them"""
    world = np.load(os.path.join(GOLD, "patch96x72.npz"))["points"].astype(np.float64)
    rng = np.random.default_rng(18)
    odoms, frames = [], []
    for k in range(5):
        yaw = 0.03 * k
        q = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])
        t = np.array([0.6 * k, 0.05 * k, 0.0])
        R = np.array(qmat(q)).reshape(3, 3)
        local = ((world - t) @ R + rng.normal(0.0, 0.004, world.shape)).astype(np.float32)      # R^T (p - t), plus sensor noise
        odoms.append(np.concatenate([t, q]))
        frames.append(types.SimpleNamespace(cloud=np.ascontiguousarray(local).view(np.uint8).reshape(-1), width=96, height=72, point_step=12,
                                            row_step=96 * 12, offsets=(0, 4, 8), xyz=local))
    return odoms, frames


def _run_tick(seg, with_model, tmp_path, name):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    odoms, frames = _tick_inputs()
    S = SemanticGraphSLAM(default_slam_params(), segmentation=seg)
    if with_model:
        S.set_fitness_information(voxel_leaf=0.1)
    for k in range(5):
        if k != 2:                                                              # the keyframe in the middle has no cloud
            S.setPointCloudData(frames[k])
        assert S.VIOCallback((k, 0), odoms[k])
    assert S.run() and S.last_stats.keyframes_added == 5
    path = str(tmp_path / name)
    S.saveGraph(path)
    rows = [[float(v) for v in line.split()[1:]] for line in open(path) if line.startswith("EDGE_SE3:QUAT")]
    assert len(rows) == 4 and [(int(r[0]), int(r[1])) for r in rows] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    infos = []
    for r in rows:
        W = np.zeros((6, 6))
        W[np.triu_indices(6)] = r[9:30]
        infos.append(W + np.triu(W, 1).T)
    return S, frames, [np.array(r[2:9]) for r in rows], infos


def test_tick_information_from_fitness(seg, tmp_path):
    from semantic_slam_amd.segmentation import information_from_fitness
    const = np.diag([1.0 / 0.0667] * 6)
    S, frames, zs, infos = _run_tick(seg, True, tmp_path, "fitness.g2o")
    score, used = S.last_fitness()
    assert len(score) == 4
    ds = {k: seg.downsamplePointcloud(frames[k].xyz[np.isfinite(frames[k].xyz).all(1)], 0.1)[0] for k in (0, 1, 3, 4)}
    for e, (a, b) in enumerate(((0, 1), (1, 2), (2, 3), (3, 4))):
        if 2 in (a, b):                                                         # an edge touching the cloudless keyframe
            assert infos[e].tobytes() == const.tobytes() and score[e] == -1.0 and used[e] == -1
            continue
        T = np.concatenate([qmat(zs[e][3:]), zs[e][:3]])                        # of the measurement the row carries
        rscore, rused, _, _ = fitness_ref(ds[a], ds[b], T)
        lib_score, lib_used = seg.fitness_scores([ds[a], ds[b]], [(0, 1, T, None)])
        print(f"edge {a}-{b}: {len(ds[a])} x {len(ds[b])} voxels, score {score[e]:.17g} ref {rscore:.17g}, used {used[e]}, "
              f"information {infos[e][0, 0]:.6g} / {infos[e][3, 3]:.6g}")
        assert 50 < rused == used[e] == lib_used[0] and len(ds[b]) == rused
        assert score[e] == lib_score[0] and abs(score[e] - rscore) <= rused * 2.0 ** -52 * rscore
        assert 0 < rscore < DBL_MAX
        assert infos[e].tobytes() == information_from_fitness(rscore).tobytes() == information_ref(rscore).tobytes()
        assert infos[e].tobytes() != const.tobytes()
    # the same inputs without the setter: the constant matrix on every edge, as before
    S0, _, zs0, infos0 = _run_tick(seg, False, tmp_path, "constant.g2o")
    assert all(w.tobytes() == const.tobytes() for w in infos0) and all(np.array_equal(a, b) for a, b in zip(zs, zs0))
    assert len(S0.last_fitness()[0]) == 0


def test_tick_keeps_the_last_cloud_for_the_next_tick(seg):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    odoms, frames = _tick_inputs()
    S = SemanticGraphSLAM(default_slam_params(), segmentation=seg)
    S.set_fitness_information()
    whole = SemanticGraphSLAM(default_slam_params(), segmentation=seg)
    whole.set_fitness_information()
    for k in range(4):
        for X in (S, whole):
            X.setPointCloudData(frames[k])
            assert X.VIOCallback((k, 0), odoms[k])
        if k == 1:
            assert S.run() and len(S.last_fitness()[0]) == 1
    assert S.run() and whole.run()
    two, one = S.last_fitness(), whole.last_fitness()                           # edges 1-2, 2-3 against edges 0-1, 1-2, 2-3
    assert len(two[0]) == 2 and len(one[0]) == 3
    assert two[0].tobytes() == one[0][1:].tobytes() and np.array_equal(two[1], one[1][1:]) and (two[1] > 50).all()
    # without a frontend handle the model cannot run
    from semantic_slam_amd import SslamError
    N = SemanticGraphSLAM(default_slam_params())
    N.set_fitness_information()
    for k in range(2):
        N.setPointCloudData(frames[k])
        assert N.VIOCallback((k, 0), odoms[k])
    with pytest.raises(SslamError) as ei:
        N.run()
    assert ei.value.code == -1


# ---- the C++ shim -------------------------------------------------------------------------------------------------------------------

def _shim_clouds():
    """the clouds and the pose of tests/shim_information_check.cpp: keep the two in step"""
    i = np.arange(300)
    c1 = np.stack([np.float32(0.125) * (i % 20).astype(np.float32), np.float32(0.25) * (i // 20).astype(np.float32),
                   np.float32(0.0625) * ((i * 7) % 11).astype(np.float32)], 1)
    i = np.arange(130)
    c2 = np.stack([np.float32(0.1875) * (i % 13).astype(np.float32) + np.float32(0.03125), np.float32(0.375) * (i // 13).astype(np.float32),
                   np.float32(0.09375) * ((i * 5) % 7).astype(np.float32)], 1)
    c2[17, 1] = np.nan
    c, s = 0.9950041652780258, 0.09983341664682815
    return c1.astype(np.float32), c2.astype(np.float32), np.array([c, -s, 0, s, c, 0, 0, 0, 1, 0.05, -0.02, 0.01])


def test_cpp_shim_information_end_to_end(seg, tmp_path):
    from semantic_slam_amd import library_path
    from semantic_slam_amd.segmentation import information_from_fitness
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_information")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_information_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"shim information ok: score (\S+) info((?: \S+){36})", out.stdout)
    assert m, out.stdout
    c1, c2, T = _shim_clouds()
    score, used = seg.fitness_scores([c1, c2], [(0, 1, T, 0.04), (0, 1, T, None)])
    assert 0 < used[0] < used[1] == 129
    _check_pair((float(score[0]), int(used[0])) + _one(seg, c1, c2, T, 0.04)[2:], fitness_ref(c1, c2, T, 0.04), "shim clouds")
    print("shim", m.group(1), "mirror", repr(float(score[0])))
    assert float(m.group(1)) == score[0]
    assert np.array([float(v) for v in m.group(2).split()]).tobytes() == information_from_fitness(float(score[1])).tobytes()
