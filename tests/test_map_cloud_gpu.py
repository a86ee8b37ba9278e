"""The map cloud on the GPU: sslam_seg_map_cloud against tests/map_ref.py's NumPy restatement of its contract, and sslam_slam_map_cloud
(the tick keeping its keyframe clouds on the device) against the same call fed by hand.

Every comparison is exact: np.array_equal on cells and counts, equal bytes of the centroids.  The contract fixes every operation in
float32 / int64 / float64 without fused multiply-add and with order-independent integer sums, so nothing is left to a tolerance;
tests/test_map_cloud_cpu.py shows on the reference alone that the cases bite.  ONE exception, beyond what the contract asks of the shim:
the tick part of test_cpp_shim_map compares the C++ shim's replay with the Python mirror's.  The shim's VIOCallback takes the odometry
as a matrix and the mirror's as a quaternion, so the two poses differ in their last bits before they reach the library; that comparison
takes the cloud count exactly, the voxel count to 1 % and the first centroid to 1e-5.  The shim's generate part is exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loop_ref as LR
import loop_scene as LS
import map_ref as MR
from fitness_ref import qmat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    return PointCloudSegmentation()


def _same(got, want, what=""):
    xyz, counts, cells = got[:3]
    wx, wc, wk = want[:3]
    assert np.array_equal(cells, wk), what
    assert np.array_equal(counts, wc), what
    assert xyz.dtype == np.float32 and xyz.tobytes() == wx.tobytes(), what


def _stats_match(st, ref):
    assert (st.n_clouds, st.n_points, st.n_used, st.n_bricks, st.n_voxels) == \
           (ref["n_clouds"], ref["n_points"], ref["n_used"], ref["n_bricks"], ref["n_voxels"])


@pytest.fixture(scope="module")
def lattice():
    clouds, poses = MR.lattice_case()
    return clouds, poses, {m: MR.map_ref(clouds, poses, MR.LATTICE_RESOLUTION, m) for m in (1, 2, 4)}


def _lattice_passes(seg, lattice):
    clouds, poses, ref = lattice
    for m in (1, 2, 4):
        xyz, counts, cells, st = seg.map_cloud(clouds, poses, MR.LATTICE_RESOLUTION, m, return_cells=True)
        _same((xyz, counts, cells), ref[m], "min_points %d" % m)
        _stats_match(st, ref[m][3])
        assert seg.last_map_count == len(ref[m][1])
        assert st.upload_bytes == 12 * st.n_points + 48 * st.n_clouds + 4 * (st.n_clouds + 1)
        assert st.kernel_ms > 0 and abs(seg.last_map_timing().sum() - st.kernel_ms) <= 1e-9 * st.kernel_ms


# 1
def test_lattice(seg, lattice):
    _lattice_passes(seg, lattice)
    # no clouds, and clouds without a usable point: 0
    assert len(seg.map_cloud([], [], 0.25)[0]) == 0
    clouds, poses, _ = lattice
    xyz, counts, st = seg.map_cloud(clouds[-1:], poses[-1:], 0.25)
    assert len(xyz) == 0 and (st.n_points, st.n_used, st.n_voxels) == (len(clouds[-1]), 0, 0)
    assert len(seg.map_cloud(clouds[:1], poses[:1], 0.25)[0]) == 0             # one cloud, no points


# 2
@pytest.mark.parametrize("resolution", [0.05, 0.1, 0.37])
def test_generic(seg, resolution):
    clouds, poses = MR.generic_case()
    ref = MR.map_ref(clouds, poses, resolution)
    xyz, counts, cells, st = seg.map_cloud(clouds, poses, resolution, return_cells=True)
    _same((xyz, counts, cells), ref)
    _stats_match(st, ref[3])
    print("resolution", resolution, st, "passes ms", seg.last_map_timing())


# 3
def test_shared_voxel(seg):
    clouds, poses = MR.shared_voxel_case()
    ref = MR.map_ref(clouds, poses, MR.SHARED_RESOLUTION)
    xyz, counts, cells, st = seg.map_cloud(clouds, poses, MR.SHARED_RESOLUTION, return_cells=True)
    assert counts.tolist() == [60000] and cells.tolist() == [list(MR.SHARED_CELL)]
    _same((xyz, counts, cells), ref)
    _stats_match(st, ref[3])
    # min_points above and at the count
    assert len(seg.map_cloud(clouds, poses, MR.SHARED_RESOLUTION, 60001)[0]) == 0
    assert seg.map_cloud(clouds, poses, MR.SHARED_RESOLUTION, 60000)[1].tolist() == [60000]


# 4
def test_permuted_and_split_clouds(seg):
    clouds, poses = MR.generic_case(seed=5, n_clouds=12)
    full = seg.map_cloud(clouds, poses, 0.1, return_cells=True)
    _same(full, MR.map_ref(clouds, poses, 0.1))
    perm = np.random.default_rng(0).permutation(len(clouds))
    assert not np.array_equal(perm, np.arange(len(clouds)))
    _same(seg.map_cloud([clouds[k] for k in perm], [poses[k] for k in perm], 0.1, return_cells=True), full, "permuted")
    # the points of a cloud reversed, and a cloud cut into two clouds with the same pose
    cut = [clouds[0][:100], clouds[0][100:]] + [c[::-1] for c in clouds[1:]]
    _same(seg.map_cloud(cut, [poses[0]] + list(poses), 0.1, return_cells=True), full, "cut and reversed")
    # two calls over the two halves: cells are global, so the same cell means the same place, and the counts add up to the full map's
    half = len(clouds) // 2
    merged = {}
    for part in (slice(0, half), slice(half, None)):
        xyz, counts, cells, st = seg.map_cloud(clouds[part], poses[part], 0.1, return_cells=True)
        _same((xyz, counts, cells), MR.map_ref(clouds[part], poses[part], 0.1))
        for cell, n in zip(map(tuple, cells.tolist()), counts.tolist()):
            merged[cell] = merged.get(cell, 0) + n
    assert merged == dict(zip(map(tuple, full[2].tolist()), full[1].tolist()))


# 5
def test_max_out_below_the_count(seg, lattice):
    clouds, poses, ref = lattice
    total = len(ref[1][1])
    for cap in (0, 1, 257, total - 1, total, total + 5):
        xyz, counts, cells, st = seg.map_cloud(clouds, poses, MR.LATTICE_RESOLUTION, return_cells=True, max_out=cap)
        assert seg.last_map_count == total and len(xyz) == len(counts) == len(cells) == min(cap, total)
        _same((xyz, counts, cells), tuple(a[:cap] for a in ref[1][:3]), "max_out %d" % cap)
    # exactly max_out records are written: the rows behind them keep what the caller put there
    lib, cl = seg._lib, [np.ascontiguousarray(c, np.float32) for c in clouds]
    start = np.zeros(len(cl) + 1, np.int32); start[1:] = np.cumsum([len(c) for c in cl])
    pts, T = np.concatenate(cl), np.ascontiguousarray(poses, np.float64)
    out = np.full((10, 3), 7.5, np.float32); cnt = np.full(10, -3, np.int32); cel = np.full((10, 3), -9, np.int32)
    rc = lib.sslam_seg_map_cloud(seg._h, pts.ctypes.data, start.ctypes.data, len(cl), T.ctypes.data, C.c_float(MR.LATTICE_RESOLUTION), 1,
                                 out.ctypes.data, cel.ctypes.data, cnt.ctypes.data, 6, None)
    assert rc == total
    assert out[:6].tobytes() == ref[1][0][:6].tobytes() and (out[6:] == 7.5).all() and (cnt[6:] == -3).all() and (cel[6:] == -9).all()
    # max_out = 0 with a NULL xyz_out
    assert lib.sslam_seg_map_cloud(seg._h, pts.ctypes.data, start.ctypes.data, len(cl), T.ctypes.data, C.c_float(MR.LATTICE_RESOLUTION), 1,
                                   None, None, None, 0, None) == total


# 6
def test_limits(seg, lattice):
    from semantic_slam_amd import SslamError
    clouds, poses = MR.far_case()
    with pytest.raises(SslamError) as ei:                                      # more than 2^26 bricks in the box
        seg.map_cloud(clouds, poses, 0.001)
    assert ei.value.code == MR.UNSUPPORTED and "bricks" in str(ei.value)
    _lattice_passes(seg, lattice)
    assert len(seg.map_cloud(clouds, poses, 1.0)[0]) == 2                      # the same two points at a resolution that fits
    I = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    with pytest.raises(SslamError) as ei:                                      # a cell index that does not fit 32 bits
        seg.map_cloud([np.array([[0, 0, 0], [1e30, 0, 0]], np.float32)], [I], 0.1)
    assert ei.value.code == MR.UNSUPPORTED and "32 bits" in str(ei.value)
    _lattice_passes(seg, lattice)
    # a point times a pose that overflows to inf is skipped, not an error
    big = I.copy(); big[0] = 1e30
    pts = np.array([[1e30, 0.5, 0.5], [0.0, 0.5, 0.5]], np.float32)            # 1e30 * 1e30 overflows float32; 0 * 1e30 does not
    xyz, counts, cells, st = seg.map_cloud([pts], [big], 0.25, return_cells=True)
    _same((xyz, counts, cells), MR.map_ref([pts], [big], 0.25))
    assert (st.n_points, st.n_used) == (2, 1) and counts.tolist() == [1]
    _lattice_passes(seg, lattice)


# 7
def test_repeats(gpu_lib, seg):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    clouds, poses = MR.generic_case(seed=7, n_clouds=10)
    a = seg.map_cloud(clouds, poses, 0.1, 2, return_cells=True)
    b = seg.map_cloud(clouds, poses, 0.1, 2, return_cells=True)
    c = PointCloudSegmentation().map_cloud(clouds, poses, 0.1, 2, return_cells=True)
    _same(b, a, "same handle")
    _same(c, a, "second handle")
    assert len(a[0]) > 100


# 8
def _loop_struct():
    from semantic_slam_amd.semantic_graph_slam import default_loop_params
    p = default_loop_params()
    for k, v in LS.LOOP_KW.items():
        if k == "inf":
            for (f, _), x in zip(p.inf._fields_, v):
                setattr(p.inf, f, x)
        else:
            setattr(p, k, v)
    return p


def _product(seg, map_on):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    p = default_slam_params()
    p.const_stddev_x, p.const_stddev_q = LS.ODOM_STDDEV_X, LS.ODOM_STDDEV_Q
    S = SemanticGraphSLAM(p, seg)
    S.set_loop_closure(_loop_struct())
    if map_on:
        S.set_map_clouds(True, 0.3)
    return S


def test_tick_keeps_map_clouds(seg):
    events = LS.make_events()
    on, off = _product(seg, True), _product(seg, False)
    kept = []                                                                  # the downsampled cloud of every processed keyframe
    pending = []
    first_check = 32                                                           # events before the upload accounting is looked at
    loops = 0
    for k, ev in enumerate(events):
        for S in (on, off):
            S.setPointCloudData(ev.cloud)
            assert S.VIOCallback(ev.stamp, ev.odom)                            # every sample of the scene is a keyframe
        P = ev.cloud.xyz()
        pending.append(seg.downsamplePointcloud(P[np.isfinite(P).all(1)], 0.3)[0])
        if not ev.run_after:
            continue
        assert on.run() and off.run()
        loops += sum(L.outcome == LR.ADDED for L in on.last_loops())
        # the switch does not touch the tick: estimates and chi2 bit for bit
        (ia, ea), (ib, eb) = on.getKeyframes(), off.getKeyframes()
        assert ia.tobytes() == ib.tobytes() and ea.tobytes() == eb.tobytes()
        assert np.float64(on.last_stats.opt.chi2_after).tobytes() == np.float64(off.last_stats.opt.chi2_after).tobytes()
        new, pending = pending, []
        kept += new
        if k + 1 == first_check:
            first = on.map_cloud(0.2)
            assert first[5].upload_bytes == 12 * sum(len(c) for c in kept) + 48 * len(kept)
            again = on.map_cloud(0.2)                                          # no keyframe in between: only the poses travel
            assert again[5].upload_bytes == 48 * len(kept) == 48 * again[5].n_clouds
            _same(again, first)
        elif k + 1 == first_check + LS.RUN_EVERY:                              # one more tick: the new clouds once, and the poses
            st = on.map_cloud(0.2)[5]
            assert len(new) == LS.RUN_EVERY and st.n_clouds == len(kept)
            assert st.upload_bytes == 12 * sum(len(c) for c in new) + 48 * len(kept)
    assert loops >= 3 and len(kept) > first_check + LS.RUN_EVERY               # the estimates the map is built at did move
    xyz, counts, cells, ids, poses, st = on.map_cloud(0.2)
    kf_ids, est = on.getKeyframes()
    assert np.array_equal(ids, kf_ids) and len(ids) == len(kept) == st.n_clouds
    want = np.array([list(qmat(LR.from_tq(e)[1])) + list(LR.from_tq(e)[0]) for e in est])
    assert np.abs(poses - want).max() <= 1e-12
    pred = seg.map_cloud(kept, poses, 0.2, return_cells=True)
    _same((xyz, counts, cells), pred)
    assert (st.n_points, st.n_used, st.n_voxels) == (pred[3].n_points, pred[3].n_used, pred[3].n_voxels) and st.n_voxels == len(xyz) > 1000
    _same((xyz, counts, cells), MR.map_ref(kept, poses, 0.2))
    # min_points through the tick's call
    m3 = on.map_cloud(0.2, 3)
    _same(m3, MR.map_ref(kept, poses, 0.2, 3))
    assert 0 < len(m3[0]) < len(xyz)
    # off: nothing kept, 0
    o = off.map_cloud(0.2)
    assert len(o[0]) == 0 and o[5].n_clouds == 0 and o[5].upload_bytes == 0
    on.set_map_clouds(False)                                                   # turning it off drops what was kept
    assert len(on.map_cloud(0.2)[0]) == 0


def test_tick_downsamples_at_its_own_leaf(seg):
    """loop closure off, then on with another leaf: the map clouds are downsampled by the tick itself at keyframe_leaf (with equal leaves,
    as in the test above, the loop stage's cloud is shared instead)"""
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    events = LS.make_events(12)
    for loop_leaf in (None, 0.3):
        S = SemanticGraphSLAM(None, seg)
        if loop_leaf is not None:
            p = _loop_struct()
            p.voxel_leaf = loop_leaf
            S.set_loop_closure(p)
        S.set_map_clouds(True, 0.25)
        kept = []
        for ev in events:
            S.setPointCloudData(ev.cloud)
            assert S.VIOCallback(ev.stamp, ev.odom)
            P = ev.cloud.xyz()
            kept.append(seg.downsamplePointcloud(P[np.isfinite(P).all(1)], 0.25)[0])
            if ev.run_after:
                assert S.run()
        xyz, counts, cells, ids, poses, st = S.map_cloud(0.2)
        assert len(ids) == len(kept) == 12 and st.n_points == sum(len(c) for c in kept)
        assert st.upload_bytes == 12 * st.n_points + 48 * 12
        wrong = [seg.downsamplePointcloud(ev.cloud.xyz(), 0.3)[0] for ev in events]
        assert sum(len(c) for c in wrong) != st.n_points                      # the loop stage's leaf would give other clouds
        _same((xyz, counts, cells), seg.map_cloud(kept, poses, 0.2, return_cells=True), "loop leaf %s" % loop_leaf)
        _same((xyz, counts, cells), MR.map_ref(kept, poses, 0.2))


# 9
def _shim_input():
    """what tests/shim_map_check.cpp builds: keep the two in step"""
    clouds, poses = [], []
    for c in range(3):
        i = np.arange(200 + 50 * c)
        clouds.append(np.stack([0.125 * (i % 16) - 1.0, 0.0625 * (i // 16) + 0.5 * c, 0.03125 * ((i * 7) % 13)], 1).astype(np.float32))
        R = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])][c]
        poses.append(np.concatenate([R.reshape(-1), [0.25 * c, -0.5 * c, 0.125]]))
    return clouds, poses


def test_cpp_shim_map(gpu_lib, seg, tmp_path):
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_map")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_map_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    events = LS.make_events(8)
    rec = str(tmp_path / "replay.bin")
    with open(rec, "wb") as f:
        for ev in events:
            f.write(np.array([ev.stamp[0], ev.stamp[1], int(ev.run_after)], np.int32).tobytes())
            f.write(np.asarray(ev.odom, np.float64).tobytes())
            f.write(ev.cloud.cloud.tobytes())
    out = subprocess.run([exe, rec], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    g = re.search(r"shim map generate: voxels (\d+) first (\S+) (\S+) (\S+) count (\d+)", out.stdout)
    t = re.search(r"shim map tick: clouds (\d+) voxels (\d+) first (\S+) (\S+) (\S+)", out.stdout)
    assert g and t and "shim map ok" in out.stdout, out.stdout
    clouds, poses = _shim_input()
    xyz, counts, st = seg.map_cloud(clouds, poses, 0.25)
    assert int(g.group(1)) == len(xyz) > 10 and int(g.group(5)) == counts[0]
    assert np.array([float(g.group(k)) for k in (2, 3, 4)], np.float32).tobytes() == xyz[0].tobytes()
    # the tick through the shim: the same replay through the Python mirror.  The shim hands the odometry over as a matrix, so its
    # quaternions may differ from the mirror's in the last bits: the count of clouds exactly, the first centroid to 1e-5
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    S = SemanticGraphSLAM(None, seg)
    S.set_map_clouds(True, 0.3)
    for ev in events:
        S.setPointCloudData(ev.cloud)
        S.VIOCallback(ev.stamp, ev.odom)
        if ev.run_after:
            assert S.run()
    mx, mc, mk, ids, mp, mst = S.map_cloud(0.2)
    assert int(t.group(1)) == len(ids) == 8 and abs(int(t.group(2)) - len(mx)) <= 0.01 * len(mx)
    print("shim", t.groups(), "mirror", len(mx), mx[0])
    assert np.abs(np.array([float(t.group(k)) for k in (3, 4, 5)]) - mx[0]).max() <= 1e-5
