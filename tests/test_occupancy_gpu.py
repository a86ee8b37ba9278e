"""The occupancy map on the GPU: sslam_seg_occupancy_map against tests/occupancy_ref.py's restatement of its contract, and
sslam_slam_occupancy_map (the tick's resident keyframe clouds) against the same call fed by hand.

Every comparison is exact: cells, hits and misses by np.array_equal, the log-odds by their bytes.  The contract fixes every operation --
float32 without fused multiply-add up to the sub-cell position, integers from there, integer atomics -- so nothing is left to a
tolerance; tests/test_occupancy_cpu.py shows on the reference alone that the traversal is the exact one and that the cases bite."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loop_scene as LS
import occupancy_ref as OR
from fitness_ref import qmat
import loop_ref as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg(gpu_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    return PointCloudSegmentation()


def _struct(P):
    """the reference's parameter dict as sslam_occ_params: the same floats on both sides"""
    from semantic_slam_amd._lib import OccParams
    p = OccParams()
    for k, v in P.items():
        if k == "sensor_origin":
            p.sensor_origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, int(v) if k == "emit" else float(v))
    return p


def _same(got, want, what=""):
    for k, name in enumerate(("cells", "hits", "misses")):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, name)
    assert got[3].dtype == np.float32 and got[3].tobytes() == want[3].tobytes(), (what, "logodds")


def _stats_match(st, ref):
    for k, v in ref.items():
        assert getattr(st, k) == v, (k, getattr(st, k), v)


@pytest.fixture(scope="module")
def lattice():
    clouds, poses = OR.lattice_case()
    P = OR.lattice_params()
    return clouds, poses, P, {e: OR.occupancy_ref(clouds, poses, dict(P, emit=e)) for e in (0, 1, 2)}


def _lattice_passes(seg, lattice):
    clouds, poses, P, ref = lattice
    got = seg.occupancy_map(clouds, poses, _struct(P))
    _same(got, ref[0], "lattice")
    _stats_match(got[4], ref[0][4])
    return got


def _raw(seg, clouds, poses, p, cells=None, hits=None, misses=None, lo=None, max_out=0, stats=None, start=None, T=None, n_clouds=None):
    from semantic_slam_amd.segmentation import pack_clouds
    xyz, st, TT = pack_clouds(clouds, poses)
    start = st if start is None else start
    T = TT if T is None else T
    ptr = lambda a: None if a is None else a.ctypes.data
    return seg._lib.sslam_seg_occupancy_map(seg._h, ptr(xyz) if len(xyz) else None, ptr(start), len(clouds) if n_clouds is None else n_clouds, ptr(T),
                                            None if p is None else C.byref(p), ptr(cells), ptr(hits), ptr(misses), ptr(lo), max_out,
                                            None if stats is None else C.byref(stats))


# 1
def test_lattice(seg, lattice):
    got = _lattice_passes(seg, lattice)
    st = got[4]
    assert st.upload_bytes == 12 * st.n_points + 48 * st.n_clouds + 4 * (st.n_clouds + 1)
    assert st.kernel_ms > 0 and abs(seg.last_occupancy_timing().sum() - st.kernel_ms) <= 1e-9 * st.kernel_ms
    assert st.n_steps == int(got[1].sum()) + int(got[2].sum()) and seg.last_occupancy_count == len(got[0])
    _same(seg.occupancy_map(lattice[0], lattice[1], _struct(lattice[2])), got, "repeated call")


# 2
@pytest.mark.parametrize("resolution", [0.05, 0.1, 0.37])
def test_generic(seg, resolution):
    clouds, poses, max_range = OR.generic_case()
    P = OR.default_params(resolution=resolution, max_range=max_range, sensor_origin=OR.GENERIC_ORIGIN)
    ref = OR.occupancy_ref(clouds, poses, P)
    got = seg.occupancy_map(clouds, poses, _struct(P))
    _same(got, ref)
    _stats_match(got[4], ref[4])
    assert 0.1 * got[4].n_rays < got[4].n_truncated < 0.3 * got[4].n_rays
    print("resolution", resolution, got[4], "passes ms", seg.last_occupancy_timing())


# 3
def test_hits_are_the_map_cloud(seg):
    """max_range beyond every point and an open z range: the records with hits are the voxels of sslam_seg_map_cloud, with its counts"""
    clouds, poses, _ = OR.generic_case(seed=3)
    P = OR.default_params(resolution=0.1, max_range=50.0, z_min=-np.inf, z_max=np.inf, sensor_origin=OR.GENERIC_ORIGIN)
    cells, hits, misses, lo, st = seg.occupancy_map(clouds, poses, _struct(P))
    assert st.n_truncated == 0 and st.n_clipped_z == 0 and st.n_rays == st.n_points
    xyz, counts, mcells, mst = seg.map_cloud(clouds, poses, 0.1, 1, return_cells=True)
    assert np.array_equal(cells[hits > 0], mcells) and np.array_equal(hits[hits > 0], counts) and int(hits.sum()) == mst.n_used
    _same((cells, hits, misses, lo), OR.occupancy_ref(clouds, poses, P))


# 4
def test_order_independence(seg):
    clouds, poses, max_range = OR.generic_case(seed=5)
    p = _struct(OR.default_params(resolution=0.1, max_range=max_range, sensor_origin=OR.GENERIC_ORIGIN))
    full = seg.occupancy_map(clouds, poses, p)
    perm = [2, 0, 3, 1]
    _same(seg.occupancy_map([clouds[k] for k in perm], [poses[k] for k in perm], p), full, "clouds permuted")
    rng = np.random.default_rng(0)
    _same(seg.occupancy_map([c[rng.permutation(len(c))] for c in clouds], poses, p), full, "points permuted")
    cut = [clouds[0][:100], clouds[0][100:]] + list(clouds[1:])
    _same(seg.occupancy_map(cut, [poses[0]] + list(poses), p), full, "one cloud split in two")
    _same(seg.occupancy_map(clouds, poses, p), full, "repeated")
    assert len(full[0]) > 1000


# 5
def test_non_finite_rows_and_empty_clouds(seg, lattice):
    clouds, poses, P, _ = lattice
    bad = [c.copy() for c in clouds[:3]]
    bad[0][5] = (np.nan, 0, 0); bad[0][62] = (0, np.inf, 0); bad[2][63] = (0, 0, -np.inf); bad[2][64] = (np.nan, np.nan, np.nan)
    cl = [bad[0], np.zeros((0, 3), np.float32), bad[1], bad[2], np.full((7, 3), np.nan, np.float32)]
    ps = [poses[0], poses[1], poses[1], poses[2], poses[3]]
    ref = OR.occupancy_ref(cl, ps, P)
    got = seg.occupancy_map(cl, ps, _struct(P))
    _same(got, ref)
    _stats_match(got[4], ref[4])
    assert got[4].n_points - got[4].n_rays - got[4].n_clipped_z == 4 + 7
    # a point times a pose that overflows to inf is skipped; so is a cloud whose ray origin overflows
    big = OR.identity_pose(); big[0] = 1e30
    pts = np.array([[1e30, 0.5, 0.5], [0.0, 0.5, 0.5]], np.float32)            # 1e30 * 1e30 overflows float32; 0 * 1e30 does not
    Q = dict(P, sensor_origin=np.zeros(3, np.float32))
    got = seg.occupancy_map([pts], [big], _struct(Q))
    _same(got, OR.occupancy_ref([pts], [big], Q))
    assert (got[4].n_points, got[4].n_rays) == (2, 1) and int(got[1].sum()) == 1
    Q = dict(P, sensor_origin=np.array([1e30, 0, 0], np.float32))
    got = seg.occupancy_map([pts], [big], _struct(Q))
    _same(got, OR.occupancy_ref([pts], [big], Q))
    assert got[4].n_rays == 0 and got[4].n_clipped_z == 0
    # no clouds, clouds without points
    st = seg.occupancy_map([], [], _struct(P))[4]
    assert (st.n_clouds, st.n_points, st.n_cells) == (0, 0, 0) and seg.last_occupancy_count == 0
    assert len(seg.occupancy_map(cl[1:2], ps[1:2], _struct(P))[0]) == 0
    _lattice_passes(seg, lattice)


# 6
def test_emit_modes_and_max_out(seg, lattice):
    from semantic_slam_amd._lib import OccStats
    clouds, poses, P, ref = lattice
    got = {e: seg.occupancy_map(clouds, poses, _struct(dict(P, emit=e))) for e in (0, 1, 2)}
    for e in (0, 1, 2):
        _same(got[e], ref[e], "emit %d" % e)
        _stats_match(got[e][4], ref[e][4])                                     # n_cells counts before emit in every mode
    assert len(got[1][0]) > 0 and len(got[2][0]) > 0 and len(got[1][0]) + len(got[2][0]) == len(got[0][0])
    assert (got[1][3] >= P["l_occ"]).all() and (got[2][3] < P["l_occ"]).all()
    both = np.concatenate([got[1][0], got[2][0]])
    assert len(np.unique(both, axis=0)) == len(both) == len(got[0][0])
    # max_out below the count: the true count is returned and the prefix is written; the rows behind it keep what the caller put there
    total = len(ref[0][0])
    p = _struct(P)
    for cap in (0, 1, 257, total - 1, total + 5):
        cells = np.full((total + 9, 3), -9, np.int32); hits = np.full(total + 9, -3, np.int32); misses = np.full(total + 9, -4, np.int32)
        lo = np.full(total + 9, 7.5, np.float32)
        assert _raw(seg, clouds, poses, p, cells, hits, misses, lo, cap) == total
        m = min(cap, total)
        _same((cells[:m], hits[:m], misses[:m], lo[:m]), tuple(a[:m] for a in ref[0][:4]), "max_out %d" % cap)
        assert (cells[m:] == -9).all() and (hits[m:] == -3).all() and (misses[m:] == -4).all() and (lo[m:] == 7.5).all()
    # every optional output pointer NULL, one at a time and all at once
    st = OccStats()
    assert _raw(seg, clouds, poses, p, None, None, None, None, total, st) == total and st.n_cells == total
    hits = np.zeros(total, np.int32)
    assert _raw(seg, clouds, poses, p, None, hits, None, None, total, None) == total and np.array_equal(hits, ref[0][1])
    lo = np.zeros(total, np.float32)
    assert _raw(seg, clouds, poses, p, None, None, None, lo, total, None) == total and lo.tobytes() == ref[0][3].tobytes()


# 7
def test_error_returns(gpu_lib, seg, lattice):
    from semantic_slam_amd import SslamError
    from semantic_slam_amd.synth import make_frame
    clouds, poses, P, _ = lattice
    clouds, poses = clouds[:2], poses[:2]
    bad = [dict(resolution=0.0), dict(resolution=-0.1), dict(resolution=np.nan), dict(resolution=np.inf), dict(resolution=1e-45),
           dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.nan), dict(max_range=np.inf),
           dict(max_range=128.5),                                              # R = 128.5 * 8 * 1024 > 2^20
           dict(max_range=1e-5),                                               # R = 0
           dict(l_hit=0.0), dict(l_hit=-0.5), dict(l_miss=0.0), dict(l_miss=0.5), dict(l_hit=np.nan), dict(l_miss=np.nan),
           dict(l_min=1.0, l_max=0.5), dict(z_min=1.0, z_max=0.5), dict(l_min=np.nan), dict(z_max=np.nan), dict(l_occ=np.nan),
           dict(emit=3), dict(emit=-1), dict(sensor_origin=(0, np.nan, 0))]
    for kw in bad:
        assert _raw(seg, clouds, poses, _struct(dict(P, **{k: (np.asarray(v, np.float32) if k == "sensor_origin" else v) for k, v in kw.items()}))) == OR.INVALID, kw
    p = _struct(P)
    assert _raw(seg, clouds, poses, _struct(dict(P, max_range=128.0))) > 0    # R = 2^20 exactly is allowed
    assert _raw(seg, clouds, poses, None) == OR.INVALID
    assert _raw(seg, clouds, poses, p, max_out=-1) == OR.INVALID
    assert _raw(seg, clouds, poses, p, n_clouds=-1) == OR.INVALID
    assert _raw(seg, clouds, poses, p, start=np.array([0, 63, 62], np.int32)) == OR.INVALID and b"decreases" in gpu_lib.sslam_last_error()
    assert _raw(seg, clouds, poses, p, start=np.array([-1, 63, 127], np.int32)) == OR.INVALID
    T = np.ascontiguousarray(poses, np.float64).copy(); T[1, 10] = np.nan
    assert _raw(seg, clouds, poses, p, T=T) == OR.INVALID and b"not finite" in gpu_lib.sslam_last_error()
    assert gpu_lib.sslam_seg_occupancy_map(None, None, None, 0, None, C.byref(p), None, None, None, None, 0, None) == OR.INVALID
    # the limits: two points 3000 m apart at resolution 0.01 -- the brick grid fails before any table is sized
    fc, fp = OR.far_case()
    with pytest.raises(SslamError) as ei:
        seg.occupancy_map(fc, fp, _struct(OR.default_params(resolution=0.01, max_range=10.0)))
    assert ei.value.code == OR.UNSUPPORTED and "bricks" in str(ei.value)
    assert len(seg.occupancy_map(fc, fp, _struct(OR.default_params(resolution=0.5, max_range=10.0)))[0]) > 2   # the same at a resolution that fits
    with pytest.raises(SslamError) as ei:                                      # a ray beyond 2^19 cells
        seg.occupancy_map([np.array([[30000.0, 0, 0]], np.float32)], fp[:1], _struct(OR.default_params()))
    assert ei.value.code == OR.UNSUPPORTED and "2^19" in str(ei.value)
    _lattice_passes(seg, lattice)
    # a batch in flight
    seg.submit_frames([make_frame(seed=3, n_boxes=2)])
    assert _raw(seg, clouds, poses, p) == OR.INVALID and b"in flight" in gpu_lib.sslam_last_error()
    seg.collect_frames()
    _lattice_passes(seg, lattice)


def test_tiny_negative_coordinate(seg):
    """u - floorf(u) rounds to 1 for a tiny negative u: the sub-cell position stays at 1023"""
    pts = np.array([[-1e-9, 0.3, 0.2], [0.4, -1e-9, 0.2], [-0.5, -0.7, -1e-9]], np.float32)
    P = OR.default_params(resolution=0.125, sensor_origin=(-1e-9, -1e-9, 0.25))
    got = seg.occupancy_map([pts], [OR.identity_pose()], _struct(P))
    _same(got, OR.occupancy_ref([pts], [OR.identity_pose()], P))
    assert got[4].n_rays == 3


# 8
def _product(seg):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    p = default_slam_params()
    p.const_stddev_x, p.const_stddev_q = LS.ODOM_STDDEV_X, LS.ODOM_STDDEV_Q
    S = SemanticGraphSLAM(p, seg)
    S.set_map_clouds(True, 0.3)
    return S


def test_tick(seg):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, occupancy_default_params
    events = LS.make_events(16)
    S = _product(seg)
    bare = SemanticGraphSLAM(None, seg)
    p = occupancy_default_params()
    p.resolution = 0.2
    assert len(bare.occupancy_map(p)[0]) == 0 and bare.occupancy_map(p)[4].n_clouds == 0       # nothing kept: what map_cloud returns then
    kept = []
    for ev in events:
        S.setPointCloudData(ev.cloud)
        assert S.VIOCallback(ev.stamp, ev.odom)
        P = ev.cloud.xyz()
        kept.append(seg.downsamplePointcloud(P[np.isfinite(P).all(1)], 0.3)[0])
        if ev.run_after:
            assert S.run()
    first = S.occupancy_map(p, max_out=0)                                                     # one call: it counts, and the clouds travel with it, once
    assert first[4].upload_bytes == 12 * sum(len(c) for c in kept) + 48 * len(kept)
    ids, poses = S.map_cloud(0.2)[3:5]
    got = S.occupancy_map(p)
    assert got[4].n_clouds == len(kept) == len(ids) == 16 and got[4].upload_bytes == 48 * len(kept)
    assert got[4].n_cells == first[4].n_cells == len(got[0])
    _same(S.occupancy_map(p), got, "repeated")
    kf_ids, est = S.getKeyframes()
    want = np.array([list(qmat(LR.from_tq(e)[1])) + list(LR.from_tq(e)[0]) for e in est])
    assert np.array_equal(ids, kf_ids) and np.abs(poses - want).max() <= 1e-12                 # the poses are keyframes()' estimates
    by_hand = seg.occupancy_map(kept, poses, p)
    _same(got, by_hand)
    for k in ("n_points", "n_rays", "n_truncated", "n_clipped_z", "n_steps", "n_bricks", "n_cells"):
        assert getattr(got[4], k) == getattr(by_hand[4], k)
    assert got[4].n_cells == len(got[0]) > 1000 and (got[1] > 0).any() and (got[2] > 0).any()
    p.emit = 1
    occ = S.occupancy_map(p)
    assert 0 < len(occ[0]) < len(got[0]) and (occ[3] >= p.l_occ).all() and occ[4].n_cells == got[4].n_cells
    S.set_map_clouds(False)
    assert len(S.occupancy_map(p)[0]) == 0


# 9
def _shim_input():
    """what tests/shim_occupancy_check.cpp builds: keep the two in step"""
    clouds, poses = [], []
    for c in range(3):
        i = np.arange(200 + 50 * c)
        clouds.append(np.stack([0.125 * (i % 16) - 1.0, 0.0625 * (i // 16) + 0.5 * c, 0.03125 * ((i * 7) % 13)], 1).astype(np.float32))
        R = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])][c]
        poses.append(np.concatenate([R.reshape(-1), [0.25 * c, -0.5 * c, 0.125]]))
    return clouds, poses


def test_cpp_shim_occupancy(gpu_lib, seg, tmp_path):
    from semantic_slam_amd import library_path
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, occupancy_default_params
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_occupancy")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_occupancy_check.cpp"), "-o", exe,
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
    g = re.search(r"shim occupancy generate: cells (\d+) occupied (\d+) hits (\d+) misses (\d+) logodds sum (\S+) centre (\S+) (\S+) (\S+)", out.stdout)
    t = re.search(r"shim occupancy tick: clouds (\d+) cells (\d+) steps (\d+)", out.stdout)
    assert g and t and "shim occupancy ok" in out.stdout, out.stdout
    clouds, poses = _shim_input()
    p = occupancy_default_params()
    p.resolution = 0.125
    p.sensor_origin[:] = [0.0, 0.0, 0.5]
    cells, hits, misses, lo, st = seg.occupancy_map(clouds, poses, p)
    assert [int(g.group(k)) for k in (1, 2, 3, 4)] == [len(cells), int((lo >= p.l_occ).sum()), int(hits.sum()), int(misses.sum())] and len(cells) > 100
    assert np.float64(g.group(5)) == np.float64(repr(float(lo.astype(np.float64).sum())))
    centre = (cells[0].astype(np.float32) + np.float32(0.5)) * np.float32(0.125)
    assert np.array([float(g.group(k)) for k in (6, 7, 8)], np.float32).tobytes() == centre.tobytes()
    # the tick through the shim and through the Python mirror.  The shim hands the odometry over as a matrix, so its quaternions may differ
    # from the mirror's in their last bits and a point on a cell border may change its cell: the cloud count exactly, the cells to 1 %
    S = SemanticGraphSLAM(None, seg)
    S.set_map_clouds(True, 0.3)
    for ev in events:
        S.setPointCloudData(ev.cloud)
        S.VIOCallback(ev.stamp, ev.odom)
        if ev.run_after:
            assert S.run()
    p = occupancy_default_params()
    p.resolution = 0.2
    m = S.occupancy_map(p)
    print("shim", t.groups(), "mirror", m[4])
    assert int(t.group(1)) == m[4].n_clouds == 8 and abs(int(t.group(2)) - len(m[0])) <= 0.01 * len(m[0])
    assert abs(int(t.group(3)) - m[4].n_steps) <= 0.01 * m[4].n_steps
