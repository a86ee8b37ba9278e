"""The per-scan occupancy map on the GPU: sslam_seg_occupancy_map_scans against tests/occupancy_scan_ref.py's restatement of its contract, and
sslam_slam_occupancy_map_scans (the tick's resident keyframe clouds) against the same call fed by hand.

Every comparison is exact, stats included: cells, hits and misses by np.array_equal, the log-odds by their bytes.  The contract fixes every
operation -- the ray entry's integers up to the visited cells, then one float32 add and two clamps per (scan, cell) in the order of the clouds
-- so nothing is left to a tolerance.  tests/test_occupancy_scans_cpu.py shows on the references alone that the cases tell this entry from the
ray entry: with per-ray counts or a clamp of the sum behind the new name, tests 1, 3, 5 and 6 fail."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loop_scene as LS
import occupancy_ref as OR
import occupancy_scan_ref as SR

pytestmark = pytest.mark.gpu

CHUNK_EDGES = (1, 31, 32, 33, 63, 64, 65, 129, 130)        # around both chunk widths the kernels may use, 32 and 64


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
    assert st.reserved == 0


def _check(seg, clouds, poses, P, ref, what=""):
    got = seg.occupancy_map_scans(clouds, poses, _struct(P))
    _same(got, ref, what)
    _stats_match(got[4], ref[4])
    return got


@pytest.fixture(scope="module")
def lattice():
    clouds, poses = OR.lattice_case()
    P = OR.lattice_params()
    return clouds, poses, P, {e: SR.scan_ref(clouds, poses, dict(P, emit=e)) for e in (0, 1, 2)}


@pytest.fixture(scope="module")
def moved():
    clouds, poses = SR.moved_case()
    P = SR.moved_params()
    return clouds, poses, P, {n: SR.scan_ref(clouds[:n], poses[:n], P) for n in CHUNK_EDGES}


def _raw(seg, clouds, poses, p, cells=None, hits=None, misses=None, lo=None, max_out=0, stats=None, start=None, T=None, n_clouds=None):
    from semantic_slam_amd.segmentation import pack_clouds
    xyz, st, TT = pack_clouds(clouds, poses)
    start = st if start is None else start
    T = TT if T is None else T
    ptr = lambda a: None if a is None else a.ctypes.data
    return seg._lib.sslam_seg_occupancy_map_scans(seg._h, ptr(xyz) if len(xyz) else None, ptr(start), len(clouds) if n_clouds is None else n_clouds, ptr(T),
                                                  None if p is None else C.byref(p), ptr(cells), ptr(hits), ptr(misses), ptr(lo), max_out,
                                                  None if stats is None else C.byref(stats))


# 1
def test_lattice(seg, lattice):
    clouds, poses, P, ref = lattice
    got = _check(seg, clouds, poses, P, ref[0], "lattice")
    st = got[4]
    assert st.upload_bytes == 12 * st.n_points + 48 * st.n_clouds + 4 * (st.n_clouds + 1)
    t4, t2 = seg.last_occupancy_timing(), seg.last_occupancy_scan_timing()
    assert st.kernel_ms > 0 and abs(t4.sum() - st.kernel_ms) <= 1e-9 * st.kernel_ms
    assert (t2 > 0).all() and abs(t2.sum() - t4[2]) <= 1e-9 * t4[2]           # slot 2 is mark plus fold
    assert st.n_steps == int(got[1].sum()) + int(got[2].sum()) and seg.last_occupancy_count == len(got[0])
    visited, issued = seg.last_occupancy_scan_counts()
    assert visited == seg.occupancy_map(clouds, poses, _struct(P))[4].n_steps and st.n_steps <= issued <= visited
    _same(seg.occupancy_map_scans(clouds, poses, _struct(P)), got, "repeated call")


# 2
@pytest.mark.parametrize("resolution", [0.05, 0.1, 0.37])
def test_generic(seg, resolution):
    clouds, poses, max_range = OR.generic_case()
    P = OR.default_params(resolution=resolution, max_range=max_range, sensor_origin=OR.GENERIC_ORIGIN)
    got = _check(seg, clouds, poses, P, SR.scan_ref(clouds, poses, P))
    assert 0.1 * got[4].n_rays < got[4].n_truncated < 0.3 * got[4].n_rays
    print("resolution", resolution, got[4], "passes ms", seg.last_occupancy_timing(), "mark, fold ms", seg.last_occupancy_scan_timing())


# 3
def test_moved_forward_and_reversed(seg, moved):
    clouds, poses, P, ref = moved
    fwd = _check(seg, clouds, poses, P, ref[130], "forward")
    rev = _check(seg, clouds[::-1], poses[::-1], P, SR.scan_ref(clouds[::-1], poses[::-1], P), "reversed")
    assert np.array_equal(fwd[0], rev[0]) and np.array_equal(fwd[1], rev[1]) and np.array_equal(fwd[2], rev[2])
    assert fwd[3].tobytes() != rev[3].tobytes() and int(((fwd[3] >= P["l_occ"]) != (rev[3] >= P["l_occ"])).sum()) >= 15


# 4
@pytest.mark.parametrize("n", CHUNK_EDGES)
def test_chunk_edges(seg, moved, n):
    clouds, poses, P, ref = moved
    _check(seg, clouds[:n], poses[:n], P, ref[n], "first %d clouds" % n)


# 5
def test_points_permuted_and_repeated(seg, lattice, moved):
    rng = np.random.default_rng(0)
    for clouds, poses, P, ref in (lattice[:3] + (lattice[3][0],), moved[:3] + (moved[3][130],)):
        p = _struct(P)
        _same(seg.occupancy_map_scans([c[rng.permutation(len(c))] for c in clouds], poses, p), ref, "points permuted")
        twice = [np.concatenate([c, c]) for c in clouds]
        got = seg.occupancy_map_scans(twice, poses, p)
        _same(got, ref, "every cloud twice in itself")
        assert got[4].n_steps == ref[4]["n_steps"] and got[4].n_rays == 2 * ref[4]["n_rays"]
        once, doubled = seg.occupancy_map(clouds, poses, p), seg.occupancy_map(twice, poses, p)
        assert np.array_equal(doubled[1], 2 * once[1]) and np.array_equal(doubled[2], 2 * once[2])   # the ray entry counts rays


# 6
def test_one_point_per_cloud(seg, moved):
    """a scan of one ray has nothing to de-duplicate: the counts are the ray entry's, the log-odds are sequential.  The same grid ray of
    clouds 50 .. 89: twenty scans end on the patch, twenty pass through it"""
    clouds, poses, P, _ = moved
    clouds, poses = [c[5:6] for c in clouds[50:90]], poses[50:90]
    got = _check(seg, clouds, poses, P, SR.scan_ref(clouds, poses, P))
    ray = seg.occupancy_map(clouds, poses, _struct(P))
    assert got[4].n_clouds == 40 == got[4].n_rays
    assert np.array_equal(got[0], ray[0]) and np.array_equal(got[1], ray[1]) and np.array_equal(got[2], ray[2]) and got[4].n_steps == ray[4].n_steps
    assert int((got[3] != ray[3]).sum()) >= 3                                  # the clamp after every update shows (5 cells on the CPU)


# 7
def test_clouds_that_take_no_part(seg, lattice, moved):
    clouds, poses, P, _ = lattice
    bad = [c.copy() for c in clouds[:3]]
    bad[0][5] = (np.nan, 0, 0); bad[0][62] = (0, np.inf, 0); bad[2][63] = (0, 0, -np.inf); bad[2][64] = (np.nan, np.nan, np.nan)
    # the ray origin of this pose overflows in its last addition, 2.6e38 + 3e38: the cloud is a scan without updates
    over = OR.identity_pose(); over[0:3] = (3e38, -3e38, 3e38); over[9] = 3e38
    assert not OR.transform(P["sensor_origin"].reshape(1, 3), over)[1][0]
    empty = np.zeros((0, 3), np.float32)
    cl = [bad[0], empty, bad[1], clouds[3], np.full((7, 3), np.nan, np.float32), bad[2], empty]
    ps = [poses[0], poses[1], poses[1], over, poses[3], poses[2], poses[4]]
    got = _check(seg, cl, ps, P, SR.scan_ref(cl, ps, P), "with the clouds that take no part")
    assert got[4].n_points - got[4].n_rays - got[4].n_clipped_z == 4 + len(clouds[3]) + 7
    rows = lambda c: c[np.isfinite(c).all(1)]
    _same(seg.occupancy_map_scans([rows(bad[0]), bad[1], rows(bad[2])], [poses[0], poses[1], poses[2]], _struct(P)), got, "without them")
    assert len(seg.occupancy_map_scans([empty, clouds[3]], [poses[0], over], _struct(P))[0]) == 0
    st = seg.occupancy_map_scans([], [], _struct(P))[4]
    assert (st.n_clouds, st.n_points, st.n_cells) == (0, 0, 0) and seg.last_occupancy_count == 0
    # 64 consecutive empty clouds in the middle of the moved case: whole chunks without a ray, bits that stay clear
    clouds, poses, P, ref = moved
    cl, ps = clouds[:40] + [empty] * 64 + clouds[40:], poses[:40] + [poses[0]] * 64 + poses[40:]
    got = seg.occupancy_map_scans(cl, ps, _struct(P))
    _same(got, ref[130], "64 empty clouds")
    _stats_match(got[4], dict(ref[130][4], n_clouds=194))


# 8
def test_emit_modes_and_max_out(seg, lattice, moved):
    from semantic_slam_amd._lib import OccStats
    clouds, poses, P, ref = lattice
    for e in (0, 1, 2):
        _check(seg, clouds, poses, dict(P, emit=e), ref[e], "emit %d" % e)   # n_cells and n_steps count before emit in every mode
    clouds, poses, P, mref = moved                                             # where the sequential log-odds and the clamp of the sum disagree
    got = {e: seg.occupancy_map_scans(clouds, poses, _struct(dict(P, emit=e))) for e in (0, 1, 2)}
    _same(got[0], mref[130])
    assert len(got[1][0]) > 0 and len(got[2][0]) > 0 and len(got[1][0]) + len(got[2][0]) == len(got[0][0])
    assert (got[1][3] >= P["l_occ"]).all() and (got[2][3] < P["l_occ"]).all()
    occupied = got[0][3] >= P["l_occ"]
    for e, pick in ((1, occupied), (2, ~occupied)):
        _same(got[e], tuple(a[pick] for a in got[0][:4]), "emit %d" % e)
        _stats_match(got[e][4], mref[130][4])
    assert (OR.cell_logodds(got[0][1], got[0][2], P)[~occupied] >= P["l_occ"]).any()   # free here, occupied by the clamp of the sum
    # max_out below the count: the true count is returned and the prefix is written; the rows behind it keep what the caller put there
    clouds, poses, P, ref = lattice
    total = len(ref[0][0])
    p = _struct(P)
    for cap in (0, 1, 257, total - 1, total + 5):
        cells = np.full((total + 9, 3), -9, np.int32); hits = np.full(total + 9, -3, np.int32); misses = np.full(total + 9, -4, np.int32)
        lo = np.full(total + 9, 7.5, np.float32)
        assert _raw(seg, clouds, poses, p, cells, hits, misses, lo, cap) == total
        m = min(cap, total)
        _same((cells[:m], hits[:m], misses[:m], lo[:m]), tuple(a[:m] for a in ref[0][:4]), "max_out %d" % cap)
        assert (cells[m:] == -9).all() and (hits[m:] == -3).all() and (misses[m:] == -4).all() and (lo[m:] == 7.5).all()
    # a count-only call, and every optional output pointer NULL
    st = OccStats()
    assert _raw(seg, clouds, poses, p) == total
    assert _raw(seg, clouds, poses, p, None, None, None, None, total, st) == total and st.n_cells == total and st.n_steps == ref[0][4]["n_steps"]
    lo = np.zeros(total, np.float32)
    assert _raw(seg, clouds, poses, p, None, None, None, lo, total, None) == total and lo.tobytes() == ref[0][3].tobytes()
    assert _raw(seg, clouds, poses, _struct(dict(P, emit=1))) == len(ref[1][0])


# 9
def test_error_returns(gpu_lib, seg, lattice):
    from semantic_slam_amd import SslamError
    from semantic_slam_amd.synth import make_frame
    clouds, poses, P, ref = lattice
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
    assert gpu_lib.sslam_seg_occupancy_map_scans(None, None, None, 0, None, C.byref(p), None, None, None, None, 0, None) == OR.INVALID
    # the limits: two points 3000 m apart at resolution 0.01 -- the brick grid fails before any table is sized
    fc, fp = OR.far_case()
    with pytest.raises(SslamError) as ei:
        seg.occupancy_map_scans(fc, fp, _struct(OR.default_params(resolution=0.01, max_range=10.0)))
    assert ei.value.code == OR.UNSUPPORTED and "bricks" in str(ei.value)
    assert len(seg.occupancy_map_scans(fc, fp, _struct(OR.default_params(resolution=0.5, max_range=10.0)))[0]) > 2   # the same at a resolution that fits
    with pytest.raises(SslamError) as ei:                                      # a ray beyond 2^19 cells
        seg.occupancy_map_scans([np.array([[30000.0, 0, 0]], np.float32)], fp[:1], _struct(OR.default_params()))
    assert ei.value.code == OR.UNSUPPORTED and "2^19" in str(ei.value)
    _check(seg, lattice[0], lattice[1], P, ref[0])
    # a batch in flight
    seg.submit_frames([make_frame(seed=3, n_boxes=2)])
    assert _raw(seg, clouds, poses, p) == OR.INVALID and b"in flight" in gpu_lib.sslam_last_error()
    seg.collect_frames()
    _check(seg, lattice[0], lattice[1], P, ref[0])


# 10
def test_interleaved_with_the_ray_entry(seg, lattice):
    clouds, poses, P, ref = lattice
    ray = OR.occupancy_ref(clouds, poses, P)
    for _ in range(2):
        got = seg.occupancy_map(clouds, poses, _struct(P))
        _same(got, ray, "the ray entry")
        for k, v in ray[4].items():
            assert getattr(got[4], k) == v, k
        _check(seg, clouds, poses, P, ref[0], "the scan entry")


# 11
def test_tick(seg):
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params, occupancy_default_params
    events = LS.make_events(16)
    sp = default_slam_params()
    sp.const_stddev_x, sp.const_stddev_q = LS.ODOM_STDDEV_X, LS.ODOM_STDDEV_Q
    S = SemanticGraphSLAM(sp, seg)
    S.set_map_clouds(True, 0.3)
    bare = SemanticGraphSLAM(None, seg)
    p = occupancy_default_params()
    p.resolution = 0.2
    assert len(bare.occupancy_map_scans(p)[0]) == 0 and bare.occupancy_map_scans(p)[4].n_clouds == 0   # nothing kept
    kept = []
    for ev in events:
        S.setPointCloudData(ev.cloud)
        assert S.VIOCallback(ev.stamp, ev.odom)
        P = ev.cloud.xyz()
        kept.append(seg.downsamplePointcloud(P[np.isfinite(P).all(1)], 0.3)[0])
        if ev.run_after:
            assert S.run()
    first = S.occupancy_map_scans(p, max_out=0)                                # one call: it counts, and the clouds travel with it, once
    assert first[4].upload_bytes == 12 * sum(len(c) for c in kept) + 48 * len(kept)
    ids, poses = S.map_cloud(0.2)[3:5]
    got = S.occupancy_map_scans(p)
    assert got[4].n_clouds == len(kept) == len(ids) == 16 and got[4].upload_bytes == 48 * len(kept)
    assert got[4].n_cells == first[4].n_cells == len(got[0])
    _same(S.occupancy_map_scans(p), got, "repeated")
    by_hand = seg.occupancy_map_scans(kept, poses, p)
    _same(got, by_hand)
    for k in ("n_points", "n_rays", "n_truncated", "n_clipped_z", "n_steps", "n_bricks", "n_cells"):
        assert getattr(got[4], k) == getattr(by_hand[4], k)
    ray = S.occupancy_map(p)                                                   # the same clouds and poses through the ray entry
    assert ray[4].upload_bytes == 48 * len(kept) and np.array_equal(ray[0], got[0]) and got[4].n_steps < ray[4].n_steps
    assert (got[1] <= 16).all() and (got[2] <= 16).all() and (got[1] > 0).any() and len(got[0]) > 1000
    p.emit = 1
    occ = S.occupancy_map_scans(p)
    assert 0 < len(occ[0]) < len(got[0]) and (occ[3] >= p.l_occ).all() and occ[4].n_cells == got[4].n_cells
    S.set_map_clouds(False)
    assert len(S.occupancy_map_scans(p)[0]) == 0


# 12
def _shim_input():
    """what tests/shim_occupancy_scans_check.cpp builds: keep the two in step"""
    clouds, poses = [], []
    for c in range(3):
        i = np.arange(200 + 50 * c)
        clouds.append(np.stack([0.125 * (i % 16) - 1.0, 0.0625 * (i // 16) + 0.5 * c, 0.03125 * ((i * 7) % 13)], 1).astype(np.float32))
        R = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])][c]
        poses.append(np.concatenate([R.reshape(-1), [0.25 * c, -0.5 * c, 0.125]]))
    return clouds, poses


def test_cpp_shim_occupancy_scans(gpu_lib, seg, tmp_path):
    from semantic_slam_amd import library_path
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, occupancy_default_params
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_occupancy_scans")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "shim_occupancy_scans_check.cpp"), "-o", exe,
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
    g = re.search(r"shim occupancy scans generate: cells (\d+) occupied (\d+) hits (\d+) misses (\d+) logodds sum (\S+)", out.stdout)
    t = re.search(r"shim occupancy scans tick: clouds (\d+) cells (\d+) steps (\d+)", out.stdout)
    assert g and t and "shim occupancy scans ok" in out.stdout, out.stdout
    clouds, poses = _shim_input()
    p = occupancy_default_params()
    p.resolution = 0.125
    p.sensor_origin[:] = [0.0, 0.0, 0.5]
    cells, hits, misses, lo, st = seg.occupancy_map_scans(clouds, poses, p)
    assert [int(g.group(k)) for k in (1, 2, 3, 4)] == [len(cells), int((lo >= p.l_occ).sum()), int(hits.sum()), int(misses.sum())] and len(cells) > 100
    assert np.float64(g.group(5)) == np.float64(repr(float(lo.astype(np.float64).sum())))
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
    m = S.occupancy_map_scans(p)
    print("shim", t.groups(), "mirror", m[4])
    assert int(t.group(1)) == m[4].n_clouds == 8 and abs(int(t.group(2)) - len(m[0])) <= 0.01 * len(m[0])
    assert abs(int(t.group(3)) - m[4].n_steps) <= 0.01 * m[4].n_steps
