"""The per-scan occupancy reference on its own (no GPU): tests/occupancy_scan_ref.py's two formulations against each other, and the proof that
the cases of tests/test_occupancy_scans_gpu.py tell OctoMap's per-scan update from the ray entry's per-ray counts and clamp of the sum.  Each
bar sits below the value measured when the cases were written, which follows it in parentheses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import occupancy_ref as OR
import occupancy_scan_ref as SR


@pytest.fixture(scope="module")
def lattice():
    clouds, poses = OR.lattice_case()
    P = OR.lattice_params()
    return clouds, poses, P, SR.scan_ref(clouds, poses, P), OR.occupancy_ref(clouds, poses, P)


@pytest.fixture(scope="module")
def moved():
    clouds, poses = SR.moved_case()
    P = SR.moved_params()
    return clouds, poses, P, SR.scan_ref(clouds, poses, P), OR.occupancy_ref(clouds, poses, P)


def _equal(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a[4] == b[4]


def test_the_two_formulations_agree(lattice, moved):
    for clouds, poses, P, ref, _ in (lattice, moved):
        _equal(ref, SR.scan_ref_vec(clouds, poses, P))
    clouds, poses, P = lattice[:3]
    for e in (1, 2):
        _equal(SR.scan_ref(clouds, poses, dict(P, emit=e)), SR.scan_ref_vec(clouds, poses, dict(P, emit=e)))
    gc, gp, max_range = OR.generic_case()
    for r in (0.05, 0.37):
        Q = OR.default_params(resolution=r, max_range=max_range, sensor_origin=OR.GENERIC_ORIGIN)
        _equal(SR.scan_ref(gc, gp, Q), SR.scan_ref_vec(gc, gp, Q))


def test_known_cells_are_the_ray_entrys(lattice, moved):
    for _, _, _, ref, ray in (lattice, moved):
        assert np.array_equal(ref[0], ray[0]) and len(ref[0]) > 1000
        for k in ("n_clouds", "n_points", "n_rays", "n_truncated", "n_clipped_z", "n_cells", "n_bricks"):
            assert ref[4][k] == ray[4][k], k
        assert ref[4]["n_steps"] == int(ref[1].sum() + ref[2].sum()) < ray[4]["n_steps"]
        assert (ref[1] + ref[2] > 0).all() and (ref[1] <= ray[1]).all() and (ref[2] <= ray[2]).all()


def test_lattice_case_bites(lattice):
    clouds, poses, P, ref, ray = lattice
    overridden = sum(len(H & V) for H, V, _ in (SR.scan_sets(c, T, P) for c, T in zip(clouds, poses)))
    assert overridden >= 100                                                   # (scan, cell) pairs where a hit overrides a miss (168)
    assert int((ref[1] != ray[1]).sum()) >= 5                                  # cells whose hit counts differ from the ray entry's (8)
    assert int((ref[2] != ray[2]).sum()) >= 1000                               # cells whose miss counts differ (1904)
    assert ref[1].max() <= len(clouds) and ref[2].max() <= len(clouds)         # a cell is counted once per scan


def test_moved_case_bites(moved):
    clouds, poses, P, ref, ray = moved
    assert sum(len(c) for c in clouds) == 3120 and len(clouds) == 130
    assert int((np.abs(ref[3] - OR.cell_logodds(ref[1], ref[2], P)) > 0.1).sum()) >= 20   # sequential against clamp of the sum (63)
    rev = SR.scan_ref(clouds[::-1], poses[::-1], P)
    assert np.array_equal(rev[0], ref[0]) and np.array_equal(rev[1], ref[1]) and np.array_equal(rev[2], ref[2])
    assert int(((ref[3] >= P["l_occ"]) != (rev[3] >= P["l_occ"])).sum()) >= 15            # occupied in one order, free in the other (41)
    assert int((ref[3] == P["l_min"]).sum()) >= 1000                                      # (4257)
    assert int((ref[3] == P["l_max"]).sum()) >= 20                                        # (131)
    # the object that has gone: occupied for ever under the clamp of the sum, free under OctoMap's rule
    gone = (ray[3] >= P["l_occ"]) & (ref[3] < P["l_occ"]) & (ref[1] >= 10)
    assert int(gone.sum()) >= 10


def test_update_rule_by_hand():
    P = OR.default_params()
    lo = np.float32(0.0)
    for _ in range(70):
        lo = SR.update(lo, P["l_hit"], P)
    assert lo == P["l_max"]
    n = 0
    while lo >= P["l_occ"]:
        lo = SR.update(lo, P["l_miss"], P)
        n += 1
    assert n == 9                                                              # l_max 3.51 over l_miss -0.405: free after nine misses
    one = np.array([[1.0, 0.02, 0.02], [1.0, 0.021, 0.02], [2.0, 0.04, 0.04]], np.float32)   # two rays end in one cell, the third passes through it
    cells, hits, misses, lo, st = SR.scan_ref([one], [OR.identity_pose()], P)
    at = np.flatnonzero((cells == (20, 0, 0)).all(1))
    assert len(at) == 1 and hits[at[0]] == 1 and misses[at[0]] == 0 and lo[at[0]] == P["l_hit"]
    assert hits.sum() == 2 and (misses <= 1).all() and st["n_steps"] == len(cells)


# ---- the host side of the C-ABI: what answers without a GPU ----------------------------------------------------------------------------
def test_argument_errors_are_the_ray_entrys(hip_lib):
    from semantic_slam_amd import SslamError
    from semantic_slam_amd.segmentation import PointCloudSegmentation, occupancy_default_params, pack_clouds
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    seg = PointCloudSegmentation()
    xyz, start, T = pack_clouds([np.ones((3, 3), np.float32), np.zeros((2, 3), np.float32)], [OR.identity_pose(), OR.identity_pose()])
    p = occupancy_default_params()

    def call(entry, q, start=start, T=T, max_out=0, n_clouds=2):
        return entry(seg._h, xyz.ctypes.data, start.ctypes.data, n_clouds, T.ctypes.data, None if q is None else C.byref(q), None, None, None, None, max_out, None)

    def both(*a, **kw):
        rc = [call(e, *a, **kw) for e in (hip_lib.sslam_seg_occupancy_map, hip_lib.sslam_seg_occupancy_map_scans)]
        assert rc[0] == rc[1], (a, kw, rc)
        return rc[1]
    for field, v in (("resolution", 0.0), ("resolution", np.nan), ("max_range", -1.0), ("max_range", 6000.0), ("l_hit", 0.0), ("l_miss", 0.0),
                     ("l_min", 9.0), ("z_min", 9.0), ("emit", 3), ("emit", -1)):
        q = occupancy_default_params()
        setattr(q, field, v)
        assert both(q) == OR.INVALID, field                                     # refused before the device is looked for
    assert both(None) == OR.INVALID and both(p, max_out=-1) == OR.INVALID and both(p, n_clouds=-1) == OR.INVALID
    assert both(p, start=np.array([0, 3, 2], np.int32)) == OR.INVALID and both(p, start=np.array([-1, 3, 5], np.int32)) == OR.INVALID
    Tb = T.copy(); Tb[1, 3] = np.inf
    assert both(p, T=Tb) == OR.INVALID and b"pose of cloud 1" in hip_lib.sslam_last_error()
    assert hip_lib.sslam_seg_occupancy_map_scans(None, None, None, 0, None, C.byref(p), None, None, None, None, 0, None) == OR.INVALID
    assert both(p) == (OR.NO_DEVICE if hip_lib.sslam_device_count() == 0 else 4)   # valid arguments reach the device
    ms = np.ones(2)
    assert hip_lib.sslam_seg_last_occupancy_scan_timing(seg._h, ms.ctypes.data) == 0 and (ms >= 0).all()
    assert hip_lib.sslam_seg_last_occupancy_scan_timing(None, ms.ctypes.data) == OR.INVALID
    assert hip_lib.sslam_seg_last_occupancy_scan_timing(seg._h, None) == OR.INVALID
    n = np.ones(2, np.int64)
    assert hip_lib.sslam_seg_last_occupancy_scan_counts(seg._h, n.ctypes.data) == 0 and (n >= 0).all()
    assert hip_lib.sslam_seg_last_occupancy_scan_counts(None, n.ctypes.data) == OR.INVALID
    if hip_lib.sslam_device_count() == 0:
        with pytest.raises(SslamError) as ei:
            seg.occupancy_map_scans([np.ones((3, 3), np.float32)], [OR.identity_pose()])
        assert ei.value.code == OR.NO_DEVICE
    # the tick's entry: nothing kept -> 0 without touching the device, the argument rules first
    S = SemanticGraphSLAM(None, seg)
    S.set_map_clouds(True, 0.3)
    out = S.occupancy_map_scans()
    assert all(len(a) == 0 for a in out[:4]) and out[4].n_clouds == 0 and out[4].upload_bytes == 0
    q = occupancy_default_params()
    q.emit = -1
    with pytest.raises(SslamError):
        S.occupancy_map_scans(q)
    assert hip_lib.sslam_slam_occupancy_map_scans(None, C.byref(p), None, None, None, None, 0, None) == OR.INVALID
    assert hip_lib.sslam_slam_occupancy_map_scans(S._h, None, None, None, None, None, 0, None) == OR.INVALID


def test_cpp_shim_compiles_and_refuses_on_the_host(hip_lib, tmp_path):
    """tests/shim_occupancy_scans_check.cpp without a recording: the shim headers compile and link, and the host-side refusals hold"""
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_occupancy_scans")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(root, "tests", "shim_occupancy_scans_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "shim occupancy scans ok" in out.stdout, out.stdout + out.stderr
