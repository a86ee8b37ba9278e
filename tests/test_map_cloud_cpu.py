"""The map cloud without a GPU: the cases of tests/map_ref.py bite (checked on the reference alone), the new symbols are exported and
bound, and the argument errors that are decided before the device is touched come back as the header states them."""
import ctypes as C

import numpy as np
import pytest

import map_ref as MR


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def test_lattice_case_bites():
    clouds, poses = MR.lattice_case()
    assert [len(c) for c in clouds][:10] == [0, 1, 63, 64, 65, 255, 256, 0, 257, 1000]
    xyz, counts, cells, st = MR.map_ref(clouds, poses, MR.LATTICE_RESOLUTION)
    # exact arithmetic: the float64 restatement gives the same map, so a failure on this case is about cells, order or layout
    x64, c64, k64, _ = MR.map_ref(clouds, poses, MR.LATTICE_RESOLUTION, transform=MR.transform_f64)
    assert np.array_equal(cells, k64) and np.array_equal(counts, c64) and xyz.tobytes() == x64.tobytes()
    # points exactly on voxel faces: a transformed coordinate that is a multiple of the resolution
    T = np.concatenate([MR.transform_f32(c, p)[0][MR.transform_f32(c, p)[1]] for c, p in zip(clouds, poses)])
    assert (np.mod(T, MR.LATTICE_RESOLUTION) == 0).any(0).all()
    # negative cells, and bricks on both sides of 0 on every axis
    bricks = cells >> 3
    assert (cells.min(0) < -8).all() and (cells.max(0) >= 8).all()
    assert (bricks.min(0) < 0).all() and (bricks.max(0) > 0).all()
    assert st["n_bricks"] > 8 and st["n_voxels"] == len(cells) > 1000
    # the rows that take no part: two in each of the two clouds with bad rows, and the whole last cloud
    assert st["n_points"] - st["n_used"] == 4 + len(clouds[-1])
    # a voxel fed by at least 3 different clouds
    shared = np.floor(MR.LATTICE_SHARED / MR.LATTICE_RESOLUTION).astype(int)
    feeders = 0
    for c, p in zip(clouds, poses):
        t, ok = MR.transform_f32(c, p)
        feeders += bool((np.floor(t[ok] / MR.LATTICE_RESOLUTION).astype(int) == shared).all(1).any())
    assert feeders >= 3
    k = np.flatnonzero((cells == shared).all(1))
    assert len(k) == 1 and counts[k[0]] >= feeders
    # min_points 2 and 4 each drop some voxels and keep some
    assert (counts == 1).any() and (counts >= 4).any()
    kept = [len(MR.map_ref(clouds, poses, MR.LATTICE_RESOLUTION, m)[1]) for m in (1, 2, 4)]
    assert kept[0] > kept[1] > kept[2] > 0
    # the order: bricks ascending with x fastest, then the local index with x fastest
    key = np.stack([cells[:, 0] & 7, cells[:, 1] & 7, cells[:, 2] & 7, bricks[:, 0], bricks[:, 1], bricks[:, 2]], 1)[:, ::-1]
    assert all(tuple(a) < tuple(b) for a, b in zip(key[:-1], key[1:]))


@pytest.mark.parametrize("resolution", [0.05, 0.1, 0.37])
def test_generic_case_needs_the_float32_transform(resolution):
    clouds, poses = MR.generic_case()
    assert len(clouds) == 40 and all(300 <= len(c) <= 3000 for c in clouds)
    xyz, counts, cells, st = MR.map_ref(clouds, poses, resolution)
    x64, c64, k64, _ = MR.map_ref(clouds, poses, resolution, transform=MR.transform_f64)
    # the float32 rule is tested only where a float64 transform gives another map: at every resolution the sums (so the centroids) differ,
    # and at the two finer ones points change their cell as well
    same_cells = len(cells) == len(k64) and np.array_equal(cells, k64) and np.array_equal(counts, c64)
    assert not same_cells or (resolution > 0.3 and xyz.tobytes() != x64.tobytes())
    # many occupied bricks, most of the brick grid empty
    bricks = np.unique(cells >> 3, axis=0)
    box = np.prod((bricks.max(0) - bricks.min(0) + 1).astype(np.int64))
    print("bricks", len(bricks), "of", box, "voxels", len(cells))
    assert len(bricks) == st["n_bricks"] > 100 and len(bricks) < 0.2 * box


def test_shared_voxel_case_is_one_voxel():
    clouds, poses = MR.shared_voxel_case()
    xyz, counts, cells, st = MR.map_ref(clouds, poses, MR.SHARED_RESOLUTION)
    assert len(clouds) == 8 and cells.tolist() == [list(MR.SHARED_CELL)] and counts.tolist() == [60000]
    assert st["n_used"] == 60000 and st["n_bricks"] == 1


def test_far_case_exceeds_the_brick_bound():
    clouds, poses = MR.far_case()
    assert abs(np.linalg.norm(clouds[0][1].astype(np.float64)) - 3000.0) < 1e-3
    per_axis = int(np.floor(clouds[0][1, 0] * (np.float32(1) / np.float32(0.001)))) >> 3
    assert per_axis ** 3 > 2 ** 26 and 8 * per_axis < 2 ** 31


# ---- host-only behaviour of the library -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("sslam_seg_map_cloud", "sslam_seg_last_map_timing", "sslam_slam_set_map_clouds", "sslam_slam_map_clouds_kept", "sslam_slam_map_cloud")


def test_symbols_are_exported_and_bound(hip_lib):
    import subprocess
    from semantic_slam_amd import library_path
    out = subprocess.run(["nm", "-D", "--defined-only", library_path()], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in exported
        assert getattr(hip_lib, name).argtypes is not None, name
    assert not any("seg_map_cloud_device" in e for e in exported)              # the device-pointer entry stays internal
    from semantic_slam_amd._lib import MapStats
    assert C.sizeof(MapStats) == 40 and MapStats.upload_bytes.offset == 24 and MapStats.kernel_ms.offset == 32
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    assert callable(PointCloudSegmentation.map_cloud) and callable(SemanticGraphSLAM.map_cloud) and callable(SemanticGraphSLAM.set_map_clouds)


def _call(lib, h, xyz, start, n_clouds, T, resolution=0.1, min_points=1, out=True, max_out=4):
    buf = np.zeros((4, 3), np.float32)
    return lib.sslam_seg_map_cloud(h, None if xyz is None else xyz.ctypes.data, None if start is None else start.ctypes.data, n_clouds,
                                   None if T is None else T.ctypes.data, C.c_float(resolution), min_points,
                                   buf.ctypes.data if out else None, None, None, max_out, None)


def test_seg_map_cloud_argument_errors(hip_lib):
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    seg = PointCloudSegmentation()
    xyz = np.zeros((3, 3), np.float32)
    start = np.array([0, 2, 3], np.int32)
    T = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (2, 1))
    bad = lambda *a, **k: _call(hip_lib, *a, **k) == MR.INVALID
    assert bad(None, xyz, start, 2, T)                                          # a NULL handle
    assert bad(seg._h, xyz, None, 2, T)                                         # cloud_start NULL with clouds
    assert bad(seg._h, None, start, 2, T)                                       # xyz NULL with points
    assert bad(seg._h, xyz, start, 2, None)                                     # T NULL with clouds
    assert bad(seg._h, xyz, start, 2, T, out=False)                             # xyz_out NULL with max_out > 0
    assert bad(seg._h, xyz, start, -1, T)
    assert bad(seg._h, xyz, start, 2, T, max_out=-1)
    assert bad(seg._h, xyz, start, 2, T, min_points=-1)
    assert bad(seg._h, xyz, np.array([0, 3, 2], np.int32), 2, T)                # decreases
    assert bad(seg._h, xyz, np.array([-1, 2, 3], np.int32), 2, T)               # starts below 0
    for r in (0.0, -0.1, np.nan, np.inf, 1e-45):                                # 1 / 1e-45 overflows float32
        assert bad(seg._h, xyz, start, 2, T, resolution=r), r
    for v in (np.nan, np.inf):
        Tb = T.copy(); Tb[1, 10] = v
        assert bad(seg._h, xyz, start, 2, Tb)
    assert b"pose of cloud 1" in hip_lib.sslam_last_error()
    # valid arguments reach the device: without one the call says so, with one it answers
    rc = _call(hip_lib, seg._h, xyz, start, 2, T)
    assert rc == (MR.NO_DEVICE if hip_lib.sslam_device_count() == 0 else 1)
    ms = np.ones(4)
    assert hip_lib.sslam_seg_last_map_timing(seg._h, ms.ctypes.data) == 0 and (ms >= 0).all()
    assert hip_lib.sslam_seg_last_map_timing(None, ms.ctypes.data) == MR.INVALID


def test_set_map_clouds_argument_errors(hip_lib):
    from semantic_slam_amd import SslamError
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    assert hip_lib.sslam_slam_set_map_clouds(None, 1, C.c_float(0.1)) == MR.INVALID
    bare = SemanticGraphSLAM()
    with pytest.raises(SslamError) as ei:                                       # `on` without a frontend handle
        bare.set_map_clouds(True)
    assert ei.value.code == MR.INVALID and "frontend handle" in str(ei.value)
    bare.set_map_clouds(False)                                                  # off needs none
    seg = PointCloudSegmentation()
    S = SemanticGraphSLAM(None, seg)
    for leaf in (-0.1, np.nan, np.inf):
        with pytest.raises(SslamError):
            S.set_map_clouds(True, leaf)
    # the kept clouds are read by the frontend's kernels on the frontend's device: the two handles on different devices are refused, on the host
    from semantic_slam_amd.semantic_graph_slam import default_slam_params
    for slam_dev, seg_dev in ((0, 1), (1, 0)):
        other = SemanticGraphSLAM(default_slam_params(slam_dev), PointCloudSegmentation(device=seg_dev))
        with pytest.raises(SslamError) as ei:
            other.set_map_clouds(True)
        assert ei.value.code == MR.UNSUPPORTED and "same device" in str(ei.value)
        other.set_map_clouds(False)
        assert other.map_cloud(0.2)[5].n_clouds == 0
    S.set_map_clouds(True, 0.0)                                                 # 0 -> 0.1
    S.set_map_clouds(True, 0.3)
    # nothing kept yet: 0 without touching the device, the argument rules first
    n = C.c_int32(-1)
    assert hip_lib.sslam_slam_map_clouds_kept(S._h, C.byref(n)) == 0 and n.value == 0
    xyz, counts, cells, ids, poses, st = S.map_cloud(0.2)
    assert len(xyz) == len(counts) == len(cells) == len(ids) == len(poses) == 0 and st.n_clouds == 0 and st.upload_bytes == 0
    with pytest.raises(SslamError):
        S.map_cloud(0.0)
    with pytest.raises(SslamError):
        S.map_cloud(0.2, min_points=-1)
    assert hip_lib.sslam_slam_map_cloud(None, C.c_float(0.2), 1, None, None, None, 0, None, None, 0, None) == MR.INVALID
    assert hip_lib.sslam_slam_map_cloud(S._h, C.c_float(0.2), 1, None, None, None, 0, None, None, -1, None) == MR.INVALID
    assert hip_lib.sslam_slam_map_cloud(S._h, C.c_float(0.2), 1, None, None, None, 3, None, None, 0, None) == MR.INVALID   # xyz_out NULL, max_out > 0
    S.set_map_clouds(False)
    assert S.map_cloud(0.2)[5].n_clouds == 0


def test_cpp_shim_compiles_and_refuses_on_the_host(hip_lib, tmp_path):
    """tests/shim_map_check.cpp without a recording: the shim headers compile and link, and the host-side refusals hold"""
    import os
    import subprocess
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_map")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(root, "tests", "shim_map_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "shim map ok" in out.stdout, out.stdout + out.stderr
