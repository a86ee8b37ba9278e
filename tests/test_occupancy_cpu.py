"""The occupancy reference on its own (no GPU): tests/occupancy_ref.py's restatement of the traversal against a second reference that does not
come from the contract -- per cell, in fractions.Fraction, the parameter interval in which the exact segment Qo -> Qe lies inside the cell's
cube -- and the proof that the cases of tests/test_occupancy_gpu.py bite: ties, ends on faces, cut and clipped rays, clamps."""
import numpy as np
import pytest

import occupancy_ref as OR


@pytest.fixture(scope="module")
def lattice():
    clouds, poses = OR.lattice_case()
    P = OR.lattice_params()
    rays, st = OR.rays_of(clouds, poses, P)
    return clouds, poses, P, rays, st


def _some_rays(rays, n, seed):
    pick = np.random.default_rng(seed).permutation(len(rays))[:n]
    return [rays[k] for k in pick]


def _check_walk(Qo, Qe):
    path = OR.walk(Qo, Qe)
    co, ce = tuple(o >> 10 for o in Qo), tuple(e >> 10 for e in Qe)
    assert path[0] == co and path[-1] == ce
    assert len(path) - 1 == sum(abs(a - b) for a, b in zip(co, ce))           # the steps are the Manhattan distance of the end cells
    for a, b in zip(path, path[1:]):
        assert sorted(abs(x - y) for x, y in zip(a, b)) == [0, 0, 1]            # one step on one axis
    touched, crossed = OR.segment_cells_exact(Qo, Qe)
    assert set(path) <= touched, sorted(set(path) - touched)                    # every visited cell meets the segment
    assert crossed <= set(path), sorted(crossed - set(path))                    # every cell whose interior it crosses is visited


def test_walk_against_exact_segment_lattice(lattice):
    rays = lattice[3]
    tied = [r for r in rays if OR.ties_of(r[0], r[1]) >= 2]
    on_face = [r for r in rays if any(e < o and e & 1023 == 0 for o, e in zip(r[0], r[1]))]
    for Qo, Qe, _ in tied[:25] + on_face[:15] + _some_rays(rays, 25, 0):
        _check_walk(Qo, Qe)


def test_walk_against_exact_segment_generic():
    clouds, poses, max_range = OR.generic_case()
    P = OR.default_params(resolution=0.37, max_range=max_range, sensor_origin=OR.GENERIC_ORIGIN, z_min=-10, z_max=10)
    rays, st = OR.rays_of(clouds, poses, P)
    assert 0.1 * st["n_rays"] < st["n_truncated"] < 0.3 * st["n_rays"]         # about a fifth of the rays are cut
    for Qo, Qe, _ in _some_rays(rays, 40, 1):
        _check_walk(Qo, Qe)


def test_walk_by_hand():
    # from the middle of cell 0 one cell up the diagonal: the corner (1, 1) is an exact tie, x goes first
    assert OR.walk([512, 512, 512], [1536, 1536, 512]) == [(0, 0, 0), (1, 0, 0), (1, 1, 0)]
    # the three-axis corner: x, then y, then z
    assert OR.walk([0, 0, 0], [1536, 1536, 1536]) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
    # going down and ending exactly on the face between cells -1 and 0: the end cell is 0, the face is not crossed
    assert OR.walk([2560, 100, 100], [0, 100, 100]) == [(2, 0, 0), (1, 0, 0), (0, 0, 0)]
    # going up and ending exactly on a face: the end cell is the one above it
    assert OR.walk([100, 100, 100], [2048, 100, 100]) == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    # starting on a face and going down leaves the start cell at once
    assert OR.walk([1024, 512, 0], [512, 512, 0]) == [(1, 0, 0), (0, 0, 0)]
    assert OR.walk([5, 6, 7], [5, 6, 7]) == [(0, 0, 0)]
    # the cut: |D| = 5000 > R = 2500 halves the ray exactly; an inexact quotient is rounded towards zero on both sides of zero
    assert OR.cut([0, 0, 0], [3000, -4000, 0], 2500) == ([1500, -2000, 0], True)
    assert OR.cut([0, 0, 0], [3001, -4001, 1], 2500) == ([1499, -1999, 0], True)
    assert OR.cut([0, 0, 0], [1500, -2000, 0], 2500) == ([1500, -2000, 0], False)
    # a tiny negative coordinate: u - floor(u) rounds to 1, q stays at 1023
    assert OR.position(np.float32(-1e-9), np.float32(8.0)) == -1024 + 1023
    assert OR.position(np.float32(-0.125), np.float32(8.0)) == -1024 and OR.position(np.float32(0.125), np.float32(8.0)) == 1024


def test_lattice_case_bites(lattice):
    clouds, poses, P, rays, st = lattice
    assert [len(c) for c in clouds] == list(OR.LATTICE_SIZES)
    ties = [OR.ties_of(r[0], r[1]) for r in rays]
    assert sum(t >= 2 for t in ties) >= 20 and sum(t == 3 for t in ties) >= 5
    assert sum(any(e < o and e & 1023 == 0 for o, e in zip(r[0], r[1])) for r in rays) >= 10   # going down, ending exactly on a face
    assert st["n_truncated"] >= 10 and st["n_clipped_z"] >= 10
    assert st["n_rays"] + st["n_clipped_z"] == st["n_points"]
    zero = [r for r in rays if [o >> 10 for o in r[0]] == [e >> 10 for e in r[1]]]
    assert len(zero) >= 5
    cells, hits, misses, lo, stats = OR.occupancy_ref(clouds, poses, P)
    assert (cells < 0).any(0).all()                                            # negative cells on every axis
    assert stats["n_bricks"] > 8 and stats["n_cells"] == len(cells) and stats["n_steps"] == hits.sum() + misses.sum()
    for a in range(3):                                                         # rays that cross brick borders on every axis
        assert any((r[0][a] >> 13) != (r[1][a] >> 13) for r in rays)
    raw = hits.astype(np.float32) * P["l_hit"] + misses.astype(np.float32) * P["l_miss"]
    assert (raw < P["l_min"]).any() and (raw > P["l_max"]).any()                # both clamps bite
    assert (lo == P["l_min"]).any() and (lo == P["l_max"]).any() and ((lo > P["l_min"]) & (lo < P["l_max"])).any()
    # a cell that one cloud hits and another only misses
    per = [OR.occupancy_ref([c], [T], P) for c, T in zip(clouds, poses)]
    hit_by = [set(map(tuple, p[0][p[1] > 0].tolist())) for p in per]
    missed_only_by = [set(map(tuple, p[0][(p[1] == 0) & (p[2] > 0)].tolist())) for p in per]
    assert any(hit_by[a] & missed_only_by[b] for a in range(len(per)) for b in range(len(per)) if a != b)
    shared = set.intersection(*[set(map(tuple, p[0].tolist())) for p in per[:3]])
    assert len(shared) >= 7                                                    # three clouds share cells


def test_vectorised_reference_is_the_restatement(lattice):
    clouds, poses, P = lattice[:3]
    cases = [(clouds, poses, dict(P, emit=e)) for e in (0, 1, 2)]
    gc, gp, max_range = OR.generic_case()
    cases += [(gc, gp, OR.default_params(resolution=r, max_range=max_range, sensor_origin=OR.GENERIC_ORIGIN)) for r in (0.05, 0.37)]
    for cl, ps, Q in cases:
        a, b = OR.occupancy_ref(cl, ps, Q), OR.occupancy_ref_vec(cl, ps, Q)
        for x, y in zip(a[:4], b[:4]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert a[4] == b[4]


def test_emit_modes_partition(lattice):
    clouds, poses, P = lattice[:3]
    every, occ, free = (OR.occupancy_ref(clouds, poses, dict(P, emit=e)) for e in (0, 1, 2))
    assert len(occ[0]) > 0 and len(free[0]) > 0 and len(occ[0]) + len(free[0]) == len(every[0])
    assert (occ[3] >= P["l_occ"]).all() and (free[3] < P["l_occ"]).all()
    assert every[4]["n_cells"] == occ[4]["n_cells"] == free[4]["n_cells"] == len(every[0])


def test_far_rays_are_refused():
    clouds, poses = OR.far_case()
    with pytest.raises(OR.Unsupported):
        OR.occupancy_ref([np.array([[30000.0, 0, 0]], np.float32)], poses[:1], OR.default_params(resolution=0.05, max_range=10))
    cells = OR.occupancy_ref(clouds, poses, OR.default_params(resolution=0.01))[0]
    assert (cells.max(0) - cells.min(0))[:2].min() > 8 * 20000                 # the box of bricks the GPU test expects to be refused


# ---- the host side of the C-ABI: what answers without a GPU ----------------------------------------------------------------------------
def test_default_params_and_argument_errors(hip_lib):
    import ctypes as C
    from semantic_slam_amd import SslamError
    from semantic_slam_amd._lib import OccParams
    from semantic_slam_amd.segmentation import PointCloudSegmentation, occupancy_default_params, pack_clouds
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM
    p, d = occupancy_default_params(), OR.default_params()
    for k in ("resolution", "max_range", "z_min", "z_max", "l_hit", "l_miss", "l_min", "l_max", "l_occ"):
        assert np.float32(getattr(p, k)).tobytes() == d[k].tobytes(), k        # the same floats on both sides
    assert list(p.sensor_origin) == [0.0, 0.0, 0.0] and p.emit == 0 and C.sizeof(OccParams) == 52
    seg = PointCloudSegmentation()
    xyz, start, T = pack_clouds([np.ones((3, 3), np.float32), np.zeros((2, 3), np.float32)], [OR.identity_pose(), OR.identity_pose()])

    def call(q, start=start, T=T, max_out=0):
        return hip_lib.sslam_seg_occupancy_map(seg._h, xyz.ctypes.data, start.ctypes.data, 2, T.ctypes.data, None if q is None else C.byref(q),
                                               None, None, None, None, max_out, None)
    for field, v in (("resolution", 0.0), ("resolution", np.nan), ("max_range", -1.0), ("max_range", 6000.0), ("l_hit", 0.0), ("l_miss", 0.0),
                     ("l_min", 9.0), ("z_min", 9.0), ("emit", 3)):
        q = occupancy_default_params()
        setattr(q, field, v)
        assert call(q) == OR.INVALID, field                                     # refused before the device is looked for
    assert call(None) == OR.INVALID and call(p, max_out=-1) == OR.INVALID
    assert call(p, start=np.array([0, 3, 2], np.int32)) == OR.INVALID
    Tb = T.copy(); Tb[1, 3] = np.inf
    assert call(p, T=Tb) == OR.INVALID and b"pose of cloud 1" in hip_lib.sslam_last_error()
    assert call(p) == (OR.NO_DEVICE if hip_lib.sslam_device_count() == 0 else 4)   # valid arguments reach the device
    ms = np.ones(4)
    assert hip_lib.sslam_seg_last_occupancy_timing(seg._h, ms.ctypes.data) == 0 and (ms >= 0).all()
    assert hip_lib.sslam_seg_last_occupancy_timing(None, ms.ctypes.data) == OR.INVALID
    # the tick's entry: nothing kept -> 0 without touching the device, the argument rules first
    S = SemanticGraphSLAM(None, seg)
    S.set_map_clouds(True, 0.3)
    out = S.occupancy_map()
    assert all(len(a) == 0 for a in out[:4]) and out[4].n_clouds == 0 and out[4].upload_bytes == 0
    q = occupancy_default_params()
    q.emit = -1
    with pytest.raises(SslamError):
        S.occupancy_map(q)
    assert hip_lib.sslam_slam_occupancy_map(None, C.byref(p), None, None, None, None, 0, None) == OR.INVALID
    assert hip_lib.sslam_slam_occupancy_map(S._h, None, None, None, None, None, 0, None) == OR.INVALID


def test_cpp_shim_compiles_and_refuses_on_the_host(hip_lib, tmp_path):
    """tests/shim_occupancy_check.cpp without a recording: the shim headers compile and link, and the host-side refusals hold"""
    import os
    import subprocess
    from semantic_slam_amd import library_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_occupancy")
    libdir = os.path.dirname(library_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(root, "tests", "shim_occupancy_check.cpp"), "-o", exe,
                           "-L" + libdir, "-lsslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "shim occupancy ok" in out.stdout, out.stdout + out.stderr
