"""bench.py --dump-outputs on the host side (no GPU: a stand-in for the device batch): float64 .npy files within 64 MB, the same seeded
sample of graphs every run, and the workload's edge counts read back from a .g2o file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _HostBatch:
    """the part of GraphBatch that dump_outputs uses; the estimates stay those of the host graphs"""

    def __init__(self, graphs):
        self.graphs, self.downloads = graphs, 0

    def download(self):
        self.downloads += 1


def _graphs(hip_lib, n):
    from semantic_slam_amd import GraphSLAM
    from semantic_slam_amd.synth import make_graph
    return [GraphSLAM.from_synth(make_graph(60, 12, seed=s)) for s in range(n)]


def test_dump_outputs_float64_seeded_sample_within_64mb(hip_lib, tmp_path):
    from semantic_slam_amd._lib import OptStats
    graphs = _graphs(hip_lib, bench.DUMP_GRAPHS + 8)
    stats = [OptStats(iterations=k % 7, trials=k % 7 + 1, status=k % 2, chi2_before=10.0 + k, chi2_after=1.0 + k) for k in range(len(graphs))]
    b = _HostBatch(graphs)
    bench.dump_outputs(str(tmp_path / "a"), b, stats)
    bench.dump_outputs(str(tmp_path / "b"), _HostBatch(graphs), stats)
    assert b.downloads == 1
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert {"chi2_after.npy", "iterations.npy", "trials.npy", "status.npy", "estimates.npy", "estimates_graph_index.npy"} <= set(files)
    total = 0
    for f in files:
        a, c = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, c), f
        total += os.path.getsize(tmp_path / "a" / f)
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "chi2_after.npy"), [s.chi2_after for s in stats])
    pick = np.load(tmp_path / "a" / "estimates_graph_index.npy").astype(int)
    est = np.load(tmp_path / "a" / "estimates.npy")
    assert len(pick) == bench.DUMP_GRAPHS and len(set(pick)) == len(pick) and est.shape == (len(pick), 72, 7)
    for k, g in enumerate(pick):
        assert np.array_equal(est[k], graphs[g].estimates())


def test_edge_counts_of_a_saved_graph(hip_lib, tmp_path):
    g = _graphs(hip_lib, 1)[0]
    path = str(tmp_path / "g.g2o")
    g.save(path)
    from semantic_slam_amd.synth import make_graph
    s = make_graph(60, 12, seed=0)
    assert bench.edge_counts(path) == (len(s.odom_ij), len(s.lm_ij))


def test_scalar_pose_compose_is_bit_identical_to_pose_compose():
    from semantic_slam_amd.synth import _pose_compose_scalar, pose_compose, quat_from_rotvec
    rng = np.random.default_rng(11)
    a = np.concatenate([rng.normal(0, 5, (500, 3)), quat_from_rotvec(rng.normal(0, 1, (500, 3)))], axis=1)
    b = np.concatenate([rng.normal(0, 0.3, (500, 3)), quat_from_rotvec(rng.normal(0, 0.1, (500, 3)))], axis=1)
    for x, y in zip(a, b):
        assert np.array_equal(np.array(_pose_compose_scalar(x.tolist(), y.tolist())), pose_compose(x, y))


def test_from_synth_matches_the_per_call_construction(hip_lib, tmp_path):
    """GraphSLAM.from_synth (bulk) builds the graph the public add_* calls build: the same .g2o bytes"""
    from semantic_slam_amd import GraphSLAM
    from semantic_slam_amd.synth import make_graph
    for kind in ("point", "plane"):
        g = make_graph(80, 15, seed=4, landmark_kind=kind)
        H = GraphSLAM()
        for i in range(g.n_poses):
            H.add_se3_node(g.poses_init[i])
        for lm in g.lms_init:
            (H.add_plane_node if kind == "plane" else H.add_point_xyz_node)(lm)
        for (i, j), z, w in zip(g.odom_ij, g.odom_z, g.odom_info):
            H.add_se3_edge(int(i), int(j), z, w)
        for (i, l), z, w in zip(g.lm_ij, g.lm_z, g.lm_info):
            (H.add_se3_plane_edge if kind == "plane" else H.add_se3_point_xyz_edge)(int(i), g.n_poses + int(l), z, w)
        a, b = str(tmp_path / f"bulk_{kind}.g2o"), str(tmp_path / f"calls_{kind}.g2o")
        GraphSLAM.from_synth(g).save(a)
        H.save(b)
        assert open(a).read() == open(b).read()
