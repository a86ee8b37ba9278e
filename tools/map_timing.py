"""What a map costs: sslam_seg_map_cloud on 1, 64 and 1024 synthetic clouds of 4096 points each.  The poses lie along a 200 m loop (a
circle, the keyframes facing along it); every cloud holds points of two world planes (floor z = 0, ceiling z = 3) in an 8 m x 8 m patch
ahead of its pose, expressed in the pose's frame, so neighbouring clouds share voxels.  Resolution 0.05.
Prints, per size: the hipEvent time of each of the four passes (min / max, bricks, accumulate, voxels + records) and their sum, the wall
time of the call (staging of the host clouds and the copies back included), the time of tests/map_ref.py's NumPy restatement on the same
input, and whether the two agree bit for bit.  Each size runs in a child process of its own under `timeout`; the first failure ends the run.
usage (GPU box): python tools/map_timing.py [--sizes 1 64 1024] [--points 4096] [--resolution 0.05] [--repeats 5] [--limit 300]"""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOOP_M = 200.0


def scene(n_clouds, n_points, seed=0):
    rng = np.random.default_rng(seed)
    radius = LOOP_M / (2 * math.pi)
    clouds, poses = [], []
    for k in range(n_clouds):
        a = 2 * math.pi * k / max(n_clouds, 1)
        yaw = a + 0.5 * math.pi
        c, s = math.cos(yaw), math.sin(yaw)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        t = np.array([radius * math.cos(a), radius * math.sin(a), 1.2])
        local = np.stack([rng.uniform(0.0, 8.0, n_points), rng.uniform(-4.0, 4.0, n_points), np.zeros(n_points)], 1)
        world = local @ R.T + t
        world[:, 2] = np.where(rng.random(n_points) < 0.5, 0.0, 3.0)
        clouds.append(((world - t) @ R).astype(np.float32))
        poses.append(np.concatenate([R.reshape(-1), t]))
    return clouds, poses


def one_size(n_clouds, n_points, resolution, repeats):
    import map_ref as MR
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    clouds, poses = scene(n_clouds, n_points)
    seg = PointCloudSegmentation()
    seg.map_cloud(clouds, poses, resolution)                                   # warm-up: the first launches, the allocator
    rows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        xyz, counts, cells, st = seg.map_cloud(clouds, poses, resolution, return_cells=True)
        rows.append(np.concatenate([[1e3 * (time.perf_counter() - t0)], seg.last_map_timing()]))
    r = np.median(np.array(rows), 0)
    t0 = time.perf_counter()
    wx, wc, wk, _ = MR.map_ref(clouds, poses, resolution)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    same = np.array_equal(cells, wk) and np.array_equal(counts, wc) and xyz.tobytes() == wx.tobytes()
    print(f"clouds {n_clouds:5d} points {st.n_points:8d} bricks {st.n_bricks:7d} voxels {st.n_voxels:8d} | kernels {r[1:].sum():8.3f} ms = minmax {r[1]:7.3f}"
          f" + bricks {r[2]:7.3f} + accumulate {r[3]:7.3f} + voxels {r[4]:7.3f} | call {r[0]:9.3f} ms | numpy reference {ref_ms:10.1f} ms |"
          f" {'bitwise equal' if same else 'DIFFERENT'} (median of {repeats})", flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        sys.exit(one_size(a.child, a.points, a.resolution, a.repeats))
    for n in a.sizes:                                                          # a fresh process per size, each under its own time limit
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--points", str(a.points),
                              "--resolution", str(a.resolution), "--repeats", str(a.repeats)])
        if rc != 0:
            print(f"size {n}: exit status {rc}; stopping")
            sys.exit(rc)


if __name__ == "__main__":
    main()
