"""What an occupancy map costs: sslam_seg_occupancy_map on 1, 64 and 1024 synthetic clouds of 4096 points each, at the default parameters
(resolution 0.05, max_range 10, z -1 .. 5: the reference's octomap_server launch).  The scene is tools/map_timing.py's: poses along a 200 m
loop, every cloud points of two world planes (floor z = 0, ceiling z = 3) in an 8 m x 8 m patch ahead of its pose; the sensor sits at the
pose, 1.2 m up, so a ray is 1.2 to about 9 m long.
Prints, per size: the hipEvent time of each of the four passes (box, bricks, accumulate, cells + records) and their sum, n_steps (the cells
visited = the integer atomics of the accumulate pass) and their rate in that pass, the wall time of the call that fetches the records (the
staging of the host clouds and the copies back included), the time of tests/occupancy_ref.py's NumPy restatement on the same input, and
whether the two agree bit for bit.  Each size runs in a child process of its own under `timeout`; the first failure ends the run.
With --scans every size prints two rows from one process: the ray entry's as above (without its reference), then sslam_seg_occupancy_map_scans
on the same scene -- box, bricks, mark, fold, cells + records, the cells the mark launches visit per second, the share of them that needed
the atomic OR, the (scan, cell) updates, the call -- checked against tests/occupancy_scan_ref.py's scan_ref_vec.  --no-reference skips that
check (for comparing builds of the kernels).
usage (GPU box): python tools/occupancy_timing.py [--scans [--no-reference]] [--sizes 1 64 1024] [--points 4096] [--repeats 5] [--limit 900]"""
import argparse
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def in_thread(reference, n_clouds):
    """reference() in a worker thread (minutes at 1024 clouds: a line a minute says it is alive) -> (its result or None, milliseconds)"""
    t0 = time.perf_counter()
    box = []
    worker = threading.Thread(target=lambda: box.append(reference()))
    worker.start()
    while worker.is_alive():
        worker.join(60.0)
        if worker.is_alive():
            print(f"  ... the NumPy reference of {n_clouds} clouds is at {time.perf_counter() - t0:.0f} s", flush=True)
    return (box[0] if box else None), 1e3 * (time.perf_counter() - t0)


def same_as(got, want):
    cells, hits, misses, lo, st = got
    wc, wh, wm, wl, wst = want
    return (np.array_equal(cells, wc) and np.array_equal(hits, wh) and np.array_equal(misses, wm) and lo.tobytes() == wl.tobytes()
            and all(getattr(st, k) == v for k, v in wst.items()))


def one_size_scans(n_clouds, n_points, repeats, reference):
    import occupancy_ref as OR
    import occupancy_scan_ref as SR
    from map_timing import scene
    from semantic_slam_amd.segmentation import PointCloudSegmentation, occupancy_default_params
    clouds, poses = scene(n_clouds, n_points)
    seg = PointCloudSegmentation()
    p = occupancy_default_params()
    med = {}
    for name, call in (("rays", seg.occupancy_map), ("scans", seg.occupancy_map_scans)):
        call(clouds, poses, p)                                                 # warm-up: the first launches, the allocator; it also counts
        cap = seg.last_occupancy_count
        rows = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            got = call(clouds, poses, p, max_out=cap)
            rows.append(np.concatenate([[1e3 * (time.perf_counter() - t0)], seg.last_occupancy_timing(), seg.last_occupancy_scan_timing()]))
        med[name] = (np.median(np.array(rows), 0), got)
    r, got = med["rays"]
    st = got[4]
    print(f"clouds {n_clouds:5d} rays {st.n_rays:8d} truncated {st.n_truncated:6d} bricks {st.n_bricks:7d} cells {st.n_cells:9d} steps {st.n_steps:11d} |"
          f" kernels {r[1:5].sum():8.3f} ms = box {r[1]:7.3f} + bricks {r[2]:7.3f} + accumulate {r[3]:8.3f} + cells {r[4]:7.3f} |"
          f" {st.n_steps / (1e6 * r[3]):7.2f} G atomics/s in accumulate | call {r[0]:9.3f} ms | the ray entry (median of {repeats})", flush=True)
    r, got = med["scans"]
    st = got[4]
    visited, issued = seg.last_occupancy_scan_counts()                         # of the last repeat: the share varies a little from run to run
    verdict = "not checked"
    if reference:
        want, ref_ms = in_thread(lambda: SR.scan_ref_vec(clouds, poses, OR.default_params()), n_clouds)
        if want is None:
            print("the NumPy reference failed")
            return 1
        verdict = f"numpy reference {ref_ms:10.1f} ms | {'bitwise equal' if same_as(got, want) else 'DIFFERENT'}"
    print(f"clouds {n_clouds:5d} by scans: cells {st.n_cells:9d} updates {st.n_steps:11d} marks {visited:11d} |"
          f" kernels {r[1:5].sum():8.3f} ms = box {r[1]:7.3f} + bricks {r[2]:7.3f} + mark {r[5]:8.3f} + fold {r[6]:8.3f} + cells {r[4]:7.3f} |"
          f" {visited / (1e6 * r[5]):7.2f} G marks/s | {100.0 * issued / max(visited, 1):5.1f} % of the marks issued the atomic |"
          f" call {r[0]:9.3f} ms | {verdict} (median of {repeats})", flush=True)
    return 1 if "DIFFERENT" in verdict else 0


def one_size(n_clouds, n_points, repeats):
    import occupancy_ref as OR
    from map_timing import scene
    from semantic_slam_amd.segmentation import PointCloudSegmentation, occupancy_default_params
    clouds, poses = scene(n_clouds, n_points)
    seg = PointCloudSegmentation()
    p = occupancy_default_params()
    seg.occupancy_map(clouds, poses, p)                                        # warm-up: the first launches, the allocator; it also counts
    cap = seg.last_occupancy_count
    rows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cells, hits, misses, lo, st = seg.occupancy_map(clouds, poses, p, max_out=cap)
        rows.append(np.concatenate([[1e3 * (time.perf_counter() - t0)], seg.last_occupancy_timing()]))
    r = np.median(np.array(rows), 0)
    want, ref_ms = in_thread(lambda: OR.occupancy_ref_vec(clouds, poses, OR.default_params()), n_clouds)
    if want is None:
        print("the NumPy reference failed")
        return 1
    same = same_as((cells, hits, misses, lo, st), want)
    print(f"clouds {n_clouds:5d} rays {st.n_rays:8d} truncated {st.n_truncated:6d} bricks {st.n_bricks:7d} cells {st.n_cells:9d} steps {st.n_steps:11d} |"
          f" kernels {r[1:].sum():8.3f} ms = box {r[1]:7.3f} + bricks {r[2]:7.3f} + accumulate {r[3]:8.3f} + cells {r[4]:7.3f} |"
          f" {st.n_steps / (1e6 * r[3]):7.2f} G atomics/s in accumulate | call {r[0]:9.3f} ms | numpy reference {ref_ms:10.1f} ms |"
          f" {'bitwise equal' if same else 'DIFFERENT'} (median of {repeats})", flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds a size may take (most of it is the NumPy reference)")
    ap.add_argument("--scans", action="store_true", help="time sslam_seg_occupancy_map_scans next to the ray entry")
    ap.add_argument("--no-reference", action="store_true", help="with --scans: skip the NumPy reference")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        sys.exit(one_size_scans(a.child, a.points, a.repeats, not a.no_reference) if a.scans else one_size(a.child, a.points, a.repeats))
    mode = (["--scans"] if a.scans else []) + (["--no-reference"] if a.no_reference else [])
    for n in a.sizes:                                                          # a fresh process per size, each under its own time limit
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--points", str(a.points),
                              "--repeats", str(a.repeats)] + mode)
        if rc != 0:
            print(f"size {n}: exit status {rc}; stopping")
            sys.exit(rc)


if __name__ == "__main__":
    main()
