"""What a frame of scan-matching odometry costs: sslam_odom_push, where the frame goes up once and stays on the device from the raw cloud
to the 12 doubles of the pose, next to the same frames through the COMPOSITION of the host-pointer entry points (distance filter, gather,
voxel grid, statistical outlier removal, gather, cloud covariances of the frame, register_pairs_gicp of keyframe and frame with both
covariance sets handed over), each of which uploads its input, waits and downloads its output.  Both run the decision rule of
include/sslam.h on the same frames of tests/odom_scene.py (the dense trajectory in the room of tests/loop_scene.py) with the default
parameters: distance filter 1 .. 100 m, leaf 0.1, statistical stage 20 / 1.0, GICP.  The composition reuses a keyframe's covariances as the
handle does (they are computed once, when the frame arrives); what it cannot avoid is the traffic.  Prints ms per frame: push split by
the four times of sslam_odom_stats plus the wall time seen from Python, and the composition's wall time, at 96 x 72 and 640 x 480 raw
points, after one warm-up pass over the frames.  Both paths must give the same poses bit for bit, which is checked.
usage (GPU box): python tools/odometry_timing.py [--frames 12] [--repeat 5] [--leaf 0.1]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.1)
    a = ap.parse_args()
    from semantic_slam_amd import load_library
    if load_library().sslam_device_count() < 1:
        sys.exit("odometry_timing: no HIP device is visible; the library has no CPU fallback, so there is nothing to time here")
    import loop_scene as LS
    import odom_ref as R
    import odom_scene as S
    from semantic_slam_amd.odometry import ScanMatchingOdometry
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    seg = PointCloudSegmentation()

    class Composition(R.Odometry):
        """the rule of sslam_odom_push over the host-pointer entry points"""

        def __init__(self):
            super().__init__(prepare=self.prep, match=self.dev_match)

        def prep(self, cloud):
            cur = cloud[seg.distance_filter(cloud, 1.0, 100.0)]
            cur = seg.downsamplePointcloud(cur, a.leaf)[0]
            if len(cur) >= 21:
                cur = cur[seg.removeOutliers(cur, 20, 1.0)[0]]
            cur = np.ascontiguousarray(cur)
            return cur, seg.cloud_covariances([cur], 20, 1e-3)[0]

        def dev_match(self, key, frame, T0):
            r = seg.register_pairs_gicp([key[0], frame[0]], [(0, 1, T0, 2.5 * 2.5)], covariances=[key[1], frame[1]], max_iterations=64, epsilon=0.01)[0]
            return r.T, r.iterations, r.converged, r.status

    print(f"{a.frames} frames, leaf {a.leaf}, GICP (k 20), one warm-up pass, then {a.repeat} passes; ms per frame, mean (min .. max over the passes)")
    for width, height in ((96, 72), (640, 480)):
        LS.WIDTH, LS.HEIGHT = width, height
        S._CACHE.clear()
        _, clouds = S.frames(a.frames)
        stamps = [S.stamp(k) for k in range(a.frames)]
        od = ScanMatchingOdometry(seg, leaf=a.leaf)
        rows, comp_ms, push_ms, poses = [], [], [], None
        for rep in range(a.repeat + 1):
            od.reset()
            t0 = time.perf_counter()
            out = [od.push(c, s) for c, s in zip(clouds, stamps)]
            t_push = (time.perf_counter() - t0) * 1e3 / a.frames
            comp = Composition()
            t0 = time.perf_counter()
            ref = [comp.push(c, s) for c, s in zip(clouds, stamps)]
            t_comp = (time.perf_counter() - t0) * 1e3 / a.frames
            for (pose, st), (want, rec) in zip(out, ref):
                assert pose.tobytes() == want.tobytes() and st.new_keyframe == rec["new_keyframe"], "the two paths disagree"
            if rep == 0:
                continue
            push_ms.append(t_push); comp_ms.append(t_comp)
            rows.append([np.mean([getattr(st, f) for _, st in out]) for f in ("prefilter_ms", "covariance_ms", "registration_ms", "total_ms")])
        rows = np.array(rows)
        st = out[-1][1]
        print(f"{width} x {height} = {width * height} raw points, {np.mean([s.n_filtered for _, s in out]):.0f} after the prefilter, "
              f"{st.keyframes} keyframes, {np.mean([s.iterations for _, s in out[1:]]):.1f} iterations per match")
        for name, col in (("push: prefilter (hipEvents)", rows[:, 0]), ("push: covariances (hipEvents)", rows[:, 1]),
                          ("push: registration (hipEvents)", rows[:, 2]), ("push: whole call (wall, in C)", rows[:, 3]),
                          ("push: seen from Python (wall)", np.array(push_ms)), ("composition of the host entry points (wall, from Python)", np.array(comp_ms))):
            print(f"  {name:58s} {col.mean():8.3f} ({col.min():.3f} .. {col.max():.3f})")
        print(f"  upload per frame: push {12 * width * height} B; composition {12 * width * height} B raw + the intermediate clouds three more times + "
              f"the keyframe cloud and both covariance sets per match")
        print(f"  composition / push: {np.mean(comp_ms) / np.mean(push_ms):.2f}")


if __name__ == "__main__":
    main()
