"""What generalized ICP costs next to point-to-point ICP: keyframe clouds of the replay of tests/loop_scene.py, voxel-downsampled, each
registered against its neighbour on the track with both matchers, on the same build and the same pairs.  Prints the hipEvent time of the
covariance pass (sslam_seg_cloud_covariances: k_knn_cov over all clouds of the call) per call and per cloud, and of ICP and GICP per
iteration: a call capped at N iterations takes N passes of search + sums + step and one final fitness pass, so the time of one iteration
is (t(N2) - t(N1)) / (N2 - N1) with epsilon = 0, where no pair stops early; the covariances are handed to the GICP calls ready made.
usage (GPU box): python tools/gicp_timing.py [--clouds 16] [--width 96] [--height 72] [--leaf 0.1] [--k 20] [--repeat 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=72)
    ap.add_argument("--leaf", type=float, default=0.1)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import loop_scene as LS
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    LS.WIDTH, LS.HEIGHT = a.width, a.height
    events = LS.make_events(a.clouds)
    seg = PointCloudSegmentation()
    clouds = [seg.downsamplePointcloud(ev.cloud.xyz(), a.leaf)[0] for ev in events]
    pairs = [(k + 1, k, None, None) for k in range(len(clouds) - 1)]     # the next keyframe's cloud is the target, as in the tick
    sizes = [len(c) for c in clouds]
    print(f"{len(clouds)} clouds of {min(sizes)} .. {max(sizes)} points (leaf {a.leaf}), {len(pairs)} pairs, k {a.k}")

    def best(f):
        return min(f() for _ in range(a.repeat + 1))                      # the first call warms the device up

    def cov_ms():
        seg.cloud_covariances(clouds, k=a.k)
        return seg.last_covariance_ms
    t_cov = best(cov_ms)
    print(f"covariances: {t_cov:8.3f} ms per call, {t_cov / len(clouds):7.3f} ms per cloud")
    covs = seg.cloud_covariances(clouds, k=a.k)
    n1, n2 = 4, 12
    per = {}
    for name, run in (("ICP", lambda n: seg.register_pairs(clouds, pairs, max_iterations=n, epsilon=0.0)),
                      ("GICP", lambda n: seg.register_pairs_gicp(clouds, pairs, covariances=covs, k=a.k, max_iterations=n, epsilon=0.0))):
        t = {}
        for n in (n1, n2):
            def ms(n=n):
                res = run(n)
                assert all(r.iterations == n or r.status != 0 or r.converged for r in res)
                return seg.last_registration_ms
            t[n] = best(ms)
        per[name] = (t[n2] - t[n1]) / (n2 - n1)
        print(f"{name:5s} {t[n1]:8.3f} ms at {n1} iterations, {t[n2]:8.3f} ms at {n2}: {per[name]:7.3f} ms per iteration of {len(pairs)} pairs")
    full = {name: best(lambda f=f: (f(), seg.last_registration_ms)[1]) for name, f in
            (("ICP", lambda: seg.register_pairs(clouds, pairs, max_iterations=64, epsilon=1e-6)),
             ("GICP", lambda: seg.register_pairs_gicp(clouds, pairs, covariances=covs, k=a.k, max_iterations=64, epsilon=1e-6)))}
    it = {"ICP": seg.register_pairs(clouds, pairs, max_iterations=64, epsilon=1e-6), "GICP": seg.register_pairs_gicp(clouds, pairs, covariances=covs, k=a.k, max_iterations=64, epsilon=1e-6)}
    for name in ("ICP", "GICP"):
        print(f"{name:5s} to epsilon 1e-6: {full[name]:8.3f} ms, {max(r.iterations for r in it[name])} iterations at most, mean score {np.mean([r.score for r in it[name]]):.5f}")
    print(f"GICP / ICP per iteration {per['GICP'] / per['ICP']:.2f}; covariances of one new cloud / one GICP iteration {t_cov / len(clouds) / per['GICP']:.2f}")


if __name__ == "__main__":
    main()
