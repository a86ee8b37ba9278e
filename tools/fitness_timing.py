#!/usr/bin/env python3
"""Fitness-score pass (sslam_seg_fitness_scores: k_nn_pairs + k_nn_finish), timed on the GPU at two sizes:

  downsampled   8 pairs of 4 000 x 4 000 points: the voxel-downsampled keyframe clouds of one tick, all pairs in one launch;
  full frame    one pair of 307 200 x 307 200 points: two raw 640 x 480 frames against each other.

The time is the hipEvent time the call reports (the memset of the result table and the two kernels; copies excluded).  After one warm-up
call per workload the MEDIAN OF FIVE calls is reported, next to the arithmetic of the pass: (query, target) distance evaluations, the
rate they were made at, and the ~11 VALU operations each costs as a share of the fp32 vector peak the caller names (--peak-tflops; see
DESIGN.md section 4 for the figure used there).  Scores are checked to repeat bitwise.  Prints one JSON line per workload; needs a GPU
(there is no CPU fallback).

  python tools/fitness_timing.py [--skip-full] [--peak-tflops 157.3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPEATS = 5
OPS_PER_EVALUATION = 11      # three subtractions, three products, two sums, one compare, two selects


def scene(rng, n):
    """n points on a floor, a wall and some clutter, 6 m x 4 m x 2.5 m: what a downsampled indoor cloud looks like"""
    k = n // 3
    floor = np.stack([rng.uniform(-3, 3, k), rng.uniform(0, 4, k), rng.normal(0, 0.01, k)], 1)
    wall = np.stack([rng.uniform(-3, 3, k), 4 + rng.normal(0, 0.01, k), rng.uniform(0, 2.5, k)], 1)
    rest = np.stack([rng.uniform(-3, 3, n - 2 * k), rng.uniform(0, 4, n - 2 * k), rng.uniform(0, 1.0, n - 2 * k)], 1)
    return np.concatenate([floor, wall, rest]).astype(np.float32)


def moved(rng, cloud, T):
    """the same scene seen from the other pose (source = T^-1 target) with sensor noise, in another point order"""
    R, t = T[:9].reshape(3, 3), T[9:]
    p = (cloud.astype(np.float64) - t) @ R + rng.normal(0, 0.005, cloud.shape)
    return rng.permutation(p.astype(np.float32))


def measure(seg, name, clouds, pairs, peak_tflops):
    first = seg.fitness_scores(clouds, pairs)                                    # warm-up, and the scores every repeat must give again
    times = []
    for _ in range(REPEATS):
        score, used = seg.fitness_scores(clouds, pairs)
        assert score.tobytes() == first[0].tobytes() and np.array_equal(used, first[1]), f"{name}: the scores do not repeat"
        times.append(seg.last_fitness_ms)
    evals = float(sum(len(clouds[t]) * len(clouds[s]) for t, s, _, _ in pairs))
    ms = statistics.median(times)
    out = {"workload": name, "pairs": len(pairs), "evaluations": evals, "kernel_ms_median_of_5": round(ms, 4), "kernel_ms_all": [round(t, 4) for t in times],
           "evaluations_per_second": evals / (ms * 1e-3), "valu_ops_per_evaluation": OPS_PER_EVALUATION,
           "share_of_fp32_vector_peak": OPS_PER_EVALUATION * evals / (ms * 1e-3) / (peak_tflops * 1e12), "peak_tflops_assumed": peak_tflops,
           "scores": [float(s) for s in first[0][:4]], "used": [int(u) for u in first[1][:4]]}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--skip-full", action="store_true")
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32 vector peak the share is taken of")
    args = ap.parse_args()
    from semantic_slam_amd import load_library
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    if load_library().sslam_device_count() < 1:
        sys.exit("fitness_timing.py needs a GPU: the product has no CPU fallback")
    rng = np.random.default_rng(0)
    seg = PointCloudSegmentation()
    c, s = np.cos(0.05), np.sin(0.05)
    T = np.array([c, -s, 0, s, c, 0, 0, 0, 1, 0.5, 0.02, 0.0])
    clouds = [scene(rng, 4000)]
    for _ in range(8):
        clouds.append(moved(rng, clouds[-1], T))
    measure(seg, "8 pairs of 4000 x 4000", clouds, [(k, k + 1, T, None) for k in range(8)], args.peak_tflops)
    if not args.skip_full:
        a = scene(rng, 307200)
        measure(seg, "1 pair of 307200 x 307200", [a, moved(rng, a, T)], [(0, 1, T, None)], args.peak_tflops)


if __name__ == "__main__":
    main()
