#!/usr/bin/env python3
"""Scan matching (sslam_seg_register_pairs: per iteration a reset, k_nn_pairs, k_reg_sums, k_reg_step; one fitness pass at the end), timed on
the GPU at the size of one tick's loop candidates: 8 pairs of 4 000 x 4 000 points (the workload tools/fitness_timing.py times the fitness
pass at), the source of every pair the same scene seen from a pose 0.05 rad and 0.1 m away, registered from the identity with epsilon = 0.

The time is the hipEvent time the call reports: from the first reset to the end of the final fitness pass, the host's reads of the
unfinished-pair counter (one per chunk of 8 iterations) included, the copies of the clouds excluded.  After one warm-up call the MEDIAN OF
FIVE calls is reported with the range, the iterations every pair took, and the number of passes the call enqueued (iterations are enqueued 8
at a time, so the call runs to the next multiple of 8 after the last pair finishes).  Results are checked to repeat bitwise.  Prints one
JSON line; needs a GPU (there is no CPU fallback).

  python tools/registration_timing.py [--pairs 8] [--points 4000] [--max-iterations 64]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fitness_timing import moved, scene  # noqa: E402

REPEATS = 5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--max-iterations", type=int, default=64)
    args = ap.parse_args()
    from semantic_slam_amd import load_library
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    if load_library().sslam_device_count() < 1:
        sys.exit("registration_timing.py needs a GPU: the product has no CPU fallback")
    rng = np.random.default_rng(0)
    seg = PointCloudSegmentation()
    c, s = np.cos(0.05), np.sin(0.05)
    T = np.array([c, -s, 0, s, c, 0, 0, 0, 1, 0.08, 0.06, 0.0])
    clouds = [scene(rng, args.points)]
    for _ in range(args.pairs):
        clouds.append(moved(rng, clouds[-1], T))
    pairs = [(k, k + 1, None, None) for k in range(args.pairs)]
    first = seg.register_pairs(clouds, pairs, max_iterations=args.max_iterations)      # warm-up, and the results every repeat must give again
    times = []
    for _ in range(REPEATS):
        res = seg.register_pairs(clouds, pairs, max_iterations=args.max_iterations)
        assert all(a.T.tobytes() == b.T.tobytes() and a.score == b.score and a.iterations == b.iterations for a, b in zip(res, first)), "the results do not repeat"
        times.append(seg.last_registration_ms)
    iterations = [r.iterations for r in first]
    passes = min(args.max_iterations, -(-max(iterations) // 8) * 8)
    ms = statistics.median(times)
    err = [float(np.abs(r.T - T).max()) for r in first]
    fit = seg.fitness_scores(clouds, [(k, k + 1, first[k].T, None) for k in range(args.pairs)])
    fitness_ms = seg.last_fitness_ms
    print(json.dumps({"workload": f"{args.pairs} pairs of {args.points} x {args.points}", "loop_ms_median_of_5": round(ms, 4),
                      "loop_ms_all": [round(t, 4) for t in times], "iterations": iterations, "converged": [r.converged for r in first],
                      "passes_enqueued": passes, "ms_per_pass": round(ms / (passes + 1), 4), "one_fitness_pass_ms": round(fitness_ms, 4),
                      "largest_entry_error_vs_true_motion": [round(e, 5) for e in err], "scores": [float(r.score) for r in first[:4]],
                      "scores_equal_fitness_call": bool(all(first[k].score == fit[0][k] for k in range(args.pairs)))}), flush=True)


if __name__ == "__main__":
    main()
