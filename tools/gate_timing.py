#!/usr/bin/env python3
"""Loop-closure gate: two ways of computing the same d2 = e^T S^-1 e of N candidate edges, timed on the GPU.

  gate        GraphBatch.gate of the N candidates: one linearisation, one flat factorisation, one wave per candidate that walks path(u)
              and path(v) once each; 43 doubles per candidate come back.
  marginals   what a caller did before the gate existed: GraphBatch.marginals with the 3N requests (u,u), (u,v), (v,v) -- the same
              linearisation and factorisation, three waves per candidate that walk path(u) twice and path(v) twice between them, 108
              doubles per pose-pose candidate back -- plus the NumPy error, Jacobians, propagation, 6x6 inverse and distance on the host.

Two workloads: one batch of 32 make_graph(40, 8) graphs with CANDS_PER_GRAPH candidates each, and one L-configuration graph (5000 poses,
1000 landmarks) with --l-candidates candidates.  Every timing is a host clock around calls that end in a device synchronise; after one
warm-up call of either way the two alternate and the MEDIAN OF FIVE is reported.  Both ways must agree on d2 (1e-6 relative, both come
from the same factor) or the script fails.  Prints one JSON line per workload; needs a GPU (there is no CPU fallback).

  python tools/gate_timing.py [--l-candidates 64] [--skip-l]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gate_ref import OMEGA6, assemble, error_jac, perturbed, relative_pose   # noqa: E402  (the NumPy side of the old way: tests/gate_ref.py)

CANDS_PER_GRAPH = 8
REPEATS = 5


def pose_pairs(n_poses, n, rng):
    """n loop-closure candidates: pose pairs at least a quarter of the trajectory apart, the fixed first pose among them"""
    pairs = [(0, n_poses - 1)]
    while len(pairs) < n:
        a, b = sorted(int(x) for x in rng.integers(0, n_poses, 2))
        if b - a >= n_poses // 4:
            pairs.append((a, b))
    return pairs


def by_gate(B, cand):
    return B.gate(cand)


def by_marginals(B, cand, est):
    blocks = iter(B.marginals([rq for g, _, u, v, _, _ in cand for rq in ((g, u, u), (g, u, v), (g, v, v))]))
    d2 = np.zeros(len(cand))
    for k, (g, kind, u, v, z, info) in enumerate(cand):
        Zuu, Zuv, Zvv = next(blocks), next(blocks), next(blocks)
        e, Ju, Jv = error_jac(est[g], kind, u, v, z)
        d2[k] = assemble(e, Ju, Jv, Zuu, Zuv, Zvv, info)[1]
    return d2


def measure(name, B, cand, est):
    ways = {"gate": lambda: by_gate(B, cand), "marginals": lambda: by_marginals(B, cand, est)}
    ref = {k: f() for k, f in ways.items()}                                     # warm-up of every shape, and the agreement check
    rel = float(np.max(np.abs(ref["gate"] - ref["marginals"]) / np.abs(ref["marginals"])))
    assert rel <= 1e-6, f"{name}: the two ways disagree on d2 (max relative difference {rel:.3e})"
    times = {k: [] for k in ways}
    for _ in range(REPEATS):
        for k, f in ways.items():                                               # alternating: the host is shared
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    out = {"workload": name, "candidates": len(cand), "d2_max_rel_difference": rel,
           "gate_ms_median_of_5": round(1e3 * statistics.median(times["gate"]), 3),
           "marginals_numpy_ms_median_of_5": round(1e3 * statistics.median(times["marginals"]), 3),
           "gate_ms_all": [round(1e3 * t, 3) for t in times["gate"]], "marginals_numpy_ms_all": [round(1e3 * t, 3) for t in times["marginals"]],
           "path_walks_per_candidate": {"gate": 2, "marginals": 4}, "pcie_bytes_back_per_candidate": {"gate": 43 * 8, "marginals": 108 * 8}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--l-candidates", type=int, default=64)
    ap.add_argument("--skip-l", action="store_true")
    args = ap.parse_args()
    from semantic_slam_amd import GraphBatch, GraphSLAM, load_library
    from semantic_slam_amd.synth import make_graph
    if load_library().sslam_device_count() < 1:
        sys.exit("gate_timing.py needs a GPU: the product has no CPU fallback")
    rng = np.random.default_rng(0)

    def workload(name, synth, n_cand):
        graphs = [GraphSLAM.from_synth(g) for g in synth]
        B = GraphBatch(graphs)
        B.upload()
        B.optimize(2)
        B.download()
        est = [G.estimates() for G in graphs]
        cand = []
        for g, s in enumerate(synth):
            for a, b in pose_pairs(s.n_poses, n_cand, rng):                     # from_synth: pose k is vertex k
                cand.append((g, "se3", a, b, perturbed(relative_pose(est[g][a], est[g][b])), OMEGA6))
        measure(name, B, cand, est)

    workload("32 x make_graph(40, 8)", [make_graph(40, 8, seed=700 + k) for k in range(32)], CANDS_PER_GRAPH)
    if not args.skip_l:
        workload("L configuration: make_graph(5000, 1000)", [make_graph(5000, 1000, seed=0)], args.l_candidates)


if __name__ == "__main__":
    main()
