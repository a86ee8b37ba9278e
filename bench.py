#!/usr/bin/env python
"""bench.py — headline metric of BASELINE.json on MI355X.

  metric : graph-optimize LM iterations/sec on the synthetic 5000-pose / 1000-landmark graph with
           loop closures (BASELINE.json configs[2], the configuration the metric is quoted on).
           The reference's own timer sits around graph->optimize (src/ps_graph_slam/graph_slam.cpp:204-215).
  step   : one Levenberg-Marquardt iteration (Jacobian build + linear solve(s) + update + chi2 +
           accept/reject) over one device-resident batch of `--batch` independent graphs.
  value  : sum over graphs (and ranks) of the LM iterations they actually performed / seconds, inputs resident in HBM
           before the timed region.  g2o's LM stops by itself when ten damping trials in a row fail (rho == 0 / q == 10):
           a graph that converges before `--steps` iterations contributes only what it ran (`iters_min/max`,
           `graphs_terminated` in the JSON line say how many did).

One process per GPU; for N>1 launch with torch.distributed.run (RCCL): independent graphs shard
across ranks with no data-path collective ("scaling": "weak"); the barrier + max-over-ranks timing
uses torch.distributed.

A plain run does only what `value` needs: set up, warm up, time the `--steps` LM iterations of the batch (as a stream group, see
`--streams`), write the outputs if `--dump-outputs DIR` is given, print the JSON line.  `--full` adds everything else this script
measures: the per-kernel pass and its rooflines, the frontend, the tick replays, single-graph latency, Schur + PCG, plane landmarks
and the CPU baselines.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E ~8 TB/s
HOST_WORKERS = 16       # host processes / threads of the setup: a GPU host shares its cores, more than this only slows setup down
DUMP_GRAPHS = 32        # graphs whose final estimates --dump-outputs writes (a fixed, seeded sample of the batch)


def pmc_traffic(name, algorithmic_bytes):
    """HBM bytes per launch from the committed PMC passes (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs,
    FETCH x2 on gfx950 per MI355X_MICROARCH.md); only quoted when the profiled workload had the same algorithmic bytes."""
    for rnd in ("r6", "r5", "r4", "r3", "r2", "r1"):
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", f"{rnd}_pmc_{name}.json")))
        except (OSError, ValueError):
            continue
        if int(pmc.get("algorithmic_bytes", -1)) == int(algorithmic_bytes):
            at = pmc.get("collected_at_commit")     # stamped when the summary was committed (the GPU box has no .git)
            return int(pmc["hbm_bytes_fetch_x2"]), int(pmc["hbm_bytes_raw"]), f"profiles/{rnd}_pmc_{name}.json" + (f" (collected at commit {at})" if at else "")
    return None, None, None


def generate_graphs(kind, poses, landmarks, seeds, cache_dir):
    """One .g2o file per seed (semantic_slam_amd.synth.make_graph -> GraphSLAM::save), written by a pool of plain host processes
    (`python -m semantic_slam_amd.synth`, no HIP call) and kept in `cache_dir`: 512 distinct 5000-pose graphs cost ~1 s of Python
    each; the cache and the pool keep the setup bounded."""
    import subprocess
    os.makedirs(cache_dir, exist_ok=True)
    jobs = [(int(sd), os.path.join(cache_dir, f"{kind}_{poses}_{landmarks}_{int(sd)}.g2o")) for sd in seeds]
    todo = [sd for sd, p in jobs if not (os.path.exists(p) and os.path.getsize(p) > 0)]
    if todo:
        nproc = max(1, min(len(todo), len(os.sched_getaffinity(0)), HOST_WORKERS))
        procs = []
        for w in range(nproc):
            mine = todo[w::nproc]
            if mine:
                procs.append(subprocess.Popen([sys.executable, "-m", "semantic_slam_amd.synth", kind, str(poses), str(landmarks), cache_dir]
                                              + [str(x) for x in mine], cwd=ROOT))
        for pr in procs:
            if pr.wait() != 0:
                raise RuntimeError("graph generator process failed")
    return [p for _, p in jobs]


def load_graphs(paths, n, dev, solver):
    """`n` graphs from the .g2o files (tiled), parsed by a pool of threads: the C parser runs without the GIL."""
    from concurrent.futures import ThreadPoolExecutor
    from semantic_slam_amd import GraphSLAM

    def one(k):
        G = GraphSLAM(False, dev)
        G.load(paths[k % len(paths)])
        if solver >= 0:
            G.set_option("solver", solver)
        return G
    with ThreadPoolExecutor(max_workers=max(1, min(n, len(os.sched_getaffinity(0)), HOST_WORKERS))) as ex:
        return list(ex.map(one, range(n)))


def build_batch(paths, n, dev, solver):
    from semantic_slam_amd import GraphBatch
    batch = GraphBatch(load_graphs(paths, n, dev, solver))
    batch.upload()
    return batch


def edge_counts(path):
    """(SE3 edges, landmark edges) of one .g2o file"""
    eo = el = 0
    with open(path) as f:
        for ln in f:
            if ln.startswith("EDGE_SE3:QUAT "):
                eo += 1
            elif ln.startswith("EDGE_"):
                el += 1
    return eo, el


def dump_outputs(out_dir, batch, stats):
    """What the timed path hands its caller after the last step, as float64 .npy files: the per-graph results of the optimisation
    and the final estimates ([graphs, vertices, 7], point landmarks zero-padded) of a fixed, seeded sample of the batch's graphs."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name in ("iterations", "trials", "status", "chi2_before", "chi2_after", "lambda_", "solver_iterations"):
        np.save(os.path.join(out_dir, f"{name.rstrip('_')}.npy"), np.array([getattr(s, name) for s in stats], np.float64))
    batch.download()
    pick = np.sort(np.random.default_rng(0).choice(len(batch.graphs), size=min(DUMP_GRAPHS, len(batch.graphs)), replace=False))
    np.save(os.path.join(out_dir, "estimates.npy"), np.stack([batch.graphs[int(g)].estimates() for g in pick]))
    np.save(os.path.join(out_dir, "estimates_graph_index.npy"), pick.astype(np.float64))


def timed_optimize(batch, steps, warmup, sync_all):
    """W untimed LM iterations, estimates reset, then K timed ones bracketed by barrier + device sync."""
    if warmup > 0:
        batch.optimize(warmup)
    batch.upload()
    sync_all()
    t0 = time.perf_counter()
    stats = batch.optimize(steps)       # returns after hipStreamSynchronize on the batch's stream
    sync_all()
    return stats, time.perf_counter() - t0


def bench_tick_cpu(events):
    """the CPU oracle replaying the same run as ONE C driver (oracle/oracle_slam.c: keyframe gate, association, graph growth, the C
    oracle's LM and marginals -- no Python or NumPy inside a tick; pinned tick by tick against oracle/np_slam.py in
    tests/test_oracle_slam.py), one core.  Timers are the driver's own (clock_gettime inside oslam_run)."""
    from oracle.oracle import SlamTickC
    o = SlamTickC(const_stddev_x=0.00667, const_stddev_q=0.00001)
    ticks, t_tick, t_opt, t_marg, t_assoc, iters, trials = 0, 0.0, 0.0, 0.0, 0.0, 0, 0
    for ev in events:
        if ev.objects is not None:
            o.set_segmented_objects(ev.objects)
        o.vio(ev.stamp[0], ev.stamp[1], ev.odom)
        if ev.run_after and o.run():
            st = o.last_stats
            ticks += 1; t_tick += st.seconds_total; t_opt += st.seconds_optimize; t_marg += st.seconds_marginals; t_assoc += st.seconds_association
            iters += st.iterations; trials += st.trials
    nv, ne, nkf, nlm = o.counts()
    k = max(ticks, 1)
    return {"ticks": ticks, "ms_per_tick": round(1e3 * t_tick / k, 3), "ms_per_tick_optimize": round(1e3 * t_opt / k, 3),
            "ms_per_tick_marginals": round(1e3 * t_marg / k, 3), "ms_per_tick_association": round(1e3 * t_assoc / k, 3),
            "lm_iterations_per_tick": round(iters / k, 1), "lm_trials_per_tick": round(trials / k, 1),
            "cores": 1, "kind": "port", "keyframes": nkf, "landmarks": nlm,
            "sample": "the same replay through oracle/oracle_slam.c (C tick driver: association + graph growth + oracle_graph.c LM + "
                      "marginals); no Python inside the timed tick"}


def bench_tick(device, n_samples=600, cpu_baseline=True, n_landmarks=40):
    """Orchestrator tick replay: a synthetic run fed through sslam_slam_* -- keyframe gate, data association
    on the device, graph growth (structure rebuilt every tick), optimise to LM termination, marginals of every landmark."""
    import ctypes as C
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    from semantic_slam_amd.segmentation import Plane
    from semantic_slam_amd.synth import make_replay
    events, _ = make_replay(7, n_samples=n_samples, n_landmarks=n_landmarks)
    p = default_slam_params(device)
    p.const_stddev_x, p.const_stddev_q = 0.00667, 0.00001     # config/bucket_detector.yaml:26-27
    S = SemanticGraphSLAM(p)

    def planes_of(objs):
        out = []
        for o in objs:
            q = Plane()
            for k in range(3):
                q.centroid_cam[k] = float(o["pose"][k])
            for k in range(4):
                q.normal_d[k] = float(o["normal"][k])
            q.class_id, q.plane_type = int(o["class_id"]), int(o["plane_type"])
            out.append(q)
        return out
    ticks, t_tick, parts, lm_iters, plan_us = 0, 0.0, [0.0, 0.0, 0.0], 0, []
    for ev in events:
        if ev.objects is not None:
            S.setSegmentedObjects(planes_of(ev.objects))
        S.VIOCallback(ev.stamp, ev.odom)
        if ev.run_after:
            t0 = time.perf_counter()
            ran = S.run()
            dt = time.perf_counter() - t0
            if ran:
                st = S.last_stats
                ticks += 1; t_tick += dt; lm_iters += int(st.opt.iterations) if st.optimized else 0
                parts[0] += st.seconds_association; parts[1] += st.seconds_optimize; parts[2] += st.seconds_marginals
                if st.optimized:
                    plan_us.append(int(st.opt.host_plan_us))
    ids, _ = S.getKeyframes()
    cpu = None
    if cpu_baseline:
        try:
            cpu = bench_tick_cpu(events)
        except Exception as e:
            cpu = {"error": str(e)[:200]}
    vs = None
    if cpu and "ms_per_tick" in cpu and ticks:
        # like for like: the whole tick against the whole C tick, and the optimiser alone against the C optimiser alone (both > 1: the GPU is faster)
        vs = {"tick_speedup_vs_one_core": round(cpu["ms_per_tick"] / (1e3 * t_tick / ticks), 3),
              "optimize_speedup_vs_one_core": round(cpu["ms_per_tick_optimize"] / max(1e3 * parts[1] / ticks, 1e-9), 3)}
    return {"cpu_baseline": cpu, "vs_cpu": vs, "workload": f"synthetic run of {n_samples} odometry samples at 10 Hz, detections every sample (semantic_slam_amd.synth.make_replay), "
                        "objects pre-segmented; every tick re-optimises the whole graph to LM termination (graph_slam.cpp:205)",
            "ticks": ticks, "keyframes": int(len(ids)), "landmarks": len(S.getMappedLandmarks()),
            "ticks_per_sec": round(ticks / t_tick, 2) if t_tick > 0 else None,
            "ms_per_tick": round(1e3 * t_tick / max(ticks, 1), 3),
            "ms_per_tick_association": round(1e3 * parts[0] / max(ticks, 1), 3),
            "ms_per_tick_optimize": round(1e3 * parts[1] / max(ticks, 1), 3),
            "ms_per_tick_marginals": round(1e3 * parts[2] / max(ticks, 1), 3),
            # host work a tick's structure change costs before the first launch: batch tables + symbolic factorisation, re-done from
            # scratch at every tick (no incremental symbolic phase; part of ms_per_tick_optimize): median over the replay (the first tick
            # also allocates the handle's arena) and mean of the last ten ticks, where the graph is largest
            "ms_per_tick_host_plan_median": round(1e-3 * sorted(plan_us)[len(plan_us) // 2], 3) if plan_us else None,
            "ms_per_tick_host_plan_last10": round(1e-3 * sum(plan_us[-10:]) / max(len(plan_us[-10:]), 1), 3) if plan_us else None,
            "lm_iterations_per_tick": round(lm_iters / max(ticks, 1), 1)}


def bench_tick_robots(device, robots=4, n_samples=600, n_landmarks=40):
    """Several robots on ONE GPU (round 6: persistent launches share the device by a budget): `robots` orchestrator handles, each on its
    own host thread and stream, replay the same 110-keyframe run concurrently.  The speculative lanes are off here (ten lanes of one
    robot fill the device; the plain single-launch solve takes about a tenth of it), so the launches of different robots overlap.
    Reported: aggregate ticks per second over all robots, against ONE robot replaying alone with the same setting.  (Measured, one box:
    2 / 4 / 8 / 16 robots 1.87x / 3.26x / 2.64x / 3.16x one robot -- beyond four the host side, one Python thread per robot, is the limit.)"""
    import threading
    from semantic_slam_amd.semantic_graph_slam import SemanticGraphSLAM, default_slam_params
    from semantic_slam_amd.segmentation import Plane
    from semantic_slam_amd.synth import make_replay
    events, _ = make_replay(7, n_samples=n_samples, n_landmarks=n_landmarks)

    def planes_of(objs):
        out = []
        for o in objs:
            q = Plane()
            for k in range(3):
                q.centroid_cam[k] = float(o["pose"][k])
            for k in range(4):
                q.normal_d[k] = float(o["normal"][k])
            q.class_id, q.plane_type = int(o["class_id"]), int(o["plane_type"])
            out.append(q)
        return out
    pre = [(ev, planes_of(ev.objects) if ev.objects is not None else None) for ev in events]   # no Python conversions inside the timed replays

    def replay(count):
        p = default_slam_params(device)
        p.const_stddev_x, p.const_stddev_q = 0.00667, 0.00001
        S = SemanticGraphSLAM(p)
        S.set_graph_option("speculative_trials", 0)
        n = 0
        for ev, objs in pre:
            if objs is not None:
                S.setSegmentedObjects(objs)
            S.VIOCallback(ev.stamp, ev.odom)
            if ev.run_after and S.run():
                n += 1
        count.append(n)

    def timed(k):
        counts, th = [], [threading.Thread(target=lambda: replay(counts)) for _ in range(k)]
        t0 = time.perf_counter()
        for t in th: t.start()
        for t in th: t.join()
        return sum(counts), time.perf_counter() - t0
    timed(1)                      # warm-up (arena, plans' first launches, clocks)
    n1, t1 = timed(1)
    nk, tk = timed(robots)
    return {"robots": robots, "keyframes": 110, "speculative_trials": 0,
            "ticks_per_sec_one_robot": round(n1 / t1, 1), "ticks_per_sec_all_robots": round(nk / tk, 1),
            "scaling_vs_one_robot": round((nk / tk) / (n1 / t1), 2),
            "note": "wall time of the whole replays, Python driver included (one thread per robot; the C calls release the GIL)"}


def bench_frontend(device, frames=8, cpu_baseline=True, batch_frames=32, dist=None, ddev=None):
    """planes/sec on synthetic 640x480 clouds with 32 detection boxes of 128x96 px (BASELINE.json configs[3]).
    Headline: `batch_frames` frames per pass through ONE handle (sslam_seg_segment_batch: the boxes of all frames share every
    launch; 32 frames x 12.6 MB of box pixels = 400 MB, beyond the 256 MiB MALL).  With N ranks the frames shard across ranks
    (no collective) and the planes/s of all ranks are summed."""
    import numpy as np
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    from semantic_slam_amd import distributed as D
    from semantic_slam_amd.synth import make_frame
    rank = int(os.environ.get("RANK", "0"))
    fs = [make_frame(seed=100 * rank + s) for s in range(4)]
    seg = PointCloudSegmentation(device=device)
    for f in fs:
        seg.segmentallPointCloudData(f.robot_pose, f.cam_angle, f.boxes, f)  # warm-up (allocation)
    nplanes, kms = 0, 0.0
    t0 = time.perf_counter()
    for k in range(frames):
        f = fs[k % len(fs)]
        nplanes += len(seg.segmentallPointCloudData(f.robot_pose, f.cam_angle, f.boxes, f))
        kms += seg.last_timing()[0]
    wall = time.perf_counter() - t0
    npx = int(sum(int(b["width"]) * int(b["height"]) for b in fs[0].boxes))
    res = {"workload": "synthetic 640x480 organised cloud (depth noise 1.5e-3 z^2, clustered drop-outs), 32 boxes of 128x96 px per frame "
                       "(BASELINE.json configs[3])",
           "single_frame_calls": {"frames": frames, "planes_per_frame": round(nplanes / frames, 2),
                                  "planes_per_sec_kernels": round(nplanes / (kms * 1e-3), 1), "frames_per_sec_kernels": round(frames / (kms * 1e-3), 1),
                                  "planes_per_sec_incl_pcie_and_host": round(nplanes / wall, 1), "kernel_ms_per_frame": round(kms / frames, 4)},
           "algorithmic_bytes_per_frame": 32 * npx}
    # batched frames through one handle
    bf = [fs[k % len(fs)] for k in range(batch_frames)]
    seg.segment_frames(bf)                                                   # warm-up (allocation)
    reps, bpl, bk = 3, 0, 0.0
    if dist is not None:
        import torch
        torch.cuda.synchronize(); dist.barrier()
    t1 = time.perf_counter()
    for _ in range(reps):
        bpl += sum(len(x) for x in seg.segment_frames(bf))
        bk += seg.last_timing()[0]
    if dist is not None:
        import torch
        torch.cuda.synchronize(); dist.barrier()
    bwall = D.max_over_ranks(time.perf_counter() - t1, device=ddev)
    kern_s = D.max_over_ranks(bk * 1e-3, device=ddev)
    tot_planes = D.aggregate_throughput(float(bpl), 1.0, device=ddev)
    tot_frames = D.aggregate_throughput(float(reps * batch_frames), 1.0, device=ddev)
    gbs = 32 * npx * tot_frames / kern_s / 1e9
    res["batched"] = {"frames_per_call": batch_frames, "calls": reps, "planes_per_frame": round(bpl / (reps * batch_frames), 2),
                      "planes_per_sec_kernels": round(tot_planes / kern_s, 1), "frames_per_sec_kernels": round(tot_frames / kern_s, 1),
                      "planes_per_sec_incl_pcie_and_host": round(tot_planes / bwall, 1), "kernel_ms_per_frame": round(1e3 * kern_s / (reps * batch_frames), 4),
                      "achieved_GBps": round(gbs, 2), "hbm_frac": round(gbs / PEAK_HBM_GBS, 5), "truncated": list(seg.last_overflow())}
    # RANSAC plane per box + point-to-plane ICP per frame on the crops that batch left on the device (BASELINE.json configs[3]:
    # "RANSAC+ICP plane extraction"): one workgroup per box / per frame, 12 bytes per in-box point read once per pass
    try:
        rreps, rms, ims, rplanes, rin, rhyp = 3, 0.0, 0.0, 0, 0, 0
        icp_iters = 5
        for _ in range(rreps):
            recs, ms_r = seg.ransac_boxes(0.01, 50, 0.99, 2024)
            planes_r = np.array([list(r.coeff) for r in recs], np.float32)
            ok = np.array([r.inliers > 500 and abs(float(np.linalg.norm(planes_r[q, :3])) - 1.0) < 1e-3 for q, r in enumerate(recs)])
            box_plane = np.where(ok, np.arange(len(recs)), -1).astype(np.int32)     # every box against its own plane: the fixed point of the ICP
            icp, ms_i = seg.icp_boxes(box_plane, planes_r, icp_iters)
            rms += ms_r; ims += ms_i; rplanes += int(ok.sum()); rin += int(sum(r.inliers for q, r in enumerate(recs) if ok[q])); rhyp += int(sum(r.hypotheses for r in recs))
        pts_total = npx * batch_frames                                          # in-box points of a batch
        rbytes = 12.0 * pts_total * rreps
        ibytes = 12.0 * rin * (icp_iters + 1)
        res["ransac_icp"] = {"frames_per_call": batch_frames, "calls": rreps, "ransac_threshold_m": 0.01, "ransac_max_iterations": 50, "icp_iterations": icp_iters,
                             "planes_per_frame": round(rplanes / (rreps * batch_frames), 2), "hypotheses_per_box": round(rhyp / (rreps * len(recs)), 1),
                             "ransac_kernel_ms_per_frame": round(rms / (rreps * batch_frames), 4), "icp_kernel_ms_per_frame": round(ims / (rreps * batch_frames), 4),
                             "planes_per_sec_kernels": round(rplanes / ((rms + ims) * 1e-3), 1),
                             "ransac_achieved_GBps": round(rbytes / (rms * 1e-3) / 1e9, 2), "ransac_hbm_frac": round(rbytes / (rms * 1e-3) / 1e9 / PEAK_HBM_GBS, 5),
                             "icp_achieved_GBps": round(ibytes / (ims * 1e-3) / 1e9, 2), "icp_rms_m": round(float(np.mean([r.rms for r in icp])), 5),
                             "note": "12 B per in-box point, read from HBM once per RANSAC pass (the crop is staged in LDS and all hypotheses are scored there) "
                                     "and once per ICP round; the crops are those the segmentation left on the device"}
        if cpu_baseline:
            import ctypes as C2
            from oracle import oracle as O
            olib = O.lib()
            t3 = time.perf_counter(); nb_cpu = 0
            while time.perf_counter() - t3 < 3.0:
                f = fs[nb_cpu // 32 % len(fs)]; b = f.boxes[nb_cpu % 32]
                crop = np.ascontiguousarray(f.xyz()[b["tl_y"]:b["tl_y"] + b["height"], b["tl_x"]:b["tl_x"] + b["width"]].reshape(-1, 3))
                coeff = np.zeros(4, np.float32); inl = np.zeros(len(crop), np.int32); bi = C2.c_int(0)
                olib.os_ransac_plane(crop.ctypes.data_as(C2.c_void_p), len(crop), C2.c_float(0.01), 50, C2.c_double(0.99), C2.c_uint64(2024 + nb_cpu),
                                     coeff.ctypes.data_as(C2.c_void_p), inl.ctypes.data_as(C2.c_void_p), len(inl), None, C2.byref(bi))
                nb_cpu += 1
            dt3 = time.perf_counter() - t3
            res["ransac_icp"]["cpu_baseline"] = {"value": round(nb_cpu / dt3, 1), "unit": "boxes/s (RANSAC only)", "cores": 1, "kind": "port",
                                                 "sample": f"{nb_cpu} boxes of the same workload (oracle/oracle_seg.c os_ransac_plane)",
                                                 "gpu_boxes_per_sec_kernels": round(len(recs) * rreps / (rms * 1e-3), 1)}
    except Exception as e:
        res["ransac_icp"] = {"error": repr(e)[:300]}
    # pipelined batches (sslam_seg_submit_batch / _collect_batch): the H2D copy of batch k+1 under the kernels of batch k; the clouds
    # sit in pinned host memory, as a capture pipeline that feeds a GPU would keep them
    pins = []
    seg_params = seg.params
    from semantic_slam_amd import load_library
    lib = load_library()
    try:
        import copy
        import ctypes as C
        pinned = []
        for f in fs:
            ptr = lib.sslam_pinned_alloc(f.cloud.nbytes)          # page-locked through the product's own C-ABI (no torch needed)
            if not ptr:
                raise RuntimeError(lib.sslam_last_error().decode())
            pins.append(ptr)
            arr = np.ctypeslib.as_array((C.c_uint8 * f.cloud.nbytes).from_address(ptr)).view(f.cloud.dtype).reshape(f.cloud.shape)
            arr[...] = f.cloud
            g = copy.copy(f); g.cloud = arr
            pinned.append(g)
        pbf = [pinned[k % len(pinned)] for k in range(batch_frames)]
        list(seg.segment_stream([pbf, pbf]))                                 # warm-up (allocates the second pipeline)
        preps, ppl = 24, 0                                                    # a stream: the unhidden first copy and last kernels are 2 of 24 batches, not 2 of 6
        if dist is not None:
            import torch
            torch.cuda.synchronize(); dist.barrier()
        t2 = time.perf_counter()
        for planes in seg.segment_stream([pbf] * preps):
            ppl += sum(len(x) for x in planes)
        if dist is not None:
            torch.cuda.synchronize(); dist.barrier()
        pwall = D.max_over_ranks(time.perf_counter() - t2, device=ddev)
        ptot = D.aggregate_throughput(float(ppl), 1.0, device=ddev)
        res["pipelined"] = {"frames_per_batch": batch_frames, "batches": preps, "pinned_clouds": True,
                            "planes_per_sec_incl_pcie_and_host": round(ptot / pwall, 1),
                            "ms_per_frame_incl_pcie_and_host": round(1e3 * pwall / (preps * batch_frames), 4),
                            "h2d_MB_per_frame": round(fs[0].cloud.nbytes / 1e6, 2)}
        # the same frames as 12-byte xyz points (the frontend reads x, y, z only; the C-ABI takes any point_step): what a caller that
        # converts the sensor message anyway (pcl::fromROSMsg in the reference's callback) can hand over -- INTEGRATION.md section 2
        from semantic_slam_amd.synth import repack_xyz
        pinned12 = []
        for f in fs:
            g = repack_xyz(f, 12)
            ptr = lib.sslam_pinned_alloc(g.cloud.nbytes)
            if not ptr:
                raise RuntimeError(lib.sslam_last_error().decode())
            pins.append(ptr)
            arr = np.ctypeslib.as_array((C.c_uint8 * g.cloud.nbytes).from_address(ptr)).view(g.cloud.dtype).reshape(g.cloud.shape)
            arr[...] = g.cloud
            g.cloud = arr
            pinned12.append(g)
        pbf12 = [pinned12[k % len(pinned12)] for k in range(batch_frames)]
        list(seg.segment_stream([pbf12, pbf12]))
        ppl12 = 0
        if dist is not None:
            torch.cuda.synchronize(); dist.barrier()
        t2 = time.perf_counter()
        for planes in seg.segment_stream([pbf12] * preps):
            ppl12 += sum(len(x) for x in planes)
        if dist is not None:
            torch.cuda.synchronize(); dist.barrier()
        pwall12 = D.max_over_ranks(time.perf_counter() - t2, device=ddev)
        ptot12 = D.aggregate_throughput(float(ppl12), 1.0, device=ddev)
        res["pipelined_xyz12"] = {"frames_per_batch": batch_frames, "batches": preps, "pinned_clouds": True, "point_step_bytes": 12,
                                  "planes_per_sec_incl_pcie_and_host": round(ptot12 / pwall12, 1),
                                  "ms_per_frame_incl_pcie_and_host": round(1e3 * pwall12 / (preps * batch_frames), 4),
                                  "h2d_MB_per_frame": round(pinned12[0].cloud.nbytes / 1e6, 2), "same_planes_as_32_byte_points": bool(ppl12 == ppl)}
    except Exception as e:
        res["pipelined"] = {"error": repr(e)}
    finally:
        del seg                                                              # the handle's streams are idle before the clouds go
        for ptr in pins:
            lib.sslam_pinned_free(ptr)
    res["planes_per_sec"] = res["batched"]["planes_per_sec_kernels"]
    if cpu_baseline:
        from oracle.oracle import segment_frame   # cpu_baseline leg only
        t1 = time.perf_counter(); np_cpu = 0; nf = 0
        while time.perf_counter() - t1 < 6.0:
            ref, _, _ = segment_frame(fs[nf % len(fs)], seg_params)
            np_cpu += len(ref); nf += 1
        dt = time.perf_counter() - t1
        res["cpu_baseline"] = {"value": round(np_cpu / dt, 2), "unit": "planes/s", "frames_per_sec": round(nf / dt, 3), "cores": 1,
                               "kind": "port", "sample": f"{nf} frames of the same workload (oracle/oracle_seg.c)"}
    return res


def launcher_command(argv, gpus, environ, port=None):
    """`python bench.py --gpus N` typed on its own (no launcher, WORLD_SIZE unset) must still run N ranks: the command line that
    re-executes this script under torch.distributed.run, one process per GPU over RCCL, rendezvous on 127.0.0.1 (the container hostname
    may not resolve).  None when no re-launch is needed: N <= 1, or a launcher already set WORLD_SIZE (the driver's own
    `python -m torch.distributed.run ... bench.py --gpus N`)."""
    if gpus <= 1 or "WORLD_SIZE" in environ:
        return None
    if port is None:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={int(gpus)}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("SSLAM_BENCH_BATCH", "1024")),
                    help="independent graphs resident per GPU (~30 MB each: H, L, update matrices, tables -- 30 GB of the 288, far beyond the 256 MiB MALL).  "
                         "Round 6: 1024 (rounds 1-5: 512) -- the top of the elimination tree is latency-bound with one workgroup per graph, and twice the graphs "
                         "hide it better: 45.6 k vs 43.4 k it/s on one box; 2048: 37.0 k")
    ap.add_argument("--poses", type=int, default=5000)
    ap.add_argument("--landmarks", type=int, default=1000)
    ap.add_argument("--distinct", type=int, default=-1, help="distinct seeds generated per rank (tiled to --batch); -1 = one per graph of the batch")
    ap.add_argument("--plane-distinct", type=int, default=-1, help="distinct seeds of the plane-landmark leg (tiled to --plane-batch); -1 = one per graph")
    ap.add_argument("--cache-dir", default=os.environ.get("SSLAM_BENCH_CACHE", os.path.join(tempfile.gettempdir(), "sslam_bench_cache")))
    ap.add_argument("--solver", type=int, default=-1, help="-1 library default, 0 PCG, 1 sparse Cholesky")
    ap.add_argument("--streams", type=int, default=4,
                    help="stream group of the timed region (sslam_batch_create_streams): the batch split into this many parts, each on its own "
                         "HIP stream + host thread; <= 1: one batch-synchronous batch.  The kernel rooflines always come from a single-stream pass")
    ap.add_argument("--plane-batch", type=int, default=1024, help="graphs in the plane-landmark leg (0 = skip)")
    ap.add_argument("--edge-sharded", action="store_true",
                    help="N > 1: every rank holds the SAME batch, builds the partial normal equations of its edge shard and the ranks "
                         "all-reduce [H || b] over RCCL each LM step (SURVEY 8e mode E / BASELINE.json configs[4]); strong scaling")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline: per-kernel pass + rooflines, frontend, tick replays, single graph, "
                         "Schur + PCG, plane landmarks, CPU baselines (the --no-* / --plane-* options below select among these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed to DIR/<name>.npy (float64; rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-frontend", action="store_true")
    ap.add_argument("--no-single", action="store_true", help="skip the single-graph latency section (used under rocprofv3 --pmc)")
    args = ap.parse_args()

    cmd = launcher_command(sys.argv[1:], args.gpus, os.environ)
    if cmd is not None:   # N ranks asked for, none launched yet: become the launcher; rank 0 of the children prints the JSON line
        import subprocess
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this driver (RCCL fails with the legacy mode)
        raise SystemExit(subprocess.call(cmd, env=env))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); reporting n_gpus = {world}", file=sys.stderr)
    if os.environ.get("SSLAM_BENCH_LAUNCH_PROBE"):   # CPU test of the launch path (tests/test_bench_launcher_cpu.py): rendezvous over gloo, no GPU work
        import torch.distributed as pdist
        if world > 1:
            pdist.init_process_group("gloo")
            pdist.barrier()
            pdist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"probe": True, "n_gpus": world, "gpus_arg": args.gpus, "edge_sharded": bool(args.edge_sharded), "steps": args.steps}))
        return
    dist = None
    if world > 1:
        import torch  # loaded first so that libamdhip64 is shared with the product library
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl")
    from semantic_slam_amd import GraphSLAM, GraphBatch, load_library
    from semantic_slam_amd import distributed as D
    from semantic_slam_amd.synth import make_graph
    from oracle.oracle import GraphProblem  # only for problem packing + the cpu_baseline leg

    lib = load_library()
    if lib.sslam_device_count() < 1:
        raise SystemExit("bench.py needs a GPU: the product has no CPU fallback")
    dev = local_rank if world > 1 else 0
    ddev = "cuda" if dist is not None else None

    # one process: the interval and the count are the whole job's (D's helpers would load torch just to return them)
    def max_over_ranks(seconds):
        return D.max_over_ranks(seconds, device=ddev) if dist is not None else seconds

    def aggregate_throughput(units, seconds):
        return D.aggregate_throughput(units, seconds, device=ddev) if dist is not None else units / seconds

    def sync_all():
        if dist is not None:
            import torch
            torch.cuda.synchronize()
            dist.barrier()

    sharded = bool(args.edge_sharded and world > 1)

    def seeds_of(n_distinct):
        return [(0 if sharded else 100000 * rank) + d for d in range(n_distinct)]

    # ---- synthetic workload, resident in HBM before timing -------------------------------------
    t_setup = time.time()
    n_distinct = args.batch if args.distinct < 0 else max(1, min(args.distinct, args.batch))
    paths = generate_graphs("point", args.poses, args.landmarks, seeds_of(n_distinct), args.cache_dir)
    Eo, El = edge_counts(paths[0])
    n_streams = 1 if (sharded or args.streams <= 1 or args.solver in (0, 2)) else min(args.streams, args.batch)
    graphs = load_graphs(paths, args.batch, dev, args.solver)

    def make_batch(streams):
        b = GraphBatch(graphs, streams=streams) if streams > 1 else GraphBatch(graphs)
        b.upload()
        if sharded:
            D.init_edge_sharded(b, device=ddev)   # RCCL communicator inside the library; all-reduce issued from the C++ LM loop
        return b
    if args.full:
        # the first graphs again as flat arrays: the cpu_baseline leg
        problems = [GraphProblem.from_synth(make_graph(args.poses, args.landmarks, seed=sd)) for sd in seeds_of(min(n_distinct, 4))]
        batch = make_batch(1)
    setup_s = time.time() - t_setup

    # ---- warmup (untimed), reset to the initial estimates, K timed steps ---------------------------
    # The timed region of `value`: the batch as a stream group (--streams parts, each on its own stream + host thread, events off).
    # --full runs a kernel pass before it over the same graphs: ONE batch-synchronous batch on one stream with hipEvents round every
    # kernel group -> kernel_ms and the rooflines (launches that overlap on the chip cannot be timed one by one); identical results.
    def timed(bt, profiling):
        if args.warmup > 0:
            bt.optimize(args.warmup)
        bt.upload()
        bt.set_profiling(profiling)
        sync_all()
        t0_ = time.perf_counter()
        st_ = bt.optimize(args.steps)       # blocks until every stream of the batch is idle
        sync_all()
        return st_, max_over_ranks(time.perf_counter() - t0_)

    single_stream = None
    if not args.full:
        group_error = None
        try:
            batch = make_batch(n_streams)
            stats, dt = timed(batch, False)
        except Exception as e:   # the headline falls back to a single-stream batch (multi-rank runs must not diverge: re-raise there)
            if dist is not None or n_streams <= 1:
                raise
            group_error = f"stream group failed, value is the single-stream pass: {str(e)[:160]}"
        if group_error is not None:
            batch, n_streams = None, 1
            batch = make_batch(1)
            stats, dt = timed(batch, False)
            single_stream = {"error": group_error}
        timed_batch, timed_stats = batch, stats
        iters = [int(s.iterations) for s in stats]
        iters_total = float(sum(iters))
        steps_done = max(iters) if iters else 0
    else:
        stats, dt_single = timed(batch, True)
        iters = [int(s.iterations) for s in stats]
        iters_total = float(sum(iters))
        steps_done = max(iters) if iters else 0
        dt = dt_single
        timed_batch, timed_stats = batch, stats
        if n_streams > 1:
            try:
                group = GraphBatch(batch.graphs, streams=n_streams)
                gstats, dt = timed(group, False)
                if [int(s.iterations) for s in gstats] != iters or [int(s.trials) for s in gstats] != [int(s.trials) for s in stats]:
                    raise RuntimeError("stream group and single-stream batch disagree on iterations / trials")
                single_stream = {"value": round(aggregate_throughput(iters_total, dt_single), 3),
                                 "ms_per_step": round(1e3 * dt_single / max(steps_done, 1), 4),
                                 "note": "the same steps by one batch-synchronous batch on one stream, hipEvents round every kernel group on: "
                                         "the pass kernel_ms and the rooflines are taken from"}
                timed_batch, timed_stats = group, gstats
            except Exception as e:   # the headline falls back to the single-stream pass (multi-rank runs must not diverge: re-raise there)
                if dist is not None:
                    raise
                n_streams, dt = 1, dt_single
                single_stream = {"error": f"stream group failed, value is the single-stream pass: {str(e)[:160]}"}
    # whole-job value: graph-iterations actually performed by ALL ranks / max-over-ranks time (replicas: no data-path collective)
    value = iters_total / dt if sharded else aggregate_throughput(iters_total, dt)

    trials_total = int(sum(int(s.trials) for s in stats))
    if args.full:
        # ---- kernel times (hipEvents on the batch's stream, inside the timed region) -------------------
        # The LM rounds of a batch of distinct graphs mix full launches with partial ones (a round in which only the graphs that retry a
        # rejected trial take part): `achieved` = algorithmic bytes of the work ACTUALLY done in the timed region (per-graph bytes x graph
        # builds / graph factorisations performed) / the kernels' total time there.  The same kernels timed on the whole batch
        # (every graph taking part) are reported next to it as `full_batch`.
        names = ["linearize", "chi2", "spmv", "pcg_update", "precond", "oplus", "factor", "solve"]
        ktimes = {n: batch.kernel_time(n) for n in names}
        batch.set_profiling(False)
        dominant = max(ktimes, key=lambda n: ktimes[n][0])
        jac_bytes = batch.linearize_bytes()            # whole batch, one build of every graph
        lin_ms, lin_n = ktimes["linearize"]
        jac_done = jac_bytes / args.batch * iters_total            # every LM iteration of a graph builds its system once
        jac_gbs = jac_done / (lin_ms * 1e-3) / 1e9 if lin_ms > 0 else 0.0
        full_lin_ms = batch.time_linearize(10)
        roof_jac = {"bound": "hbm", "kernel": "jacobian_build", "achieved": round(jac_gbs, 2), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(jac_gbs / PEAK_HBM_GBS, 4), "traffic": None, "measured_in": "single-stream pass of the same steps (hipEvents per kernel group)",
                    "bytes_per_launch": jac_bytes, "graph_builds_in_region": int(iters_total), "ms_in_region": round(lin_ms, 3), "launches": lin_n,
                    "full_batch": {"ms_per_launch": round(full_lin_ms, 5), "achieved": round(jac_bytes / (full_lin_ms * 1e-3) / 1e9, 2),
                                   "frac": round(jac_bytes / (full_lin_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4), "ms_per_512_graphs": round(full_lin_ms * 512 / args.batch, 5)}}
        t, raw, src = pmc_traffic("jacobian_build", jac_bytes)
        if t is not None:
            roof_jac.update({"traffic": t, "traffic_raw_counters": raw, "traffic_source": src,
                             "traffic_kind": f"static: the committed rocprofv3 PMC passes over one launch of the same {args.batch}-graph workload, not collected in this run"})
        roofline = roof_jac
        roof_factor = None
        if ktimes["factor"][1] > 0:
            fbytes = int(batch.info("factor_bytes"))   # whole batch, one factorisation of every graph
            f_done = fbytes / args.batch * trials_total
            gbs = f_done / (ktimes["factor"][0] * 1e-3) / 1e9
            full_f_ms, full_s_ms = batch.time_solver(5)
            roof_factor = {"bound": "hbm", "kernel": "block_cholesky_factor (all kernels of one numeric factorisation + fused forward solve)",
                           "achieved": round(gbs, 2), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": None,
                           "measured_in": "single-stream pass of the same steps (hipEvents per kernel group)", "bytes_per_launch": fbytes, "graph_factorisations_in_region": trials_total, "ms_in_region": round(ktimes["factor"][0], 3),
                           "launches": ktimes["factor"][1],
                           "full_batch": {"ms_per_launch": round(full_f_ms, 4), "achieved": round(fbytes / (full_f_ms * 1e-3) / 1e9, 2),
                                          "frac": round(fbytes / (full_f_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4), "backward_solve_ms": round(full_s_ms, 4),
                                          "ms_per_512_graphs": round(full_f_ms * 512 / args.batch, 4), "backward_solve_ms_per_512_graphs": round(full_s_ms * 512 / args.batch, 4)},
                           "levels": int(batch.info("factor_levels")), "factor_doubles": int(batch.info("factor_lnz")),
                           "note": "algorithmic bytes = read H, b once + write L, y once per graph factorisation"}
            t, raw, src = pmc_traffic("factor", fbytes)
            if t is not None:
                roof_factor.update({"traffic": t, "traffic_raw_counters": raw, "traffic_source": src,
                                    "traffic_kind": f"static: the committed rocprofv3 PMC passes over one launch of the same {args.batch}-graph workload, not collected in this run"})
            if dominant == "factor":
                roofline = roof_factor
        if dominant == "spmv" and ktimes["spmv"][1] > 0:
            # H bytes + 3 vectors x 8*dim per block-SpMV
            Np, Nl = args.poses - 1, args.landmarks
            h_bytes = 8 * (36 * Np + 9 * Nl + 36 * Eo + 18 * El)
            spmv_bytes = args.batch * (h_bytes + 3 * 8 * (6 * Np + 3 * Nl))
            ms = ktimes["spmv"][0] / ktimes["spmv"][1]
            gbs = spmv_bytes / (ms * 1e-3) / 1e9
            roofline = {"bound": "hbm", "kernel": "pcg_block_spmv", "achieved": round(gbs, 2), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": None, "bytes_per_launch": spmv_bytes,
                        "ms_per_launch": round(ms, 5), "launches": ktimes["spmv"][1],
                        "note": "bytes assume every still-active graph; converged graphs early-exit"}

    out = {
        "metric": "graph-optimize LM iters/sec (5k poses, 1k landmarks)",
        "value": round(value, 3), "unit": "iters/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / max(steps_done, 1), 4), "higher_is_better": True, "scaling": "strong" if sharded else "weak",
        "vs_baseline": None, "dtype": "f64",
        "data": f"synthetic ({len(paths)} distinct graphs per GPU" + (")" if len(paths) >= args.batch else f" tiled to the batch of {args.batch})"),
        "config": {"workload": f"synthetic {args.poses}-pose / {args.landmarks}-landmark graph with loop closures "
                               f"(BASELINE.json configs[2]), batch of {args.batch} independent graphs per GPU, point landmarks "
                               f"(EdgeSE3PointXYZ, the reference's live landmark type)",
                   "graphs_per_gpu": args.batch, "se3_edges": Eo, "landmark_edges": El,
                   "solver": int(args.solver), "streams": n_streams,
                   "parallelism": (f"edge-sharded x{world}: RCCL all-reduce of [H || b] per LM step" if sharded else f"replicas x{world}")},
        "steps_done": steps_done, "iters_min": min(iters), "iters_max": max(iters),
        "lm_trials_total": trials_total, "distinct_graphs": len(paths),
        "graphs_terminated": int(sum(1 for s in stats if s.status == 1)),
        "timed_seconds": round(dt, 4), "single_stream": single_stream,
        "keyframes_landmarks_per_sec": round(value * (args.poses + args.landmarks), 1),
        "chi2_after": stats[0].chi2_after, "lm_trials": stats[0].trials, "solver_iterations": stats[0].solver_iterations,
        "setup_seconds": round(setup_s, 1),
    }
    if args.full:
        out.update({"trial_rounds": int(ktimes["factor"][1] or ktimes["spmv"][1] and ktimes["precond"][1]),
                    "roofline": roofline, "roofline_jacobian_build": roof_jac,
                    "kernel_ms": {n: [round(v[0], 3), v[1]] for n, v in ktimes.items() if v[1]}})
        if roof_factor is not None:
            out["roofline_factor"] = roof_factor
    if sharded:
        # evidence that RCCL saw `world` ranks: the all-reduce calls this rank issued inside the LM loop and what each of them summed
        out["collective"] = {"backend": "rccl (ncclAllReduce, ncclDouble, sum, out of place)", "world": world,
                             "allreduce_calls": int(batch.info("allreduce_calls")),
                             "bytes_per_call": int(8 * (batch.info("h_doubles") + batch.info("dim"))),
                             "note": "one call per Jacobian build of the batch: [H || b] of every graph, rank-partial buffer -> full system"}
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, timed_batch, timed_stats)
    del batch, timed_batch, graphs

    frontend = None
    if args.full and not args.no_frontend:   # every rank: the frames shard across ranks
        try:
            frontend = bench_frontend(dev, cpu_baseline=(not args.no_cpu_baseline and world == 1 and rank == 0), dist=dist, ddev=ddev)
        except Exception as e:
            if dist is not None:
                raise
            frontend = {"error": str(e)[:200]}
    if rank == 0:
        if frontend is not None:
            out["frontend"] = frontend
        if args.full and not args.no_single:
            try:
                out["tick_replay"] = bench_tick(dev, cpu_baseline=not args.no_cpu_baseline)
                # the same node loop on a run four times as long (the graph grows to ~450 keyframes): where the per-tick cost of the
                # one-core CPU path (linear in the graph) crosses the GPU path's (launch-latency bound, nearly flat)
                out["tick_replay_long"] = bench_tick(dev, n_samples=2400, cpu_baseline=not args.no_cpu_baseline, n_landmarks=160)
            except Exception as e:   # the headline line must still be printed
                out["tick_replay"] = {"error": str(e)[:200]}
            try:
                out["tick_replay_robots"] = bench_tick_robots(dev)
                cpu_t = (out.get("tick_replay", {}).get("cpu_baseline") or {}).get("ms_per_tick")
                if cpu_t:   # aggregate of the robots on one GPU against one host core replaying one robot (the C tick driver)
                    out["tick_replay_robots"]["ticks_per_sec_one_host_core"] = round(1e3 / cpu_t, 1)
                    out["tick_replay_robots"]["all_robots_vs_one_core"] = round(out["tick_replay_robots"]["ticks_per_sec_all_robots"] * cpu_t / 1e3, 2)
            except Exception as e:
                out["tick_replay_robots"] = {"error": str(e)[:200]}
            # ---- single-graph latency (same graph, batch of one) -----------------------------------
            b1 = build_batch(paths[:1], 1, dev, args.solver)
            s1, d1 = timed_optimize(b1, args.steps, 1, lambda: None)
            n1 = max(int(s1[0].iterations), 1)
            out["single_graph"] = {"iters_per_sec": round(n1 / d1, 2), "ms_per_iter": round(1e3 * d1 / n1, 3), "iterations": n1,
                                   "regime": "latency-bound (working set < L2/MALL)", "chi2_after": s1[0].chi2_after}
            del b1
        if args.full and not args.no_single and world == 1:
            # ---- north_star's "Schur-complement + PCG" (solver 2) on the same L graph: what it costs per LM trial -------------
            try:
                b2 = build_batch(paths[:1], 1, dev, 2)
                t0 = time.perf_counter()
                s2 = b2.optimize(3)
                d2 = time.perf_counter() - t0
                out["schur_pcg"] = {"workload": "one L graph, 3 LM iterations, solver 2 (landmarks eliminated, matrix-free PCG on the reduced pose system, "
                                                "block-Jacobi preconditioner, relative residual 1e-10)",
                                    "iterations": int(s2[0].iterations), "trials": int(s2[0].trials), "cg_iterations": int(s2[0].solver_iterations),
                                    "cg_iterations_per_trial": round(s2[0].solver_iterations / max(int(s2[0].trials), 1), 1),
                                    "ms_per_trial": round(1e3 * d2 / max(int(s2[0].trials), 1), 2), "chi2_after": s2[0].chi2_after}
                del b2
            except Exception as e:
                out["schur_pcg"] = {"error": str(e)[:200]}
        if args.full and args.plane_batch > 0 and world == 1:
            # ---- plane landmarks (BASELINE.json metric: "5k poses, 1k planes"): VertexPlane + EdgeSE3Plane, numeric Jacobians
            try:
                n_pd = args.plane_batch if args.plane_distinct < 0 else max(1, min(args.plane_distinct, args.plane_batch))
                ppaths = generate_graphs("plane", args.poses, args.landmarks, seeds_of(n_pd), args.cache_dir)
                pb = build_batch(ppaths, args.plane_batch, dev, args.solver)
                if n_streams > 1:   # the same stream group as the headline
                    pb = GraphBatch(pb.graphs, streams=min(n_streams, args.plane_batch))
                ps, pdt = timed_optimize(pb, args.steps, min(args.warmup, 2), lambda: None)
                pit = [int(s.iterations) for s in ps]
                out["plane_landmarks"] = {"value": round(sum(pit) / pdt, 3), "unit": "iters/s", "graphs": args.plane_batch,
                                          "distinct_graphs": len(ppaths), "streams": n_streams, "iters_min": min(pit), "iters_max": max(pit), "chi2_after": ps[0].chi2_after,
                                          "workload": f"{args.poses} poses / {args.landmarks} plane landmarks (in-tree EdgeSE3Plane, "
                                                      f"central-difference Jacobians), batch of {args.plane_batch}"}
                del pb
                # the metric names "1k planes": both landmark types in the metric string (point landmarks are what the reference executes and
                # what `value` measures; the plane variant pays central-difference Jacobians on the device and more damping trials)
                out["metric"] = (f"graph-optimize LM iters/sec (5k poses, 1k landmarks): point landmarks {out['value'] / 1e3:.1f}k = value, "
                                 f"plane landmarks {out['plane_landmarks']['value'] / 1e3:.1f}k")
            except Exception as e:   # the headline line must still be printed
                out["plane_landmarks"] = {"error": str(e)[:200]}
        if args.full and not args.no_cpu_baseline and world == 1:
            # ---- CPU baseline: the oracle (restated reference algorithm), 1 core, bounded sample ----
            reps, cpu_t, cpu_it, budget = 0, 0.0, 0, 15.0
            while cpu_t < budget:
                gp = problems[reps % len(problems)].copy()
                st = gp.optimize(args.steps)
                cpu_t += st.seconds
                cpu_it += int(st.iterations)
                reps += 1
            out["cpu_baseline"] = {"value": round(cpu_it / cpu_t, 3), "unit": "iters/s", "cores": 1, "kind": "port",
                                   "sample": f"{reps} runs of <= {args.steps} LM iterations ({cpu_it} performed) on the same {args.poses}/{args.landmarks} "
                                             f"graphs (oracle/oracle_graph.c: LM + min-degree sparse Cholesky, gcc -O3 -march=native)",
                                   "host_cores_available": os.cpu_count()}
            # the same port on many host cores at once (independent graphs, one per thread; the C call releases the GIL)
            from concurrent.futures import ThreadPoolExecutor
            ncore = min(len(os.sched_getaffinity(0)), 64)
            work = [problems[k % len(problems)].copy() for k in range(ncore)]
            deadline = time.perf_counter() + 6.0

            def run(gp):
                n = 0
                while n == 0 or time.perf_counter() < deadline:
                    n += int(gp.copy().optimize(args.steps).iterations)
                return n
            tA = time.perf_counter()
            with ThreadPoolExecutor(max_workers=ncore) as ex:
                its = sum(ex.map(run, work))
            dA = time.perf_counter() - tA
            out["cpu_baseline_multicore"] = {"value": round(its / dA, 3), "unit": "iters/s", "cores": ncore, "kind": "port",
                                             "sample": f"{its} LM iterations over {ncore} threads in {dA:.1f} s, independent graphs (same oracle)"}
        print(json.dumps(out))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
