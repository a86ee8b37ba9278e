"""Inputs that the generators hold constant, on the GPU.  Every test input of the suite comes from synth.make_graph with k_obs=3,
loop_every=50 and one landmark kind, or from synth.make_frame's 640 x 480 frames with packed rows, x, y, z at 0, 4, 8 and boxes inside
the image; kernel branches that depend on those constants have seen one value.  This file varies them:

  1. graph structure (tests/graph_shapes.py): hubs, 32 and 12 observations per pose, a loop closure per pose, a bare chain, a second
     fixed pose, two components -- through linearise, every launch form of the solve, LM and the marginals;
  2. point and plane landmarks in one graph;
  3. cloud layout (tests/cloud_layout.py: permuted fields, padded rows), boxes on the image border, another image size, another
     normal_smoothing_size;
  4. a landmark table of more than two strides of k_associate, with ties between landmarks 256 and more apart (tests/assoc_ties.py).

No bar is new: each is the bar of the existing test named where it is used, against that test's reference."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import assoc_ties as AT
import cloud_layout as CL
import graph_shapes as GS
import test_batch_marginals_gpu as BM
import test_batch_solve_gpu as BS
import test_fitness_gpu as TF
import test_seg_gpu as TS
from chol_plan_exec import Plan
from oracle.oracle import GraphProblem
from semantic_slam_amd.synth import make_frame, make_graph

pytestmark = pytest.mark.gpu


def _full(U):
    return (U + sp.triu(U, 1).T).tocsc()


# ======== 1. graph structures ============================================================================================================
@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("name", GS.NAMES)
def test_linearize_every_shape(gpu_lib, name, interleave):
    from semantic_slam_amd import GraphSLAM
    gp = GS.problem(name, interleave)
    tol = 2e-5 if name in GS.PLANE_SHAPES else 1e-11                 # test_linearize_matches_oracle: 1e-11 for point graphs, 2e-5 for planes
    G = GraphSLAM.from_problem(gp)
    U, b = G.linearize()
    Uo, bo = gp.linearize()
    assert U.shape == Uo.shape
    scale = abs(Uo).max()
    eH = abs(_full(U) - _full(Uo)).max() / scale
    eb = np.abs(b - bo).max() / max(1.0, np.abs(bo).max())
    ec = abs(G.chi2() - gp.chi2()) / gp.chi2()
    print(f"{name} interleave {interleave}: dim {len(b)} degrees {GS.degrees(gp)} | H {eH:.3e} b {eb:.3e} (bar {tol:g}) chi2 {ec:.3e} (bar 1e-12)")
    assert eH <= tol and eb <= tol
    assert ec <= 1e-12                                               # test_linearize_matches_oracle
    h, n = gp.hessian_index()
    assert [G.hessian_index(v) for v in range(gp.nv)] == list(h)


def _ten():
    return [GS.problem(n) for n in GS.NAMES]


@pytest.mark.parametrize("name", GS.NAMES)
def test_solve_single_handle_every_shape(gpu_lib, name):
    """(a) a batch of one: the single launch (k_chol_flow), bars of test_batch_solve_gpu._check"""
    g = GS.NAMES.index(name)
    gp = GS.problem(name)
    _, B = BS._batch([gp])
    assert B.info("factor_front") == 0
    lam = BS._lams(10)[g]
    BS._check(gp, B.solve([lam])[0], lam, f"single handle {name}")


def test_solve_batch_of_shapes_on_the_record_kernels(gpu_lib):
    """(b) the ten shapes as one batch on the per-depth record kernels, with test_record_plan_with_compaction's masked rounds (4 of 10
    off index lists, 6 of 10 on full ranges)"""
    gps = _ten()
    _, B = BS._batch(gps)
    assert B.info("factor_front") == 0
    lam = BS._lams(10)
    full = B.solve(lam)
    assert B.info("compact_rounds") == 0
    for g, gp in enumerate(gps):
        BS._check(gp, full[g], lam[g], f"record kernels {GS.NAMES[g]}")
    BS._masked_rounds(B, gps, full, lam, sample=())


def test_solve_stream_group_of_shapes(gpu_lib):
    """(d) streams = 2, bitwise equal to (b).  A part of a stream group is a batch of its own and is planned by ITS size: the ten shapes
    split five and five fall below the eight graphs of the per-depth launches and are planned for the single launch (chol_opts_normalise:
    another cut, another summation order), so their bits are those of single-stream batches of five, not of (b) -- found on the first
    GPU run of this test (the five graphs of the second part, loop3 first, differed from (b) in the last bits; every graph was inside
    the bar).  The bitwise statement of sslam.h holds where every part is planned like the whole.  Both are pinned:
      * twenty graphs, the ten shapes twice, in two parts: each part IS the batch of (b), and gives its bits, full and compacted;
      * the ten shapes in two parts of five: the bits of the two single-stream batches of five, and the bar of (b)."""
    gps = _ten()
    lam = BS._lams(10)
    _, B = BS._batch(gps)
    full = B.solve(lam)
    _, B2 = BS._batch(gps + _ten(), streams=2)
    assert B2.info("streams") == 2 and B2.info("factor_front") == 0
    x2 = B2.solve(lam + lam)
    for g in range(20):
        assert BS._same(x2[g], full[g % 10]), f"stream group of 2 x 10 differs from the batch of ten: part {g // 10}, {GS.NAMES[g % 10]}"
    few = {1, 4, 6, 9, 11, 14, 16, 19}                              # 4 of 10 in either part: both compact
    xm = B2.solve([lam[g % 10] if g in few else -1.0 for g in range(20)])
    assert B2.info("compact_rounds") == 2                            # summed over the parts
    for g in range(20):
        assert (BS._same(xm[g], full[g % 10]) if g in few else xm[g] is None), g
    _, B3 = BS._batch(gps, streams=2)
    assert B3.info("streams") == 2
    x3 = B3.solve(lam)
    halves = BS._batch(gps[:5])[1].solve(lam[:5]) + BS._batch(gps[5:])[1].solve(lam[5:])
    print("parts of five against the batch of ten, bitwise equal:", {GS.NAMES[g]: BS._same(x3[g], full[g]) for g in range(10)})
    for g, gp in enumerate(gps):
        assert BS._same(x3[g], halves[g]), f"stream group of 2 x 5 differs from the single-stream batch of its part: {GS.NAMES[g]}"
        BS._check(gp, x3[g], lam[g], f"stream group of 2 x 5 {GS.NAMES[g]}")


def test_solve_batch_of_shapes_under_forced_front_options(gpu_lib, hip_lib, monkeypatch):
    """(c) the front options of test_forced_plan_shapes_under_compaction's last case.  front_build may refuse a plan (a level of a
    piece wider than the packed tables hold); then the record kernels run the same cut.  Which family was held to the bar is decided by
    the host plan of the same graphs under the same options, and asserted."""
    from semantic_slam_amd import GraphSLAM
    env, front_there = BS.test_forced_plan_shapes_under_compaction.pytestmark[0].args[1][-1]
    assert front_there == 1 and env["front"] == "1"
    monkeypatch.setenv("SSLAM_CHOL_OPTS", ",".join(f"{k}={v}" for k, v in env.items()))
    gps = _ten()
    want = bool(Plan(hip_lib, [GraphSLAM.from_problem(gp) for gp in gps]).front)
    alone = {n: bool(Plan(hip_lib, [GraphSLAM.from_problem(gp)]).front) for n, gp in zip(GS.NAMES, gps)}
    _, B = BS._batch(gps)
    print(f"forced front options: the batch runs the {'front' if want else 'record'} kernels; front_build of each shape alone: {alone}")
    assert B.info("factor_front") == int(want)
    lam = BS._lams(10)
    full = B.solve(lam)
    for g, gp in enumerate(gps):
        BS._check(gp, full[g], lam[g], f"forced front options ({'front' if want else 'record'} kernels) {GS.NAMES[g]}")
    BS._masked_rounds(B, gps, full, lam, sample=(4, 6, 9))


def _stable_counts(gp, iters, st):
    """the oracle's iteration and trial counts do not move under three 1e-13 relative perturbations of the measurements (the
    distinction test_lm_endgame_compacts_once_most_of_the_batch_is_done draws: counts decided by last bits are not held to equality)"""
    rng = np.random.default_rng(0)
    for _ in range(3):
        q = gp.copy()
        q.meas = gp.meas * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, gp.meas.shape))
        s = q.optimize(iters)
        if (s.iterations, s.trials) != (st.iterations, st.trials):
            return False
    return True


def _optimize_against_oracle(gp, what, iters=10):
    """bars of test_optimize_small_graph_matches_oracle: chi2 before 1e-12, chi2 after 1e-6, estimates 1e-4 of the largest"""
    from semantic_slam_amd import GraphSLAM
    G = GraphSLAM.from_problem(gp)
    assert G.optimize(iters) is True
    ref = gp.copy()
    st = ref.optimize(iters)
    stable = _stable_counts(gp, iters, st)
    s = G.last_stats
    est_rel = np.abs(G.estimates() - ref.est).max() / np.abs(ref.est).max()
    print(f"{what}: chi2 {st.chi2_before:.6g} -> {st.chi2_after:.6g}; HIP iterations {s.iterations} trials {s.trials}, oracle {st.iterations} {st.trials} "
          f"(stable under 1e-13: {stable}); chi2 before rel {abs(s.chi2_before - st.chi2_before) / st.chi2_before:.3e} after rel "
          f"{abs(s.chi2_after - st.chi2_after) / st.chi2_after:.3e} estimates rel {est_rel:.3e}")
    assert s.chi2_before == pytest.approx(st.chi2_before, rel=1e-12)
    assert s.chi2_after == pytest.approx(st.chi2_after, rel=1e-6)
    assert est_rel <= 1e-4
    assert st.chi2_after < st.chi2_before
    if stable:
        assert (s.iterations, s.trials) == (st.iterations, st.trials)
    return G, ref


@pytest.mark.parametrize("name", ["hub_120x8", "k_obs32", "loop1", "two_chains", "second_fixed"])
def test_optimize_shape_matches_oracle(gpu_lib, name):
    gp = GS.problem(name)
    G, ref = _optimize_against_oracle(gp, name)
    fixed = np.nonzero(gp.vfixed)[0]
    assert np.array_equal(G.estimates()[fixed], gp.est[fixed])       # fixed vertices (two of them in the last two shapes) do not move


@pytest.fixture(scope="module")
def hub_inverse(gpu_lib):
    """the 300 x 4 hub after two LM iterations on a single handle, and the dense inverse of the oracle's H at those estimates"""
    from semantic_slam_amd import GraphSLAM
    gp = GS.problem("hub_300x4")
    G = GraphSLAM.from_problem(gp)
    assert G.optimize(2)
    gp.est[:] = G.estimates()
    return gp, G, BM._dense_inverse(gp)


def _hub_requests(gp):
    lm, po = [int(v) for v in gp.lm_ids], [int(v) for v in gp.pose_ids]
    return [(v, v) for v in lm] + [(po[1], po[1]), (po[-1], po[-1]), (po[150], lm[2]), (lm[2], po[150])]


def test_marginals_of_the_hub_single_handle(hub_inverse):
    """landmarks with 300 observers, the first and the last free pose, a pose-landmark pair: BM._close is the bar of
    test_three_distinct_graphs_match_the_dense_inverse (1e-6 of the block's largest entry)"""
    gp, G, Hinv = hub_inverse
    req = _hub_requests(gp)
    blocks = G.computeMarginals([(G.hessian_index(r), G.hessian_index(c)) for r, c in req])
    assert len(blocks) == len(req)
    for r, c in req:
        BM._close(blocks[(G.hessian_index(r), G.hessian_index(c))], BM._ref_block(gp, Hinv, r, c), f"hub block ({r}, {c})")
    diag = G.computeLandmarkMarginals([int(v) for v in gp.lm_ids])
    for v, a in zip(gp.lm_ids, diag):
        BM._close(a, BM._ref_block(gp, Hinv, int(v), int(v)), f"hub landmark {v} (diagonal call)")


def test_marginals_of_the_hub_in_a_batch_of_three(gpu_lib):
    from semantic_slam_amd import GraphSLAM, GraphBatch
    gps = [GS.problem(n) for n in ("hub_300x4", "hub_120x8", "chain")]
    graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(graphs)
    B.upload()
    B.optimize(2)
    B.download()
    req = []
    for g, gp in enumerate(gps):
        gp.est[:] = graphs[g].estimates()
        lm, po = [int(v) for v in gp.lm_ids], [int(v) for v in gp.pose_ids]
        req += [(g, v, v) for v in lm[:8]] + [(g, po[1], po[1]), (g, po[-1], po[-1]), (g, po[len(po) // 2], lm[2]), (g, lm[2], po[len(po) // 2])]
    blocks = B.marginals(req)
    Hinv = [BM._dense_inverse(gp) for gp in gps]
    assert len(blocks) == len(req)
    for (g, r, c), a in zip(req, blocks):
        BM._close(a, BM._ref_block(gps[g], Hinv[g], r, c), f"graph {g} block ({r}, {c})")


# ======== 2. point and plane landmarks in one graph ====================================================================================
MIXED = [(60, 12, 3), (150, 30, 5)]


@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("size", MIXED)
def test_mixed_linearize_matches_oracle(gpu_lib, size, interleave):
    """test_linearize_matches_oracle's two bars, each where it applies: 1e-11 on the blocks that no plane edge touches, 2e-5 on the
    others, both relative to abs(Uo).max() (b: to max(1, |b|))"""
    from semantic_slam_amd import GraphSLAM
    gp = GS.mixed_problem(*size, interleave=interleave)
    G = GraphSLAM.from_problem(gp)
    U, b = G.linearize()
    Uo, bo = gp.linearize()
    h, n = gp.hessian_index()
    assert [G.hessian_index(v) for v in range(gp.nv)] == list(h) and U.shape == Uo.shape == (n, n)
    rows = lambda v: np.arange(h[v], h[v] + (6 if gp.vtype[v] == 0 else 3)) if h[v] >= 0 else np.arange(0)
    touched = np.zeros((n, n), bool)
    tb = np.zeros(n, bool)
    for k in np.nonzero(gp.etype == 2)[0]:
        ri, rj = rows(gp.evi[k]), rows(gp.evj[k])
        for a in (ri, rj):
            tb[a] = True
            for c in (ri, rj):
                touched[np.ix_(a, c)] = True
    dH = np.abs((_full(U) - _full(Uo)).toarray()) / abs(Uo).max()
    db = np.abs(b - bo) / max(1.0, np.abs(bo).max())
    assert touched.any() and (~touched & (_full(Uo).toarray() != 0)).any() and tb.any() and (~tb).any()
    print(f"mixed {size} interleave {interleave}: H point blocks {dH[~touched].max():.3e} (bar 1e-11) plane blocks {dH[touched].max():.3e} (bar 2e-5); "
          f"b {db[~tb].max():.3e} / {db[tb].max():.3e}; chi2 rel {abs(G.chi2() - gp.chi2()) / gp.chi2():.3e}")
    assert dH[~touched].max() <= 1e-11 and db[~tb].max() <= 1e-11
    assert dH[touched].max() <= 2e-5 and db[tb].max() <= 2e-5
    assert abs(G.chi2() - gp.chi2()) <= 1e-12 * gp.chi2()


@pytest.mark.parametrize("size", MIXED)
def test_mixed_oplus_matches_oracle(gpu_lib, size):
    from semantic_slam_amd import GraphSLAM
    gp = GS.mixed_problem(*size, interleave=True)
    G = GraphSLAM.from_problem(gp)
    _, n = gp.hessian_index()
    dx = np.random.default_rng(0).normal(0, 0.05, n)
    G.oplus(dx)
    gp.oplus(dx)
    err = np.abs(G.estimates() - gp.est).max()
    print(f"mixed {size} oplus: max error {err:.3e} (bar 1e-13)")
    assert err < 1e-13                                               # test_oplus_matches_oracle


@pytest.mark.parametrize("size", MIXED)
def test_mixed_optimize_matches_oracle(gpu_lib, size):
    _optimize_against_oracle(GS.mixed_problem(*size, interleave=True), f"mixed {size}")


@pytest.mark.parametrize("size", MIXED)
def test_mixed_graph_in_a_batch_matches_its_single_handle(gpu_lib, size):
    """between a pure point and a pure plane graph; bars of test_batch_matches_individual"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    n, m, seed = size
    gps = [GraphProblem.from_synth(make_graph(n + 7, m + 1, seed=seed + 20)), GS.mixed_problem(n, m, seed, interleave=True),
           GraphProblem.from_synth(make_graph(n - 5, m - 1, seed=seed + 21, landmark_kind="plane"), interleave=True)]
    singles = [GraphSLAM.from_problem(gp) for gp in gps]
    for G in singles:
        G.optimize(8)
    batch_graphs = [GraphSLAM.from_problem(gp) for gp in gps]
    B = GraphBatch(batch_graphs)
    B.upload()
    stats = B.optimize(8)
    B.download()
    for k, (G1, G2, st) in enumerate(zip(singles, batch_graphs, stats)):
        d = np.abs(G1.estimates() - G2.estimates()).max()
        print(f"mixed {size} batch member {k}: iterations {st.iterations} / {G1.last_stats.iterations}, chi2 rel "
              f"{abs(st.chi2_after - G1.last_stats.chi2_after) / G1.last_stats.chi2_after:.3e}, estimates {d:.3e}")
    for G1, G2, st in zip(singles, batch_graphs, stats):
        assert st.iterations == G1.last_stats.iterations
        assert st.chi2_after == pytest.approx(G1.last_stats.chi2_after, rel=1e-9)
        assert np.abs(G1.estimates() - G2.estimates()).max() < 1e-9


@pytest.mark.parametrize("size", MIXED)
def test_mixed_edge_shards_sum_to_the_full_system(gpu_lib, size):
    """world = 8, as test_edge_shards_of_the_L_graph_sum_to_the_full_system does it: 1e-12 of the largest entry"""
    from semantic_slam_amd import GraphSLAM, GraphBatch
    from semantic_slam_amd.distributed import shard_range
    gp = GS.mixed_problem(*size, interleave=True)
    B = GraphBatch([GraphSLAM.from_problem(gp)]); B.upload()
    full = B.linearize_hb()
    tot = np.zeros_like(full)
    covered = 0
    for r in range(8):
        B.set_edge_shard(r, 8)
        part = B.linearize_hb()
        assert np.abs(part).max() > 0 and np.abs(part - full).max() > 0
        tot += part
        lo, hi = shard_range(gp.ne, r, 8)
        covered += hi - lo
    assert covered == gp.ne
    err = np.abs(tot - full).max() / np.abs(full).max()
    print(f"mixed {size}: sum of 8 edge shards against the full system {err:.3e} (bar 1e-12)")
    assert err <= 1e-12
    B.set_edge_shard(0, 1)
    assert np.array_equal(B.linearize_hb(), full)


# ======== 3. frontend: layout, geometry, smoothing =====================================================================================
def _box_products(seg, frame):
    return [(seg.labels(bi).copy(), seg.normals(bi).copy()) for bi in range(len(frame.boxes))]


def _ransac_records(seg):
    recs, _ = seg.ransac_boxes(0.01, 50, 0.99, 3)
    return [bytes(r) for r in recs]


@pytest.fixture(scope="module")
def plain(gpu_lib):
    """the plain 32-byte frames through the three entry points: what every layout has to reproduce"""
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    frames = [make_frame(**kw) for kw in CL.LAYOUT_BATCH]
    assert CL.LAYOUT_BATCH[0] == CL.LAYOUT_FRAME
    seg = PointCloudSegmentation()
    batch = seg.segment_frames(frames)
    batch_ransac = _ransac_records(seg)
    f = frames[0]
    planes = seg.segmentallPointCloudData(f.robot_pose, f.cam_angle, f.boxes, f)
    products = _box_products(seg, f)
    ransac = _ransac_records(seg)
    assert len(planes) >= 5 and len(ransac) == 32 and len(batch_ransac) == 96 and [len(x) for x in batch] == [8, 7, 6]
    return frames, planes, products, ransac, batch, batch_ransac


@pytest.mark.parametrize("layout", CL.LAYOUTS)
def test_cloud_layouts_give_the_plain_frame(plain, layout):
    """permuted field offsets, other point sizes and padded rows, every byte outside x, y, z a float 7.5e8, through the blocking call,
    the batched call and the pipelined submit / collect: plane records, label images and normals of the plain frame, bit for bit
    (np.array_equal, as test_seg_gpu.py); the crops k_crop left on the device give the plain frame's RANSAC records"""
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    frames, planes, products, ransac, batch, batch_ransac = plain
    relaid = [CL.relayout(f, *layout) for f in frames]
    f = relaid[0]
    seg = PointCloudSegmentation()
    TS._same_planes(seg.segmentallPointCloudData(f.robot_pose, f.cam_angle, f.boxes, f), planes)
    for bi, ((lab, nrm), (lab0, nrm0)) in enumerate(zip(_box_products(seg, f), products)):
        assert np.array_equal(lab, lab0), f"box {bi}: label image differs"
        assert np.array_equal(nrm, nrm0, equal_nan=True), f"box {bi}: normals differ"
    assert _ransac_records(seg) == ransac
    seg2 = PointCloudSegmentation()
    got = seg2.segment_frames(relaid)
    assert seg2.last_overflow() == (0, 0, 0)
    for a, r in zip(got, batch):
        TS._same_planes(a, r)
    assert _ransac_records(seg2) == batch_ransac
    streamed = list(PointCloudSegmentation().segment_stream([relaid, relaid[::-1]]))      # two batches in flight
    assert len(streamed) == 2
    for a, r in zip(streamed[0], batch):
        TS._same_planes(a, r)
    for a, r in zip(streamed[1], batch[::-1]):
        TS._same_planes(a, r)


def test_cloud_layout_in_the_tick(gpu_lib, tmp_path, monkeypatch):
    """test_tick_information_from_fitness's scene with a padded, permuted layout handed to setPointCloudData: the host read of the
    keyframe clouds (downsampled_cloud) gives the fitness scores and information matrices of the plain layout, bit for bit"""
    from semantic_slam_amd.segmentation import PointCloudSegmentation
    seg = PointCloudSegmentation()
    S0, frames0, zs0, infos0 = TF._run_tick(seg, True, tmp_path, "plain.g2o")
    score0, used0 = S0.last_fitness()
    odoms, frames = TF._tick_inputs()
    relaid = [CL.relayout(f, 20, (8, 0, 12), 28) for f in frames]
    assert relaid[0].row_step == 96 * 20 + 28 and np.array_equal(CL.read_xyz(relaid[0]).reshape(-1, 3), frames[0].xyz, equal_nan=True)
    monkeypatch.setattr(TF, "_tick_inputs", lambda: (odoms, relaid))
    S1, frames1, zs1, infos1 = TF._run_tick(seg, True, tmp_path, "padded.g2o")
    assert frames1[0].point_step == 20
    score1, used1 = S1.last_fitness()
    print(f"tick: scores {score0} used {used0}")
    assert len(score0) == 4 and int((used0 > 50).sum()) == 2          # the two edges between keyframes that both carry a cloud
    assert score1.tobytes() == score0.tobytes() and used1.tobytes() == used0.tobytes()
    const = np.diag([1.0 / 0.0667] * 6)
    assert sum(w.tobytes() != const.tobytes() for w in infos0) == 2
    for a, b in zip(infos1, infos0):
        assert a.tobytes() == b.tobytes()


def _compare_with_oracle(frame, seg, planes, ref, nrm, lab, boxes):
    off = 0
    nvalid = 0
    for bi in boxes:
        n = int(frame.boxes[bi]["width"]) * int(frame.boxes[bi]["height"])
        assert np.array_equal(seg.labels(bi).reshape(n), lab[off:off + n]), f"box {bi}: label image differs"
        gn, on = seg.normals(bi).reshape(n, 4), nrm[off:off + n]
        assert np.array_equal(gn, on, equal_nan=True), f"box {bi}: normals differ"
        nvalid += int((~np.isnan(on[:, 0])).sum())
        off += n
    assert len(planes) == len(ref)
    for a, r in zip(planes, ref):
        assert (a.box_index, a.inlier_count, a.num_points, a.area) == (r.box_index, r.inlier_count, r.num_points, r.area)
        assert a.plane_type == ("horizontal" if r.plane_type == 0 else "vertical")
        assert np.array_equal(a.pose, np.array(r.centroid_cam, np.float32))
        assert np.array_equal(a.normal_orientation, np.array(r.normal_d, np.float32))
        assert np.array_equal(a.world_pose, np.array(r.world_pose, np.float32))
    return nvalid


@pytest.mark.parametrize("seed,box_w,box_h", CL.BORDER_FRAMES)
def test_boxes_on_the_image_border(gpu_lib, seed, box_w, box_h):
    """boxes flush against the four edges and in the four corners, and three that stick out by one pixel, against the oracle"""
    f = CL.border_boxes(make_frame(seed=seed, n_boxes=1), box_w, box_h)
    assert f.boxes["tl_x"][1] + box_w == 640 and f.boxes["tl_y"][2] + box_h == 480 and f.boxes["tl_x"][8] + box_w == 641 and f.boxes["tl_y"][9] + box_h == 481
    seg, planes, ref, nrm, lab = TS._run_both(f)
    with_plane = {r.box_index for r in ref}
    print(f"border boxes {box_w} x {box_h}, seed {seed}: the oracle finds {len(ref)} planes in boxes {sorted(with_plane)}")
    assert with_plane & set(CL.RIGHT_EDGE) and with_plane & set(CL.BOTTOM_EDGE)       # the oracle alone: a plane on either far border
    assert not with_plane & set(CL.OUTSIDE) and not {a.box_index for a in planes} & set(CL.OUTSIDE)
    _compare_with_oracle(f, seg, planes, ref, nrm, lab, range(8))
    # the three outside boxes alone: nothing, on both sides
    only = f.boxes[list(CL.OUTSIDE)]
    assert seg.segmentallPointCloudData(f.robot_pose, f.cam_angle, only, f) == []
    from oracle.oracle import segment_frame
    import dataclasses
    assert segment_frame(dataclasses.replace(f, boxes=only), seg.params)[0] == []


def test_another_image_size(gpu_lib):
    """800 x 600 with one box as wide as the image: k_distance_map's band height kBandFloats / w - 1 and k_integral's staged row
    leave the values that 640 x 480 frames with 128-pixel boxes give them"""
    from semantic_slam_amd.segmentation import default_params
    f = make_frame(**CL.WIDE_FRAME)
    assert (f.width, f.height, f.row_step) == (800, 600, 800 * 32) and int(f.boxes["width"][0]) == 800
    P = default_params(); P.image_width = 800; P.image_height = 600
    seg, planes, ref, nrm, lab = TS._run_both(f, P)
    print(f"800 x 600, one 800 x 150 box: {len(ref)} planes")
    assert len(ref) >= 3
    _compare_with_oracle(f, seg, planes, ref, nrm, lab, [0])
    # the default 640 x 480 parameters drop the box on both sides (it crosses image_width)
    seg0, planes0, ref0, _, _ = TS._run_both(f)
    assert planes0 == [] and ref0 == []


@pytest.mark.parametrize("smoothing", [10.0, 30.0])
def test_normal_smoothing_size(gpu_lib, smoothing):
    """normal_smoothing_size sets the border and the window of k_normals; 20 everywhere else in the suite"""
    from semantic_slam_amd.segmentation import default_params
    f = make_frame(seed=0)
    P = default_params(); P.normal_smoothing_size = smoothing
    seg, planes, ref, nrm, lab = TS._run_both(f, P)
    nvalid = _compare_with_oracle(f, seg, planes, ref, nrm, lab, range(32))
    print(f"normal_smoothing_size {smoothing}: {len(ref)} planes, {nvalid} valid normals")
    assert nvalid > 10000                                            # test_frame_matches_oracle_bit_exact
    P20 = default_params()
    _, _, ref20, nrm20, _ = TS._run_both(f, P20)
    assert not np.array_equal(nrm20, nrm, equal_nan=True)            # the parameter reached the kernels


# ======== 4. association beyond one stride ===============================================================================================
@pytest.mark.parametrize("use_eq", [0, 1])
@pytest.mark.parametrize("quirk", [0, 1])
def test_association_beyond_one_stride(gpu_lib, quirk, use_eq):
    """test_association_kernel_matches_oracle's loop on tests/assoc_ties.py's frames: more than 600 landmarks (three strides of
    k_associate's 256 threads, every DevBuf doubling on the way), and detections at float-equal distance from two landmarks of their
    kind that are 256 and more indices apart -- the lower index wins, in the oracle and on the device"""
    from tests.slam_replay import product_instance, planes_of
    from oracle import np_slam as S
    F = np.float32
    P = product_instance(reference_quirks=quirk, use_maha_dist=0 if use_eq else 1, use_eq_dist=use_eq)
    D = S.DataAssociation(keep_distance_min=bool(quirk), use_maha_dist=not use_eq, use_eq_dist=bool(use_eq))
    ties, gaps = 0, set()
    for fi, (pose, objs, heads) in enumerate(AT.schedule(bool(use_eq), bool(quirk))):
        got = P.find_matches(planes_of(objs), pose)
        ref = D.find_matches(objs, pose, F(0.0), lambda l: l["pose"])
        assert [(g.is_new, g.id) for g in got] == [(int(r["is_new"]), r["id"]) for r in ref], f"frame {fi}"
        for g, r in zip(got, ref):
            assert np.array_equal(np.array(g.pose[:]), r["pose"]) and np.array_equal(np.array(g.local_pose[:]), r["local_pose"])
            assert np.array_equal(np.array(g.normal[:]), r["normal"])
            if r["distance"] >= 0:
                assert abs(g.distance - r["distance"]) <= 1e-4 * max(1.0, abs(r["distance"]))   # test_association_kernel_matches_oracle
        for k, kind in enumerate(heads):                             # the ties, from the oracle's own table and arithmetic
            lo, hi = AT.TIE_INDICES[AT.TIE_KINDS.index(kind)]
            dist = []
            for i in (lo, hi):
                l = D.landmarks[i]
                assert (l["class_id"], l["plane_type"]) == kind == (objs[k]["class_id"], objs[k]["plane_type"])
                z = np.array([F(ref[k]["pose"][c] - l["pose"][c]) for c in range(3)], F)
                dist.append(F(np.sqrt(F(F(F(z[0] * z[0]) + F(z[1] * z[1])) + F(z[2] * z[2])))) if use_eq else S.mahalanobis(l["covariance"], D.q, z))
            assert hi - lo >= 256 and dist[0] == dist[1] == F(ref[k]["distance"]) and dist[0] > 0
            assert (ref[k]["is_new"], ref[k]["id"]) == (False, lo) and (got[k].is_new, got[k].id) == (0, lo)
            assert got[k].distance == float(dist[0])
            ties += 1
            gaps.add((hi - lo == 256, lo // 64 == (hi % 256) // 64))
    n = len(D.landmarks)
    print(f"quirk {quirk} use_eq {use_eq}: {n} landmarks, {ties} ties")
    assert len(P.getMappedLandmarks()) == n > 600
    assert ties >= 3
    assert gaps == {(True, True), (False, True), (False, False)}    # one stride apart in a thread; two lanes of a wave; two waves
