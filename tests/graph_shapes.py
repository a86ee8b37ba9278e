"""Graph structures that synth.make_graph's defaults (k_obs=3, loop_every=50) never produce -- test helper, not collected.

With the defaults every pose row has 3 landmark slots and 2-3 EdgeSE3 slots, every landmark about 15 observers, a graph one landmark
kind, one fixed pose and one connected component.  The kernels whose trip counts and tables follow the degree (the row-thread and
landmark-row Jacobian kernels, the piece / group / tail / front kernels of the Cholesky plan, the marginal pair kernel) have seen that
one pattern only.  The table below varies it, at the smallest sizes that do (the largest system, hub_300x4, has 1806 unknowns):

    hub_120x8, hub_300x4, hub_plane_100x6   every pose sees every landmark: landmark rows with 100-300 edges
    k_obs32                                 32 detections per keyframe (the tick's upper bound): 32 landmark slots in every pose row
    k_obs12                                 12 per keyframe on few landmarks: ~24 observers each
    loop3, loop1                            a loop closure every third pose / one per pose: pose rows with many EdgeSE3 slots
    chain                                   a bare chain, one landmark edge per pose, no loop closure
    second_fixed                            a second fixed pose in the middle of the chain: edges into a fixed vertex from both sides
    two_chains                              two disjoint components in one graph, each with its own fixed first pose and landmarks

``mixed_problem`` builds a graph that holds point AND plane landmarks (the generator makes one kind per graph).
"""
from __future__ import annotations

import numpy as np

from oracle.oracle import GraphProblem, VT_PLANE, VT_SE3
from semantic_slam_amd.synth import make_graph


def _synth(n_poses, n_landmarks, seed, interleave, **kw):
    return lambda il=None: GraphProblem.from_synth(make_graph(n_poses, n_landmarks, seed=seed, **kw), interleave=interleave if il is None else il)


def _second_fixed(il=None):
    gp = GraphProblem.from_synth(make_graph(90, 18, seed=47), interleave=True if il is None else il)
    gp.vfixed[int(gp.pose_ids[45])] = 1
    return gp


def _two_chains(il=None):
    """two graphs side by side in one vertex / edge numbering (raw arrays): vertices of the first, then of the second; the edges of the
    two interleaved one by one, so that neither the vertex nor the edge order separates the components"""
    a = GraphProblem.from_synth(make_graph(50, 10, seed=48), interleave=bool(il))
    b = GraphProblem.from_synth(make_graph(40, 8, seed=49), interleave=True if il is None else il)
    order = np.argsort(np.concatenate([np.arange(a.ne) * 2.0, np.arange(b.ne) * 2.0 + 1.0]), kind="stable")
    cat = lambda x, y: np.concatenate([x, y])[order]
    gp = GraphProblem(np.concatenate([a.vtype, b.vtype]), np.concatenate([a.vfixed, b.vfixed]), np.concatenate([a.est, b.est]),
                      cat(a.etype, b.etype), cat(a.evi, b.evi + a.nv), cat(a.evj, b.evj + a.nv), cat(a.meas, b.meas), cat(a.info, b.info))
    gp.pose_ids = np.concatenate([a.pose_ids, b.pose_ids + a.nv])
    gp.lm_ids = np.concatenate([a.lm_ids, b.lm_ids + a.nv])
    assert int(gp.vfixed.sum()) == 2
    return gp


# name -> builder(interleave=None) of a fresh GraphProblem; None takes the shape's own vertex order (both orders occur in the table)
SHAPES = {
    "hub_120x8": _synth(120, 8, 41, False, k_obs=8),
    "hub_300x4": _synth(300, 4, 42, True, k_obs=4),
    "hub_plane_100x6": _synth(100, 6, 43, False, k_obs=6, landmark_kind="plane"),
    "k_obs32": _synth(100, 400, 44, True, k_obs=32),
    "k_obs12": _synth(200, 100, 45, False, k_obs=12),
    "loop3": _synth(240, 40, 46, True, loop_every=3),
    "loop1": _synth(150, 30, 50, False, loop_every=1),
    "chain": _synth(300, 3, 51, True, k_obs=1, loop_every=0),
    "second_fixed": _second_fixed,
    "two_chains": _two_chains,
}
NAMES = tuple(SHAPES)
PLANE_SHAPES = ("hub_plane_100x6",)

_cache = {}


def problem(name, interleave=None) -> GraphProblem:
    """a fresh copy of the named shape (built once per process: the generator's Python loops cost more than the tests' kernels)"""
    key = (name, interleave)
    if key not in _cache:
        _cache[key] = SHAPES[name](interleave)
    return _cache[key].copy()


def degrees(gp):
    """(largest number of landmark edges of a pose, largest number of EdgeSE3 ends at a pose, largest number of observers of a landmark)"""
    lm = gp.etype != 0
    per_pose = np.bincount(gp.evi[lm], minlength=gp.nv).max() if lm.any() else 0
    se3 = np.bincount(np.concatenate([gp.evi[~lm], gp.evj[~lm]]), minlength=gp.nv).max()
    per_lm = np.bincount(gp.evj[lm], minlength=gp.nv).max() if lm.any() else 0
    return int(per_pose), int(se3), int(per_lm)


def mixed_problem(n_poses, n_landmarks, seed, interleave=False) -> GraphProblem:
    """Point and plane landmarks in one graph: the odd-numbered landmarks (and their edges) of make_graph(..., landmark_kind="plane"),
    the others of the same call with "point".  The two calls draw the trajectory, the observations and the odometry before they
    branch on the kind, so they share every vertex id and every edge's end points."""
    pt = GraphProblem.from_synth(make_graph(n_poses, n_landmarks, seed=seed, landmark_kind="point"), interleave=interleave)
    pl = GraphProblem.from_synth(make_graph(n_poses, n_landmarks, seed=seed, landmark_kind="plane"), interleave=interleave)
    assert np.array_equal(pt.evi, pl.evi) and np.array_equal(pt.evj, pl.evj) and np.array_equal(pt.lm_ids, pl.lm_ids)
    assert np.array_equal(pt.est[pt.pose_ids], pl.est[pl.pose_ids])
    plane_v = np.zeros(pt.nv, bool)
    plane_v[pl.lm_ids[1::2]] = True
    e = plane_v[pt.evj] & (pt.etype != 0)
    pick_v = lambda a, b: np.where(plane_v.reshape(-1, *[1] * (a.ndim - 1)), b, a)
    pick_e = lambda a, b: np.where(e.reshape(-1, *[1] * (a.ndim - 1)), b, a)
    gp = GraphProblem(pick_v(pt.vtype, pl.vtype), pt.vfixed.copy(), pick_v(pt.est, pl.est), pick_e(pt.etype, pl.etype), pt.evi.copy(), pt.evj.copy(),
                      pick_e(pt.meas, pl.meas), pick_e(pt.info, pl.info))
    gp.pose_ids, gp.lm_ids = pt.pose_ids, pt.lm_ids
    assert int((gp.vtype == VT_PLANE).sum()) == n_landmarks // 2 and int(e.sum()) > 0
    gp.plane_vertex = plane_v
    gp.pure = (pt, pl)
    return gp
