"""Reference for the loop-closure tests, in NumPy and plain Python floats:

* the host arithmetic of the tick that a prediction must repeat bit for bit -- the keyframe gate's travelled distance, the initial guess
  T0 = estimate_new^-1 * estimate_cand and the measurement of a T -- restated operation for operation from csrc/sslam_slam.hip and
  csrc/sslam_math.hpp (IEEE doubles, left to right, no fused multiply-add);
* candidates_ref: LoopDetector::find_candidates as include/sslam.h states it for sslam_slam_loop_candidates;
* predict_tick: pre-filter, candidates, registration (through a function the caller hands in: the NumPy ICP on the CPU, the device's
  register_pairs on the GPU), best-pair selection and the sequential last-edge walk;
* LoopOracle: oracle/np_slam.py's tick with given loop edges injected where the product's tick adds them."""
import math
import types

import numpy as np

from fitness_ref import DBL_MAX, fitness_ref, information_ref, qmat
from oracle import np_slam as S
from oracle import oracle as O
from registration_ref import icp_ref

ADDED, SCORE, GATE, NO_MATCH = 0, 1, 2, 3      # SSLAM_LOOP_*


# ---- the host arithmetic of csrc/sslam_slam.hip, operation for operation ---------------------------------------------------------------
def qnormalized(q):
    x, y, z, w = q
    n = math.sqrt(x * x + y * y + z * z + w * w)
    return (x / n, y / n, z / n, w / n)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz)


def qconj(q):
    return (-q[0], -q[1], -q[2], q[3])


def qrot(q, v):
    R = qmat(q)
    return (R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2], R[6] * v[0] + R[7] * v[1] + R[8] * v[2])


def from_tq(v):
    v = [float(x) for x in v]
    return ((v[0], v[1], v[2]), qnormalized((v[3], v[4], v[5], v[6])))


def to_tq(p):
    return np.array([p[0][0], p[0][1], p[0][2], p[1][0], p[1][1], p[1][2], p[1][3]])


def inverse(p):
    qi = qconj(p[1])
    t = qrot(qi, p[0])
    return ((-t[0], -t[1], -t[2]), qi)


def compose(a, b):
    r = qrot(a[1], b[0])
    return ((a[0][0] + r[0], a[0][1] + r[1], a[0][2] + r[2]), qnormalized(qmul(a[1], b[1])))


def guess_T(est_new, est_cand):
    """T0 of a (new, candidate) pair: 12 doubles, R row-major then t"""
    rel = compose(inverse(from_tq(est_new)), from_tq(est_cand))
    return np.array(list(qmat(rel[1])) + list(rel[0]))


def measurement_of_T(T):
    """(t, q xyzw) of a T: the quaternion of a rotation matrix by the branch with the largest pivot, as INTEGRATION.md section 2 has it"""
    R = [float(x) for x in T]
    z = [R[9], R[10], R[11], 0.0, 0.0, 0.0, 1.0]
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = 2 * math.sqrt(1 + tr); z[6] = s / 4; z[3] = (R[7] - R[5]) / s; z[4] = (R[2] - R[6]) / s; z[5] = (R[3] - R[1]) / s
    elif R[0] > R[4] and R[0] > R[8]:
        s = 2 * math.sqrt(1 + R[0] - R[4] - R[8]); z[3] = s / 4; z[6] = (R[7] - R[5]) / s; z[4] = (R[1] + R[3]) / s; z[5] = (R[2] + R[6]) / s
    elif R[4] > R[8]:
        s = 2 * math.sqrt(1 + R[4] - R[0] - R[8]); z[4] = s / 4; z[6] = (R[2] - R[6]) / s; z[3] = (R[1] + R[3]) / s; z[5] = (R[5] + R[7]) / s
    else:
        s = 2 * math.sqrt(1 + R[8] - R[0] - R[4]); z[5] = s / 4; z[6] = (R[3] - R[1]) / s; z[3] = (R[2] + R[6]) / s; z[4] = (R[5] + R[7]) / s
    return np.array(z)


class KeyframeTrack:
    """KeyframeUpdater::update as sslam_slam_vio runs it: which samples become keyframes, and the travelled distance each one carries"""

    def __init__(self, delta_trans=0.5, delta_angle=0.5, delta_time=1.0):
        self.dt, self.da, self.dtime = delta_trans, delta_angle, delta_time
        self.first, self.prev, self.stamp, self.accum = True, None, (0, 0), 0.0

    def update(self, stamp, odom_tq):
        odom = from_tq(odom_tq)
        if self.first:
            self.first, self.prev, self.stamp = False, odom, stamp
            return True
        delta = compose(inverse(self.prev), odom)
        t = delta[0]
        dx = math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
        da = math.acos(min(1.0, abs(delta[1][3])))
        dsec, dnsec = stamp[0] - self.stamp[0], stamp[1] - self.stamp[1]
        if dnsec < 0:
            dsec -= 1
        if dsec < self.dtime and dx < self.dt and da < self.da:
            return False
        self.accum += dx
        self.prev, self.stamp = odom, stamp
        return True


# ---- LoopDetector::find_candidates -------------------------------------------------------------------------------------------------------
def candidates_ref(keys, news, accum_distance_thresh, distance_thresh, max_candidates=0, cap=None):
    """(cand [n_new, cap] int32 with -1 where not filled, count [n_new] int32) of sslam_slam_loop_candidates, in float64"""
    keys = np.asarray(keys, np.float64).reshape(-1, 3)
    news = np.asarray(news, np.float64).reshape(-1, 3)
    if cap is None:
        cap = max_candidates if max_candidates else len(keys)
    d2t = np.float64(distance_thresh) * np.float64(distance_thresh)
    cand = np.full((len(news), cap), -1, np.int32)
    count = np.zeros(len(news), np.int32)
    with np.errstate(all="ignore"):
        for n, q in enumerate(news):
            dx, dy, da = q[0] - keys[:, 0], q[1] - keys[:, 1], q[2] - keys[:, 2]
            d2 = dx * dx + dy * dy
            ok = np.isfinite(keys).all(1) & np.isfinite(q).all() & np.isfinite(da) & np.isfinite(d2) & (da >= accum_distance_thresh) & (d2 <= d2t)
            idx = np.nonzero(ok)[0]
            if max_candidates:
                idx = idx[np.lexsort((idx, d2[idx]))][:max_candidates]     # by (d2, index)
            count[n] = len(idx)
            cand[n, :min(cap, len(idx))] = idx[:cap]
    return cand, count


# ---- the tick ----------------------------------------------------------------------------------------------------------------------------
def loop_params(**kw):
    """the fields of sslam_loop_params with sslam_loop_default_params' values, as a plain namespace"""
    p = dict(distance_thresh=5.0, accum_distance_thresh=8.0, distance_from_last_edge_thresh=5.0, fitness_score_max_range=DBL_MAX,
             fitness_score_thresh=0.5, max_iterations=64, epsilon=0.01, max_candidates=0, voxel_leaf=0.1, gate_chi2=0.0, robust_kernel=1,
             robust_delta=1.0, inf=(20.0, 0.1, 5.0, 0.05, 0.2, 0.5))
    p.update(kw)
    return types.SimpleNamespace(**p)


def register_ref(clouds, pairs, max_iterations, epsilon):
    """the registration of predict_tick on the reference chain: registration_ref.icp_ref, then fitness_ref.fitness_ref at its T"""
    out = []
    for tgt, src, T0, mc2 in pairs:
        T, it, conv, status = icp_ref(clouds[tgt], clouds[src], T0, mc2, max_iterations, epsilon)
        score, used, _, _ = fitness_ref(clouds[tgt], clouds[src], T, mc2)
        out.append(types.SimpleNamespace(T=T, score=score, used=used, iterations=it, converged=conv, status=status))
    return out


def predict_tick(olds, news, last_edge_accum, P, register, information):
    """What a tick with loop closure on does with its keyframes.  olds / news: dicts with node, est (7 doubles), accum and cloud ([m, 3]
    float32, or None) of the processed / the new keyframes, in order.  register(clouds, pairs, max_iterations, epsilon) -> results with T,
    score, used, iterations, converged, status, for pairs (target, source, T0, max_corr2); information(score) -> 6 x 6.  The gate is not
    predicted (gate_chi2 = 0).  Returns (records, last_edge_accum, skipped): the records as dicts -- the fields of sslam_loop plus z, info
    and margin, the relative distance of the best score from the runner-up and from the threshold; skipped counts the new keyframes
    the running last-edge rule passed over although the tick's starting value let them through."""
    key_of = [k for k, o in enumerate(olds) if o["cloud"] is not None and len(o["cloud"])]
    new_of = [j for j, n in enumerate(news) if n["cloud"] is not None and len(n["cloud"]) and
              not (n["accum"] - last_edge_accum < P.distance_from_last_edge_thresh)]
    if not key_of or not new_of:
        return [], last_edge_accum, 0
    keys = [[olds[k]["est"][0], olds[k]["est"][1], olds[k]["accum"]] for k in key_of]
    qs = [[news[j]["est"][0], news[j]["est"][1], news[j]["accum"]] for j in new_of]
    cand, count = candidates_ref(keys, qs, P.accum_distance_thresh, P.distance_thresh, P.max_candidates)
    clouds, pairs, first = [], [], []
    slot = {}
    for r, j in enumerate(new_of):
        first.append(len(pairs))
        if count[r] == 0:
            continue
        clouds.append(news[j]["cloud"]); target = len(clouds) - 1
        for k in cand[r, :count[r]]:
            if k not in slot:
                clouds.append(olds[key_of[k]]["cloud"]); slot[k] = len(clouds) - 1
            pairs.append((target, slot[k], guess_T(news[j]["est"], olds[key_of[k]]["est"]), P.fitness_score_max_range))
    reg = register(clouds, pairs, P.max_iterations, P.epsilon) if pairs else []
    records, skipped = [], 0
    for r, j in enumerate(new_of):
        n = news[j]
        if n["accum"] - last_edge_accum < P.distance_from_last_edge_thresh:
            skipped += 1
            continue
        if count[r] == 0:
            continue
        ok = sorted((reg[first[r] + c].score, int(cand[r, c]), first[r] + c) for c in range(count[r])
                    if reg[first[r] + c].status == 0 and reg[first[r] + c].used > 0)
        rec = dict(new_vertex=n["node"], cand_vertex=-1, n_candidates=int(count[r]), outcome=NO_MATCH, edge_id=-1, used=0, iterations=0, converged=0,
                   T=np.zeros(12), score=DBL_MAX, d2=math.nan, new_index=j, cand_index=-1, margin=math.inf)
        if ok:
            score, k, pair = ok[0]
            g = reg[pair]
            rivals = [s for s, _, _ in ok[1:]] + [P.fitness_score_thresh]
            rec.update(cand_vertex=olds[key_of[k]]["node"], cand_index=key_of[k], T=np.array(g.T, np.float64), score=score, used=g.used,
                       iterations=g.iterations, converged=g.converged, margin=min(abs(score - s) / max(abs(score), abs(s)) for s in rivals))
            if score > P.fitness_score_thresh:
                rec["outcome"] = SCORE
            else:
                rec.update(outcome=ADDED, z=measurement_of_T(g.T), info=np.asarray(information(score), np.float64).reshape(6, 6))
                last_edge_accum = n["accum"]
        records.append(rec)
    return records, last_edge_accum, skipped


class LoopOracle(S.SemanticGraphSlam):
    """oracle/np_slam.py's tick with the loop edges of `pending_loops` -- (new vertex, candidate vertex, z, info) -- added after the
    association loop and before the new keyframes move to `keyframes`, where the product's tick adds them.  run() is the base class's
    but for that insertion and for the landmark marginals, which a replay without landmarks does not have."""

    pending_loops = ()

    def run(self):
        if not self._empty_keyframe_queue():
            return False
        stats = dict(keyframes_added=len(self.new_keyframes), landmarks_added=0, landmarks_matched=0, landmark_edges_added=0,
                     optimized=False, marginals_ok=False, records=[])
        for kf in self.new_keyframes:
            if kf["boxes"] is not None and len(kf["boxes"]) > 0:
                kf["objects"] = self._segment(kf)
                kf["cloud"] = None
            if not kf["objects"]:
                continue
            rp = S.matrix2vector(kf["robot_pose"])
            cur = self.assoc.find_matches(kf["objects"], rp, S.F(self.cam_angle), self._estimate_of)
            stats["records"].append(cur)
            self._landmark_edges(cur, kf, stats)
        for i, j, z, info in self.pending_loops:
            self._add_edge(O.ET_SE3, i, j, np.asarray(z, float), np.asarray(info, float))
        self.pending_loops = ()
        self.keyframes += self.new_keyframes
        self.new_keyframes = []
        if len(self.etype) >= 10:
            gp = self.problem()
            st = gp.optimize(self.max_iterations)
            self.est = [e.copy() for e in gp.est]
            stats["optimized"] = True
            stats["opt"] = st
            stats["marginals_ok"] = True                 # no landmarks in the loop replays: computeMarginals over an empty list
            assert not self.assoc.landmarks
            last = self.keyframes[-1]
            self.robot_pose = S.tq_to_iso(self.est[last["node"]])
            self.map2odom = S._mm4(self.robot_pose, S.iso_inv(last["odom"]))
        self.first_key_added = True
        self.last_stats = stats
        return True


def information_of(P):
    return lambda score: information_ref(score, P.inf)


class Replay:
    """Feeds loop_scene events to a system and keeps what a prediction of its ticks needs: per keyframe the estimate its vertex is added
    with, the travelled distance and the downsampled cloud.  `downsample(xyz, leaf)` -> [m, 3] float32."""

    def __init__(self, P, downsample, max_keyframes_per_update=10):
        self.P, self.downsample, self.max_kf = P, downsample, max_keyframes_per_update
        self.track = KeyframeTrack()
        self.queue, self.keyframes = [], []
        self.last_edge_accum = 0.0
        self.n_vertices = 0

    def sample(self, ev):
        """-> whether the sample becomes a keyframe"""
        if not self.track.update(ev.stamp, ev.odom):
            return False
        self.queue.append(dict(est=to_tq(from_tq(ev.odom)), accum=self.track.accum, raw=ev.cloud.xyz(), truth=ev.truth, cloud=None, node=-1))
        return True

    def begin_tick(self, old_estimates):
        """the keyframes the tick takes from the queue, numbered and downsampled; `old_estimates` [n, 7]: the processed keyframes' now"""
        news = self.queue[:self.max_kf]
        del self.queue[:len(news)]
        for n in news:
            n["node"] = self.n_vertices; self.n_vertices += 1
            n["cloud"] = np.ascontiguousarray(self.downsample(n.pop("raw"), self.P.voxel_leaf), np.float32)
        assert len(old_estimates) == len(self.keyframes)
        for k, e in zip(self.keyframes, old_estimates):
            k["est"] = np.array(e, np.float64)
        return news

    def predict(self, news, register):
        records, self.last_edge_accum, skipped = predict_tick(self.keyframes, news, self.last_edge_accum, self.P, register, information_of(self.P))
        return records, skipped

    def end_tick(self, news):
        self.keyframes += news


def oracle_replay(events, P, loops, downsample, register=register_ref):
    """The events through LoopOracle, tick by tick, with the reference chain's loops injected (`loops` False: none, the plain odometry
    graph).  Returns a namespace: oracle, replay, ticks -- per tick (news, records, skipped) -- and rms, the root mean square position
    error of the keyframes against the truth."""
    import loop_scene
    Or = LoopOracle(const_stddev_x=loop_scene.ODOM_STDDEV_X, const_stddev_q=loop_scene.ODOM_STDDEV_Q)
    R = Replay(P, downsample)
    ticks = []
    for ev in events:
        assert R.sample(ev) == bool(Or.vio(ev.stamp[0], ev.stamp[1], ev.odom))
        if not ev.run_after:
            continue
        news = R.begin_tick([Or.est[kf["node"]] for kf in Or.keyframes])
        records, skipped = R.predict(news, register) if loops else ([], 0)
        Or.pending_loops = [(r["new_vertex"], r["cand_vertex"], r["z"], r["info"]) for r in records if r["outcome"] == ADDED]
        assert Or.run()
        R.end_tick(news)
        assert [k["node"] for k in Or.keyframes] == [k["node"] for k in R.keyframes]
        ticks.append((news, records, skipped))
    est = np.array([Or.est[kf["node"]] for kf in Or.keyframes])
    rms = loop_scene.rms_position_error(est, np.array([k["truth"] for k in R.keyframes]))
    return types.SimpleNamespace(oracle=Or, replay=R, ticks=ticks, rms=rms)
