"""The device tables of a batch (semantic_slam_amd/csrc/batch_tables.hpp), read back through the plan introspection -- no GPU needed.

Two graphs: a hand-built one that holds every case in which a table can go wrong (fixed poses, an edge-less vertex, swapped and
repeated pose pairs, a landmark seen twice by one pose, point-point edges in both orientations, priors), and a plane graph of the
generator behind it, so that every offset of the second graph is non-zero.

  * test_tables_match_recorded_fixture: every table, bit for bit, against tests/golden/batch_tables_mixed.npz, which was recorded from
    the batch build as it was BEFORE it was split into batch_compile / batch_upload (tests/golden/make_golden.py make_batch_tables).
  * test_table_invariants: what the kernels rely on, derived in NumPy from the graphs' inputs alone."""
import ctypes as C
import os

import numpy as np

from semantic_slam_amd import GraphSLAM, load_library
from semantic_slam_amd.synth import make_graph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_tables_mixed.npz")

SE3, POINT, PLANE = 0, 1, 2                       # vertex types
E_SE3, E_POINT, E_PLANE, E_PP, E_PXY, E_PXYZ = range(6)   # edge types
CLASS_OF = {E_SE3: "eo", E_POINT: "el", E_PLANE: "el", E_PP: "ell", E_PXY: "ep", E_PXYZ: "ep"}
CLASS_NZ = {"eo": 7, "el": 4, "ell": 3, "ep": 3}  # rows of a class's z payload
CLASS_D = {"eo": 6, "el": 3, "ell": 3, "ep": 3}   # dimension of a class's information matrices

# name -> dtype of every exported table (int32 unless listed)
TABLES = ["seg", "pose_row", "lm_row", "prow_pose", "lrow_lm", "prow_graph", "lrow_graph", "pose_vertex", "lm_vertex", "lm_kind", "prow_perm",
          "ppoff", "plblk", "llblk",
          "eo_a", "eo_b", "eo_blk", "eo_id", "eo_z", "eo_w", "el_a", "el_b", "el_blk", "el_id", "el_z", "el_w",
          "ell_a", "ell_b", "ell_blk", "ell_id", "ell_z", "ell_w", "ep_a", "ep_id", "ep_z", "ep_w", "ep_dim",
          "pslot_ptr", "pslot_rec", "lslot_ptr", "lslot_edge", "llslot_ptr", "llslot_rec", "llblk_ptr", "llblk_edge",
          "dup_eo", "dup_el", "ep_row", "ep_ptr", "ep_edge", "adj_ptr", "adj_blk", "adj_x", "adj_fmt", "shard_lo", "shard_hi"]
DTYPES = {"lm_kind": np.uint8, "adj_fmt": np.uint8}
DTYPES.update({f"{c}_{p}": np.float64 for c in ("eo", "el", "ell", "ep") for p in ("z", "w")})
SEG_FIELDS = ("prow0", "nprow", "lrow0", "nlrow", "eo0", "neo", "el0", "nel", "pose0", "npose", "lm0", "nlm", "ell0", "nell", "ep0", "nep")


class Recorded:
    """A GraphSLAM and, next to it, what went into it: vertex types / fixed flags and (type, i, j, z, information) of every edge."""

    def __init__(self):
        self.G = GraphSLAM()
        self.vtype, self.fixed, self.edges = [], [], []

    def pose(self, xyz, fixed=-1):
        self.vtype.append(SE3)
        self.fixed.append(len(self.vtype) == 1 if fixed < 0 else bool(fixed))
        return self.G.add_se3_node(np.array([*xyz, 0.0, 0.0, 0.0, 1.0]), fixed)

    def point(self, xyz):
        self.vtype.append(POINT); self.fixed.append(False)
        return self.G.add_point_xyz_node(xyz)

    def plane(self, nd):
        self.vtype.append(PLANE); self.fixed.append(False)
        return self.G.add_plane_node(nd)

    def edge(self, etype, i, j, z, info):
        z, info = np.asarray(z, np.float64), np.asarray(info, np.float64)
        add = {E_SE3: self.G.add_se3_edge, E_POINT: self.G.add_se3_point_xyz_edge, E_PLANE: self.G.add_se3_plane_edge,
               E_PP: self.G.add_point_xyz_point_xyz_edge}.get(etype)
        if add:
            add(i, j, z, info)
        elif etype == E_PXY:
            self.G.add_se3_prior_xy_edge(i, z, info)
        else:
            self.G.add_se3_prior_xyz_edge(i, z, info)
        if etype == E_PLANE:   # the library stores the measured plane with a unit normal
            z = z / np.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2])
        self.edges.append((etype, i, j, z, info))


def spd(rng, d):
    a = rng.normal(size=(d, d))
    w = a @ a.T + d * np.eye(d)
    return (w + w.T) / 2     # exactly symmetric and dense: every entry of the upper triangle is distinct


def mixed_graph():
    rng = np.random.default_rng(5)
    R = Recorded()
    p = [R.pose((k, 0.1 * k, 0.0), fixed=1 if k == 4 else -1) for k in range(8)]   # pose 0 fixed (first), pose 4 fixed in mid-chain
    q = [R.point((k, 2.0, 0.5)) for k in range(3)]                                # q[2]: only a point-point edge reaches it
    lonely = R.point((9.0, 9.0, 9.0))                                             # no edge at all
    pl = [R.plane((0.0, 0.6, 0.8, 1.0 + k)) for k in range(2)]
    assert lonely == 11
    se3 = lambda: np.array([*rng.normal(size=3), 0.0, 0.0, 0.0, 1.0])
    E = R.edge
    for k in range(7):
        E(E_SE3, p[k], p[k + 1], se3(), spd(rng, 6))            # the chain: into each fixed pose from both sides (0-1, 3-4, 4-5)
    E(E_SE3, p[6], p[2], se3(), spd(rng, 6))                     # i > j: swap bit
    E(E_SE3, p[2], p[6], se3(), spd(rng, 6))                     # the same pair again, other orientation: a duplicate
    E(E_SE3, p[6], p[2], se3(), spd(rng, 6))                     # and a third time
    E(E_SE3, p[3], p[0], se3(), spd(rng, 6))                     # the first (fixed) pose as the second end
    E(E_POINT, p[1], q[0], rng.normal(size=3), spd(rng, 3))
    E(E_PLANE, p[1], pl[0], (0.1, 0.5, 0.9, 1.1), spd(rng, 3))
    E(E_POINT, p[1], q[0], rng.normal(size=3), spd(rng, 3))      # observed twice by one pose: a duplicate pose-landmark block
    E(E_POINT, p[4], q[1], rng.normal(size=3), spd(rng, 3))      # from a fixed pose
    E(E_POINT, p[5], q[1], rng.normal(size=3), spd(rng, 3))
    E(E_PXY, p[3], -1, rng.normal(size=2), spd(rng, 2))
    E(E_PP, q[0], q[1], rng.normal(size=3), spd(rng, 3))
    E(E_PLANE, p[7], pl[1], (0.0, 0.7, 0.7, 2.0), spd(rng, 3))
    E(E_PP, q[1], q[0], rng.normal(size=3), spd(rng, 3))         # the same landmark pair, other orientation
    E(E_PXYZ, p[3], -1, rng.normal(size=3), spd(rng, 3))             # both kinds of prior on one pose
    E(E_PP, q[1], q[2], rng.normal(size=3), spd(rng, 3))         # q[2] has no other edge
    E(E_PXYZ, p[4], -1, rng.normal(size=3), spd(rng, 3))             # a prior on a fixed pose
    E(E_PLANE, p[5], pl[0], (0.1, 0.5, 0.9, 1.1), spd(rng, 3))
    return R


def synth_graph():
    g = make_graph(12, 4, landmark_kind="plane")
    R = Recorded.__new__(Recorded)
    R.G = GraphSLAM.from_synth(g)
    R.vtype = [SE3] * g.n_poses + [PLANE] * len(g.lms_init)
    R.fixed = [v == 0 for v in range(len(R.vtype))]
    R.edges = [(E_SE3, int(i), int(j), np.asarray(z, np.float64), np.asarray(w, np.float64).reshape(6, 6))
               for (i, j), z, w in zip(g.odom_ij, g.odom_z, g.odom_info)]
    for (i, l), z, w in zip(g.lm_ij, np.asarray(g.lm_z, np.float64), g.lm_info):
        R.edges.append((E_PLANE, int(i), g.n_poses + int(l), z / np.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]), np.asarray(w, np.float64).reshape(3, 3)))
    return R


def read_tables(graphs):
    """name -> array of every table the plan introspection serves for the batch of `graphs` (GraphSLAM objects)"""
    lib = load_library()
    arr = (C.c_void_p * len(graphs))(*[g._h for g in graphs])
    h = lib.sslam_debug_plan_create(arr, len(graphs))
    assert h, lib.sslam_last_error().decode()
    out = {}
    try:
        for name in TABLES:
            n = lib.sslam_debug_plan_array(h, name.encode(), None, 0)
            assert n >= 0, lib.sslam_last_error().decode()
            buf = np.zeros(max(n, 1), np.uint8)
            lib.sslam_debug_plan_array(h, name.encode(), buf.ctypes.data, n)
            out[name] = buf[:n].view(DTYPES.get(name, np.int32)).copy()
    finally:
        lib.sslam_debug_plan_destroy(h)
    return out


_CACHE = {}


def batch():
    if not _CACHE:
        _CACHE["graphs"] = [mixed_graph(), synth_graph()]
        _CACHE["tables"] = read_tables([R.G for R in _CACHE["graphs"]])
    return _CACHE["graphs"], _CACHE["tables"]


def test_tables_match_recorded_fixture():
    _, T = batch()
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(TABLES)
    for name in TABLES:
        assert gold[name].dtype == T[name].dtype and np.array_equal(gold[name], T[name]), name


def test_table_invariants():
    graphs, T = batch()
    seg = T["seg"].reshape(len(graphs), 16)
    S = [dict(zip(SEG_FIELDS, (int(x) for x in row))) for row in seg]
    n_of = {c: len(T[f"{c}_id"]) for c in CLASS_NZ}
    z = {c: T[f"{c}_z"].reshape(CLASS_NZ[c], n_of[c]) for c in CLASS_NZ}
    w = {c: T[f"{c}_w"].reshape(CLASS_D[c] * (CLASS_D[c] + 1) // 2, n_of[c]) for c in CLASS_NZ}
    pose_row, lm_row = T["pose_row"], T["lm_row"]
    n_pr, n_lr = len(T["prow_pose"]), len(T["lrow_lm"])
    assert S[1]["prow0"] > 0 and S[1]["lrow0"] > 0 and S[1]["eo0"] > 0 and S[1]["el0"] > 0 and S[1]["pose0"] > 0 and S[1]["lm0"] > 0

    # ---- the expected side, from the inputs alone: rows, classes in (graph, edge id) order, payloads
    row_of = []            # per graph: vertex -> ('p' | 'l', row) or None
    exp = {c: [] for c in CLASS_NZ}     # class -> [(graph, edge id, row of end a, row of end b, z padded, upper triangle padded)]
    npr = nlr = 0
    for g, R in enumerate(graphs):
        has_edge = set()
        for _, i, j, _, _ in R.edges:
            has_edge.add(i)
            if j is not None and j >= 0:
                has_edge.add(j)
        rows = []
        for v, (t, fx) in enumerate(zip(R.vtype, R.fixed)):
            if fx or v not in has_edge:
                rows.append(None)
            elif t == SE3:
                rows.append(("p", npr)); npr += 1
            else:
                rows.append(("l", nlr)); nlr += 1
        row_of.append(rows)
        for k, (t, i, j, zk, info) in enumerate(R.edges):
            c = CLASS_OF[t]
            d, D = info.shape[0], CLASS_D[c]
            full = np.zeros((D, D)); full[:d, :d] = info
            zp = np.zeros(CLASS_NZ[c]); zp[:len(zk)] = zk
            ra = rows[i][1] if rows[i] else -1
            rb = (rows[j][1] if rows[j] else -1) if j >= 0 else -1
            exp[c].append((g, k, ra, rb, zp, full[np.triu_indices(D)], d))
    assert (npr, nlr) == (n_pr, n_lr)

    # ---- z / w columns are the graphs' measurements and the upper triangles of their information matrices; ids, ends, order
    for c, ends in (("eo", (pose_row, pose_row)), ("el", (pose_row, lm_row)), ("ell", (lm_row, lm_row)), ("ep", (pose_row, None))):
        assert n_of[c] == len(exp[c])
        first = {"eo": "eo0", "el": "el0", "ell": "ell0", "ep": "ep0"}[c]
        for k, (g, eid, ra, rb, zp, up, d) in enumerate(exp[c]):
            assert T[f"{c}_id"][k] == eid and S[g][first] <= k < S[g][first] + S[g]["n" + first[:-1]]
            assert np.array_equal(z[c][:, k], zp) and np.array_equal(w[c][:, k], up), (c, k)
            assert ends[0][T[f"{c}_a"][k]] == ra
            if ends[1] is not None:
                assert ends[1][T[f"{c}_b"][k]] == rb
            else:
                assert T["ep_dim"][k] == d

    # ---- slots: every active end of every edge exactly once in its row's list, in edge order (pose rows: EdgeSE3 ends, then landmark edges)
    want_p = [[] for _ in range(n_pr)]
    want_l = [[] for _ in range(n_lr)]
    want_ll = [[] for _ in range(n_lr)]
    want_ep = [[] for _ in range(n_pr)]
    for k, (_, _, ra, rb, *_r) in enumerate(exp["eo"]):
        if ra >= 0: want_p[ra].append((k, 0))
        if rb >= 0: want_p[rb].append((k, 1))
    for k, (_, _, ra, rb, *_r) in enumerate(exp["el"]):
        if ra >= 0: want_p[ra].append((k, 2))
        if rb >= 0: want_l[rb].append(k)
    for k, (_, _, ra, rb, *_r) in enumerate(exp["ell"]):
        if ra >= 0: want_ll[ra].append((k, 0))
        if rb >= 0: want_ll[rb].append((k, 1))
    for k, (_, _, ra, *_r) in enumerate(exp["ep"]):
        if ra >= 0: want_ep[ra].append(k)
    csr = lambda ptr, items, r: items[ptr[r]:ptr[r + 1]]
    prec = T["pslot_rec"].reshape(-1, 4)
    assert len(T["pslot_ptr"]) == n_pr + 1 and T["pslot_ptr"][-1] == len(prec)
    for r in range(n_pr):
        got = csr(T["pslot_ptr"], prec, r)
        assert [(int(e), int(kind)) for e, kind, _, _ in got] == want_p[r], r
        for e, kind, a, b in got:   # the record carries the edge's two ends
            cls = "eo" if kind < 2 else "el"
            assert (a, b) == (T[f"{cls}_a"][e], T[f"{cls}_b"][e])
    for r in range(n_lr):
        assert csr(T["lslot_ptr"], T["lslot_edge"], r).tolist() == want_l[r]
        assert [tuple(x) for x in csr(T["llslot_ptr"], T["llslot_rec"].reshape(-1, 2), r).tolist()] == want_ll[r]
    assert T["ep_row"].tolist() == [r for r in range(n_pr) if want_ep[r]]
    for n, r in enumerate(T["ep_row"]):
        assert csr(T["ep_ptr"], T["ep_edge"], n).tolist() == want_ep[r]

    # ---- blocks: numbered by first appearance, one owner each (the lowest edge on the pair), the others are exactly the duplicate lists
    def check_blocks(c, blocks, ordered, shift, dup):
        blocks = blocks.reshape(-1, 2)
        seen, owners, dups = {}, {}, []
        for k, (_, _, ra, rb, *_r) in enumerate(exp[c]):
            code = int(T[f"{c}_blk"][k])
            if ra < 0 or rb < 0 or (ordered and ra == rb):
                assert code == -1
                continue
            pair = (min(ra, rb), max(ra, rb)) if ordered else (ra, rb)
            idx = seen.setdefault(pair, len(seen))
            assert tuple(blocks[idx]) == pair
            want = idx * 2 + (1 if ra > rb else 0) if shift else idx
            if dup is None:                      # point-point edges sum into their block: no owner coding
                assert code == want
            elif idx in owners:
                assert code == -2 - want
                dups.append(k)
            else:
                owners[idx] = k
                assert code == want
        assert len(seen) == len(blocks)
        if dup is not None:
            assert sorted(dup.tolist()) == dups
            key = [(-2 - int(T[f"{c}_blk"][k])) >> shift for k in dup]
            assert key == sorted(key) and all(a < b for a, b, ka, kb in zip(dup, dup[1:], key, key[1:]) if ka == kb)   # stable by block
        return seen
    pp = check_blocks("eo", T["ppoff"], True, 1, T["dup_eo"])
    pl = check_blocks("el", T["plblk"], False, 0, T["dup_el"])
    ll = check_blocks("ell", T["llblk"], True, 0, None)
    assert len(T["dup_eo"]) >= 2 and len(T["dup_el"]) >= 1
    for idx in range(len(ll)):                   # the edges of a landmark-landmark block, in edge order
        assert csr(T["llblk_ptr"], T["llblk_edge"], idx).tolist() == [k for k in range(n_of["ell"]) if T["ell_blk"][k] == idx]
    assert any(len(csr(T["llblk_ptr"], T["llblk_edge"], idx)) == 2 for idx in range(len(ll)))

    # ---- prow_perm: each graph's range is a permutation of its rows, sorted (stably) by (EdgeSE3 slots, all slots)
    for s in S:
        rng_ = T["prow_perm"][s["prow0"]:s["prow0"] + s["nprow"]]
        assert sorted(rng_.tolist()) == list(range(s["prow0"], s["prow0"] + s["nprow"]))
        key = [(sum(1 for _, kind in want_p[r] if kind < 2), len(want_p[r]), r) for r in rng_]
        assert key == sorted(key)

    # ---- adjacency: every row strictly increasing in column offset, and the rows together hold every block from both sides
    n_adj = 0
    for r in range(n_pr + n_lr):
        x = csr(T["adj_ptr"], T["adj_x"], r)
        assert np.all(np.diff(x) > 0), r
        n_adj += len(x)
    assert n_adj == len(T["adj_blk"]) == len(T["adj_fmt"]) == 2 * (len(pp) + len(pl) + len(ll))
