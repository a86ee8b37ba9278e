"""Host-side mirror of ``ps_graph_slam::GraphSLAM`` over the C-ABI (include/sslam.h).

Method names, argument meaning and return conventions follow the reference class
(reference include/ps_graph_slam/graph_slam.hpp:35-152, src/ps_graph_slam/graph_slam.cpp):
``add_se3_node``, ``add_point_xyz_node``, ``add_se3_edge``, ``add_se3_point_xyz_edge``,
``add_se3_prior_xy_edge`` / ``add_se3_prior_xyz_edge`` (declared in comments upstream),
``optimize`` (returns ``False`` iff the graph has fewer than 10 edges, graph_slam.cpp:184-186),
``computeLandmarkMarginals``, ``save``.  Vertex handles are plain integer ids.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from ._lib import load_library, OptStats

ERR_TOO_FEW_EDGES = -5


class SslamError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"sslam error {code}: {msg}")
        self.code = code


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _check(lib, rc: int) -> int:
    if rc < 0:
        raise SslamError(rc, lib.sslam_last_error().decode())
    return rc


def _pose7(pose) -> np.ndarray:
    """Accept [t(3), q(x,y,z,w)] or a 4x4 / 3x4 isometry (Eigen::Isometry3d in the reference)."""
    a = np.asarray(pose, np.float64)
    if a.shape == (7,):
        return np.ascontiguousarray(a)
    if a.shape in ((4, 4), (3, 4)):
        from .synth import quat_from_matrix
        return np.ascontiguousarray(np.concatenate([a[:3, 3], quat_from_matrix(a[:3, :3])]))
    raise ValueError("pose must be 7 numbers [t, q(xyzw)] or a 4x4 isometry")


# g2o's RobustKernelFactory names -> SSLAM_ROBUST_* (include/sslam.h; GemanMcClure and Tukey are left out there on purpose)
ROBUST_KERNELS = {"NONE": 0, "Huber": 1, "PseudoHuber": 2, "Cauchy": 3, "Welsch": 4, "Fair": 5, "Saturated": 6, "DCS": 7}


# candidate kinds of the loop-closure gate -> SSLAM_GATE_*
GATE_KINDS = {"se3": 0, "point": 1}


class GraphSLAM:
    """``ps_graph_slam::GraphSLAM`` on one MI355X (graph_slam.cpp:40-97)."""

    def __init__(self, verbose: bool = False, device: int = 0):
        self._lib = load_library()
        self.verbose_ = verbose
        self._h = self._lib.sslam_graph_create(device)
        self.last_stats: OptStats | None = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.sslam_graph_destroy(h)

    # -- vertices ----------------------------------------------------------------------------
    def add_se3_node(self, pose, fixed: int = -1) -> int:
        """graph_slam.cpp:104-115; the first vertex of the graph is fixed (``fixed=-1``)."""
        return _check(self._lib, self._lib.sslam_graph_add_vertex_se3(self._h, _dptr(_pose7(pose)), fixed))

    def add_point_xyz_node(self, xyz) -> int:
        """graph_slam.cpp:127-134"""
        a = np.ascontiguousarray(xyz, np.float64).reshape(3)
        return _check(self._lib, self._lib.sslam_graph_add_vertex_point(self._h, _dptr(a)))

    def add_plane_node(self, plane_coeffs) -> int:
        """graph_slam.cpp:117-125 (commented out upstream; g2o::VertexPlane)"""
        a = np.ascontiguousarray(plane_coeffs, np.float64).reshape(4)
        return _check(self._lib, self._lib.sslam_graph_add_vertex_plane(self._h, _dptr(a)))

    # -- edges -------------------------------------------------------------------------------
    def add_se3_edge(self, v1: int, v2: int, relative_pose, information_matrix) -> int:
        """graph_slam.cpp:136-148 (information must be 6x6)"""
        w = np.ascontiguousarray(information_matrix, np.float64).reshape(36)
        return _check(self._lib, self._lib.sslam_graph_add_edge_se3(self._h, v1, v2, _dptr(_pose7(relative_pose)), _dptr(w)))

    def add_se3_point_xyz_edge(self, v_se3: int, v_xyz: int, xyz, information_matrix) -> int:
        """graph_slam.cpp:150-166 (information must be 3x3)"""
        z = np.ascontiguousarray(xyz, np.float64).reshape(3)
        w = np.ascontiguousarray(information_matrix, np.float64).reshape(9)
        return _check(self._lib, self._lib.sslam_graph_add_edge_se3_point(self._h, v_se3, v_xyz, _dptr(z), _dptr(w)))

    def add_se3_plane_edge(self, v_se3: int, v_plane: int, plane_coeffs, information_matrix) -> int:
        """graph_slam.hpp:73-75 (commented out upstream) -> include/g2o/edge_se3_plane.hpp"""
        z = np.ascontiguousarray(plane_coeffs, np.float64).reshape(4)
        w = np.ascontiguousarray(information_matrix, np.float64).reshape(9)
        return _check(self._lib, self._lib.sslam_graph_add_edge_se3_plane(self._h, v_se3, v_plane, _dptr(z), _dptr(w)))

    def add_point_xyz_point_xyz_edge(self, v1_xyz: int, v2_xyz: int, xyz, information_matrix) -> int:
        """graph_slam.cpp:168-180: g2o::EdgePointXYZ between two point landmarks, measurement = p2 - p1"""
        z = np.ascontiguousarray(xyz, np.float64).reshape(3)
        w = np.ascontiguousarray(information_matrix, np.float64).reshape(9)
        return _check(self._lib, self._lib.sslam_graph_add_edge_point_point(self._h, v1_xyz, v2_xyz, _dptr(z), _dptr(w)))

    def add_se3_prior_xy_edge(self, v_se3: int, xy, information_matrix) -> int:
        """graph_slam.hpp:122-123 (commented out upstream): hdl_graph_slam's EdgeSE3PriorXY, e = t.xy - xy (information must be 2x2)"""
        z = np.ascontiguousarray(xy, np.float64).reshape(2)
        w = np.ascontiguousarray(information_matrix, np.float64).reshape(4)
        return _check(self._lib, self._lib.sslam_graph_add_edge_se3_prior_xy(self._h, v_se3, _dptr(z), _dptr(w)))

    def add_se3_prior_xyz_edge(self, v_se3: int, xyz, information_matrix) -> int:
        """graph_slam.hpp:125-126 (commented out upstream): hdl_graph_slam's EdgeSE3PriorXYZ, e = t - xyz (information must be 3x3)"""
        z = np.ascontiguousarray(xyz, np.float64).reshape(3)
        w = np.ascontiguousarray(information_matrix, np.float64).reshape(9)
        return _check(self._lib, self._lib.sslam_graph_add_edge_se3_prior_xyz(self._h, v_se3, _dptr(z), _dptr(w)))

    # -- queries -----------------------------------------------------------------------------
    # ---- per-edge robust kernels (hdl_graph_slam's GraphSLAM::add_robust_kernel)
    def add_robust_kernel(self, edge_id: int, kernel_type: str, kernel_size: float = 1.0) -> None:
        """Put the g2o kernel `kernel_type` ("NONE", "Huber", "PseudoHuber", "Cauchy", "Welsch", "Fair", "Saturated", "DCS") of width
        `kernel_size` on an edge of any class; "NONE" removes it.  A value change: the symbolic factorisation is kept."""
        if kernel_type not in ROBUST_KERNELS:
            raise ValueError(f"unknown robust kernel type '{kernel_type}' (known: {', '.join(ROBUST_KERNELS)})")
        _check(self._lib, self._lib.sslam_graph_set_edge_robust_kernel(self._h, int(edge_id), ROBUST_KERNELS[kernel_type], float(kernel_size)))

    def edge_robust_kernel(self, edge_id: int):
        """(type name, size) of the edge's own kernel; ("NONE", 0.0) without one."""
        kind, delta = C.c_int(0), C.c_double(0.0)
        _check(self._lib, self._lib.sslam_graph_get_edge_robust_kernel(self._h, int(edge_id), C.byref(kind), C.byref(delta)))
        return [k for k, v in ROBUST_KERNELS.items() if v == kind.value][0], delta.value

    def edge_chi2(self, edge_ids=None):
        """Per edge at the current estimates: (e2, rho0, weight) arrays -- the raw e^T Omega e, the robustified chi2 term and the kernel's
        rho1.  edge_ids None: all edges in id order."""
        if edge_ids is None:
            n, ids = self.num_edges(), None
        else:
            ids = np.ascontiguousarray(edge_ids, np.int32)
            n = int(ids.size)
        e2, r0, w = np.zeros(n), np.zeros(n), np.zeros(n)
        if n:
            _check(self._lib, self._lib.sslam_graph_edge_chi2(self._h, ids.ctypes.data_as(C.POINTER(C.c_int)) if ids is not None else None,
                                                              n, _dptr(e2), _dptr(r0), _dptr(w)))
        return e2, r0, w

    def num_vertices(self) -> int:
        return self._lib.sslam_graph_num_vertices(self._h)

    def num_edges(self) -> int:
        return self._lib.sslam_graph_num_edges(self._h)

    def estimate(self, vid: int) -> np.ndarray:
        out = np.zeros(7)
        n = _check(self._lib, self._lib.sslam_graph_get_vertex(self._h, vid, _dptr(out)))
        return out[:n].copy()

    def set_estimate(self, vid: int, est) -> None:
        a = np.zeros(7)
        e = np.asarray(est, np.float64).ravel()
        a[:len(e)] = e
        _check(self._lib, self._lib.sslam_graph_set_vertex(self._h, vid, _dptr(a)))

    def hessian_index(self, vid: int) -> int:
        return self._lib.sslam_graph_hessian_index(self._h, vid)

    def set_option(self, key: str, value: float) -> None:
        _check(self._lib, self._lib.sslam_graph_set_option(self._h, key.encode(), float(value)))

    def chi2(self) -> float:
        c = C.c_double(0)
        _check(self._lib, self._lib.sslam_graph_chi2(self._h, C.byref(c)))
        return c.value

    # -- the hot entry ------------------------------------------------------------------------
    def optimize(self, max_iterations: int = 1024) -> bool:
        """graph_slam.cpp:182-219. Returns False iff the graph has < 10 edges."""
        st = OptStats()
        rc = self._lib.sslam_graph_optimize(self._h, max_iterations, C.byref(st))
        self.last_stats = st
        if rc == ERR_TOO_FEW_EDGES:
            return False
        _check(self._lib, rc)
        if self.verbose_:
            print(f"iterations: {st.iterations}\nchi2: (before){st.chi2_before} -> (after){st.chi2_after}\n"
                  f"time: {st.seconds:.3f}[sec]")
        return True

    def computeLandmarkMarginals(self, vert_ids: Sequence[int]):
        """graph_slam.cpp:221-234: diagonal blocks of H^-1 for the listed vertices."""
        ids = np.ascontiguousarray(vert_ids, np.int32)
        dims = [7 - 1 if len(self.estimate(int(v))) == 7 else 3 for v in ids]
        out = np.zeros(int(sum(d * d for d in dims)))
        _check(self._lib, self._lib.sslam_graph_marginals(self._h, ids.ctypes.data_as(C.POINTER(C.c_int)), len(ids), _dptr(out)))
        blocks, o = [], 0
        for d in dims:
            blocks.append(out[o:o + d * d].reshape(d, d).copy())
            o += d * d
        return blocks

    def computeMarginals(self, vert_pairs_vec):
        """graph_slam.cpp:221-234 with the reference's own argument: (row, col) pairs of ``hessian_index`` values
        (semantic_graph_slam.cpp:186-191).  Returns {(row, col): block of H^-1}."""
        pairs = np.ascontiguousarray(vert_pairs_vec, np.int32).reshape(-1, 2)
        dim_of = {}
        for v in range(self.num_vertices()):
            h = self.hessian_index(v)
            if h >= 0:
                dim_of[h] = 6 if len(self.estimate(v)) == 7 else 3
        dims = [(dim_of[int(r)], dim_of[int(c)]) for r, c in pairs]
        out = np.zeros(int(sum(a * b for a, b in dims)))
        _check(self._lib, self._lib.sslam_graph_marginals_by_hessian_index(self._h, pairs.ctypes.data_as(C.POINTER(C.c_int)), len(pairs), _dptr(out)))
        res, o = {}, 0
        for (r, c), (a, b) in zip(pairs, dims):
            res[(int(r), int(c))] = out[o:o + a * b].reshape(a, b).copy()
            o += a * b
        return res

    # -- loop-closure gate -------------------------------------------------------------------
    def _gate(self, kind: int, v_from: int, v_to: int, z7: np.ndarray, information, d: int) -> float:
        cand = np.array([kind, int(v_from), int(v_to)], np.int32)
        w = None
        if information is not None:
            w = np.zeros(36)
            w[:d * d] = np.ascontiguousarray(information, np.float64).reshape(d * d)
        d2 = np.zeros(1)
        _check(self._lib, self._lib.sslam_graph_gate(self._h, cand.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(z7),
                                                     _dptr(w) if w is not None else None, 1, _dptr(d2), None, None))
        return float(d2[0])

    def gate_se3(self, v1: int, v2: int, relative_pose, information=None) -> float:
        """sslam_graph_gate: squared Mahalanobis distance of a candidate EdgeSE3 (arguments of add_se3_edge) that is not in the graph, in
        S = J Sigma J^T + information^-1 at the current estimates; information None: in J Sigma J^T alone.  NaN when S is singular."""
        return self._gate(GATE_KINDS["se3"], v1, v2, _pose7(relative_pose), information, 6)

    def gate_point(self, v_se3: int, v_xyz: int, xyz, information=None) -> float:
        """the same for a candidate EdgeSE3PointXYZ (arguments of add_se3_point_xyz_edge)"""
        z = np.zeros(7)
        z[:3] = np.ascontiguousarray(xyz, np.float64).reshape(3)
        return self._gate(GATE_KINDS["point"], v_se3, v_xyz, z, information, 3)

    def save(self, filename: str) -> None:
        """graph_slam.cpp:236-239 (g2o text format)"""
        _check(self._lib, self._lib.sslam_graph_save_g2o(self._h, filename.encode()))

    def load(self, filename: str) -> None:
        _check(self._lib, self._lib.sslam_graph_load_g2o(self._h, filename.encode()))

    # -- parity / measurement hooks -------------------------------------------------------------
    def linearize(self):
        """Normal equations at the current estimates: (H upper-triangular scipy CSC, b), g2o order."""
        import scipy.sparse as sp
        dim = C.c_int(0)
        nnz = C.c_int64(0)
        _check(self._lib, self._lib.sslam_graph_linearize(self._h, C.byref(dim), C.byref(nnz), None, None, None, None))
        rows = np.zeros(nnz.value, np.int32); cols = np.zeros(nnz.value, np.int32)
        vals = np.zeros(nnz.value); b = np.zeros(dim.value)
        _check(self._lib, self._lib.sslam_graph_linearize(self._h, C.byref(dim), C.byref(nnz), rows.ctypes.data, cols.ctypes.data,
                                                          vals.ctypes.data, b.ctypes.data))
        U = sp.coo_matrix((vals, (rows, cols)), shape=(dim.value, dim.value)).tocsc()
        return U, b

    def solve(self, lam: float):
        dim = C.c_int(0); nnz = C.c_int64(0)
        _check(self._lib, self._lib.sslam_graph_linearize(self._h, C.byref(dim), C.byref(nnz), None, None, None, None))
        x = np.zeros(dim.value)
        its = C.c_int64(0)
        _check(self._lib, self._lib.sslam_graph_solve(self._h, float(lam), _dptr(x), C.byref(its)))
        return x, its.value

    def oplus(self, dx) -> None:
        a = np.ascontiguousarray(dx, np.float64)
        _check(self._lib, self._lib.sslam_graph_oplus(self._h, _dptr(a)))

    # -- bulk construction helpers ----------------------------------------------------------------
    @classmethod
    def from_problem(cls, gp, device: int = 0) -> "GraphSLAM":
        """Build through the per-vertex/per-edge C-ABI from flat arrays (oracle.GraphProblem layout)."""
        G = cls(False, device)
        for v in range(gp.nv):
            t = int(gp.vtype[v])
            if t == 0:
                vid = G.add_se3_node(gp.est[v], fixed=int(gp.vfixed[v]))
            elif t == 1:
                vid = G.add_point_xyz_node(gp.est[v, :3])
            else:
                vid = G.add_plane_node(gp.est[v, :4])
            assert vid == v
        for k in range(gp.ne):
            t = int(gp.etype[k])
            i, j = int(gp.evi[k]), int(gp.evj[k])
            if t == 0:
                G.add_se3_edge(i, j, gp.meas[k], gp.info[k].reshape(6, 6))
            elif t == 1:
                G.add_se3_point_xyz_edge(i, j, gp.meas[k, :3], gp.info[k, :9].reshape(3, 3))
            elif t == 3:
                G.add_point_xyz_point_xyz_edge(i, j, gp.meas[k, :3], gp.info[k, :9].reshape(3, 3))
            else:
                G.add_se3_plane_edge(i, j, gp.meas[k, :4], gp.info[k, :9].reshape(3, 3))
        return G

    @classmethod
    def from_synth(cls, g, device: int = 0) -> "GraphSLAM":
        """Build a graph from a synth.SynthGraph: poses 0..Np-1 (the first fixed, graph_slam.cpp:109-111), then landmarks."""
        G = cls(False, device)
        lib, h, Np = G._lib, G._h, g.n_poses
        plane = g.landmark_kind == "plane"
        nl = 4 if plane else 3

        def rows(a, width):   # pointers to the rows of a C-contiguous float64 copy (kept alive by the caller's name)
            a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(len(a), width))
            base, step = a.ctypes.data, a.strides[0]
            return a, [C.cast(base + k * step, C.POINTER(C.c_double)) for k in range(len(a))]
        # the add_* calls above without their per-call conversions (thousands per graph): the same values in the same order
        pa, pp = rows(g.poses_init, 7)
        for p in pp:
            _check(lib, lib.sslam_graph_add_vertex_se3(h, p, -1))
        la, lp = rows(g.lms_init, nl)
        add_lm = lib.sslam_graph_add_vertex_plane if plane else lib.sslam_graph_add_vertex_point
        for p in lp:
            _check(lib, add_lm(h, p))
        za, zp = rows(g.odom_z, 7)
        wa, wp = rows(g.odom_info, 36)
        for (i, j), z, w in zip(g.odom_ij.tolist(), zp, wp):
            _check(lib, lib.sslam_graph_add_edge_se3(h, i, j, z, w))
        ya, yp = rows(g.lm_z, nl)
        va, vp = rows(g.lm_info, 9)
        add_e = lib.sslam_graph_add_edge_se3_plane if plane else lib.sslam_graph_add_edge_se3_point
        for (i, l), z, w in zip(g.lm_ij.tolist(), yp, vp):
            _check(lib, add_e(h, i, Np + l, z, w))
        return G

    def estimates(self) -> np.ndarray:
        n = self.num_vertices()
        out = np.zeros((n, 7))
        for v in range(n):
            e = self.estimate(v)
            out[v, :len(e)] = e
        return out


class GraphBatch:
    """Device-resident batch of independent graphs optimised together (MI355X extension)."""

    def __init__(self, graphs: Sequence[GraphSLAM], streams: int = 0):
        """streams > 1: a stream group (sslam_batch_create_streams) -- the graphs split into that many parts, each on its own HIP stream
        and host thread; 0: sslam_batch_create (one stream unless SSLAM_BATCH_STREAMS says otherwise)"""
        self._lib = load_library()
        self.graphs = list(graphs)
        arr = (C.c_void_p * len(self.graphs))(*[g._h for g in self.graphs])
        if streams > 0:
            self._h = self._lib.sslam_batch_create_streams(arr, len(self.graphs), int(streams))
        else:
            self._h = self._lib.sslam_batch_create(arr, len(self.graphs))
        if not self._h:
            raise SslamError(-1, self._lib.sslam_last_error().decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.sslam_batch_destroy(h)

    def upload(self):
        _check(self._lib, self._lib.sslam_batch_upload(self._h))

    def download(self):
        _check(self._lib, self._lib.sslam_batch_download(self._h))

    def optimize(self, max_iterations: int):
        st = (OptStats * len(self.graphs))()
        _check(self._lib, self._lib.sslam_batch_optimize(self._h, max_iterations, st))
        return list(st)

    # -- covariances -----------------------------------------------------------------------------
    def _request_array(self, requests) -> np.ndarray:
        """(graph, row vertex, column vertex) triples -> [n, 3] int32, checked against the host graphs before any C call"""
        rows = []
        for k, rq in enumerate(requests):
            try:
                g, vr, vc = rq
            except (TypeError, ValueError):
                raise ValueError(f"request {k}: expected (graph, row_vertex, col_vertex), got {rq!r}") from None
            for x in (g, vr, vc):
                if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                    raise TypeError(f"request {k}: graph index and vertex ids are integers, got {rq!r}")
            if not 0 <= g < len(self.graphs):
                raise IndexError(f"request {k}: graph index {g} out of range (the batch holds {len(self.graphs)} graphs)")
            rows.append((int(g), int(vr), int(vc)))
        return np.ascontiguousarray(rows, np.int32).reshape(-1, 3)

    def marginals(self, requests):
        """sslam_batch_marginals: blocks of H^-1 at the estimates the batch holds on the device.  ``requests`` is a sequence of
        (graph, row_vertex, col_vertex); returns the d(row) x d(col) arrays in request order."""
        req = self._request_array(requests)
        dims = []
        for k, (g, vr, vc) in enumerate(req):
            G = self.graphs[g]
            nv = G.num_vertices()
            if not (0 <= vr < nv and 0 <= vc < nv):
                raise IndexError(f"request {k}: vertex ids ({vr}, {vc}) out of range (graph {g} has {nv} vertices)")
            dims.append(tuple(6 if len(G.estimate(int(v))) == 7 else 3 for v in (vr, vc)))
        out = np.zeros(int(sum(a * b for a, b in dims)) + 1)
        _check(self._lib, self._lib.sslam_batch_marginals(self._h, req.ctypes.data_as(C.POINTER(C.c_int32)), len(req), _dptr(out)))
        blocks, o = [], 0
        for a, b in dims:
            blocks.append(out[o:o + a * b].reshape(a, b).copy())
            o += a * b
        return blocks

    # -- loop-closure gate -----------------------------------------------------------------------
    def _candidate_arrays(self, candidates):
        """(graph, "se3" | "point", v_from, v_to, z, info or None) tuples -> cand [n, 4] int32, z [n, 7], info (36 or None per candidate) and the
        dimensions, checked before any C call"""
        cand, zs, ws, dims = [], [], [], []
        for k, c in enumerate(candidates):
            try:
                g, kind, vu, vv, z, info = c
            except (TypeError, ValueError):
                raise ValueError(f"candidate {k}: expected (graph, kind, v_from, v_to, z, info), got {c!r}") from None
            for x in (g, vu, vv):
                if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                    raise TypeError(f"candidate {k}: graph index and vertex ids are integers, got {(g, vu, vv)!r}")
            if not 0 <= g < len(self.graphs):
                raise IndexError(f"candidate {k}: graph index {g} out of range (the batch holds {len(self.graphs)} graphs)")
            if not isinstance(kind, str) or kind not in GATE_KINDS:
                raise ValueError(f"candidate {k}: unknown kind {kind!r} (known: {', '.join(GATE_KINDS)})")
            d, nz = (6, 7) if kind == "se3" else (3, 3)
            z = np.asarray(z, np.float64)
            if z.shape != (nz,):
                raise ValueError(f"candidate {k}: the measurement of a '{kind}' candidate has {nz} numbers, got shape {z.shape}")
            z7 = np.zeros(7)
            z7[:nz] = z
            w = None
            if info is not None:
                info = np.asarray(info, np.float64)
                if info.shape != (d, d):
                    raise ValueError(f"candidate {k}: the information matrix of a '{kind}' candidate is {d}x{d}, got shape {info.shape}")
                w = np.zeros(36)
                w[:d * d] = info.reshape(-1)
            cand.append((int(g), GATE_KINDS[kind], int(vu), int(vv)))
            zs.append(z7)
            ws.append(w)
            dims.append(d)
        return np.array(cand, np.int32).reshape(-1, 4), np.array(zs, np.float64).reshape(-1, 7), ws, dims

    def gate(self, candidates, return_cov: bool = False):
        """sslam_batch_gate: squared Mahalanobis distances of candidate edges that are not in their graphs, at the estimates the batch
        holds on the device.  A candidate is (graph, "se3" | "point", v_from, v_to, z, info or None) with z = [t, q(xyzw)] / xyz and info
        6x6 / 3x3 (None: the distance in J Sigma J^T alone; the candidates with and those without an information matrix go in a C call
        each).  Returns d2 (float64, NaN where S is singular); with ``return_cov`` also the lists of the errors e and of the d x d matrices S."""
        cand, z, ws, dims = self._candidate_arrays(candidates)
        n = len(cand)
        d2, e, S = np.zeros(n), np.zeros((n, 6)), np.zeros((n, 36))
        for with_info in (True, False):
            idx = [k for k in range(n) if (ws[k] is not None) == with_info]
            if not idx:
                continue
            c, zz = np.ascontiguousarray(cand[idx]), np.ascontiguousarray(z[idx])
            w = np.ascontiguousarray([ws[k] for k in idx], np.float64) if with_info else None
            m = len(idx)
            pd2, pe, pS = np.zeros(m), np.zeros((m, 6)), np.zeros((m, 36))
            _check(self._lib, self._lib.sslam_batch_gate(self._h, c.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(zz),
                                                         _dptr(w) if with_info else None, m, _dptr(pd2),
                                                         _dptr(pe) if return_cov else None, _dptr(pS) if return_cov else None))
            d2[idx], e[idx], S[idx] = pd2, pe, pS
        if not return_cov:
            return d2
        return d2, [e[k, :d].copy() for k, d in enumerate(dims)], [S[k, :d * d].reshape(d, d).copy() for k, d in enumerate(dims)]

    def landmark_marginals(self, ids_per_graph):
        """diagonal blocks of H^-1 for the listed vertices of every graph: ``ids_per_graph[g]`` -> list of blocks, one list per graph"""
        ids_per_graph = [list(ids) for ids in ids_per_graph]
        if len(ids_per_graph) != len(self.graphs):
            raise ValueError(f"one id list per graph: got {len(ids_per_graph)} lists for {len(self.graphs)} graphs")
        blocks = iter(self.marginals([(g, v, v) for g, ids in enumerate(ids_per_graph) for v in ids]))
        return [[next(blocks) for _ in ids] for ids in ids_per_graph]

    # -- one linear solve per graph (parity hook) -------------------------------------------------
    def solve(self, lambdas):
        """sslam_batch_solve: (H_g + lambdas[g] I) x_g = b_g for every graph at the estimates the batch holds on the device.  A graph with
        lambdas[g] < 0 sits out as a terminated graph does in the LM endgame.  Returns one array per graph in hessian-index order, None for
        a graph that sat out; ``last_solver_iterations`` holds the PCG iterations per graph (0 for the direct solvers)."""
        lam = np.ascontiguousarray(lambdas, np.float64).reshape(-1)
        if len(lam) != len(self.graphs):
            raise ValueError(f"one lambda per graph: got {len(lam)} for {len(self.graphs)} graphs")
        n = int(self._lib.sslam_batch_solve(self._h, None, None, 0, None))
        _check(self._lib, min(n, 0))
        x = np.zeros(n + 1)
        it = (C.c_int64 * len(lam))()
        _check(self._lib, min(int(self._lib.sslam_batch_solve(self._h, _dptr(lam), _dptr(x), n, it)), 0))
        self.last_solver_iterations = list(it)
        if not hasattr(self, "_dims"):   # scalar unknowns per graph (the structure of a batch's graphs is fixed at its creation)
            self._dims = []
            for G in self.graphs:
                hv = [(G.hessian_index(v), v) for v in range(G.num_vertices())]
                h, v = max(hv) if hv else (-1, -1)
                self._dims.append(0 if h < 0 else h + (6 if len(G.estimate(v)) == 7 else 3))
        out, o = [], 0
        for g, d in enumerate(self._dims):
            out.append(x[o:o + d].copy() if lam[g] >= 0 else None)
            o += d
        assert o == n, (o, n)
        return out

    # -- edge-sharded mode (SURVEY 8e mode E) ----------------------------------------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """RCCL communicator + edge shard of this rank (every rank holds the whole batch); see distributed.init_edge_sharded."""
        _check(self._lib, self._lib.sslam_batch_comm_init(self._h, unique_id, rank, world))

    def set_edge_shard(self, rank: int, world: int) -> None:
        """install the edge shard WITHOUT a communicator: linearize_hb() then returns this rank's partial system (parity hook)"""
        _check(self._lib, self._lib.sslam_batch_set_edge_shard(self._h, rank, world))

    def linearize_hb(self) -> np.ndarray:
        """[H values || b] of the batch at the current estimates (partial if an edge shard is installed)"""
        n = int(self._lib.sslam_batch_linearize_hb(self._h, None, 0))
        _check(self._lib, min(n, 0))
        out = np.zeros(n)
        _check(self._lib, int(self._lib.sslam_batch_linearize_hb(self._h, _dptr(out), int(n))))
        return out

    def time_linearize(self, repeats: int = 20) -> float:
        ms = C.c_double(0)
        _check(self._lib, self._lib.sslam_batch_time_linearize(self._h, repeats, C.byref(ms)))
        return ms.value

    def time_solver(self, repeats: int = 5):
        """(factor ms, backward-solve ms) of one full-batch factorisation + solve, hipEvents on the batch's stream"""
        f = C.c_double(0); s = C.c_double(0)
        _check(self._lib, self._lib.sslam_batch_time_solver(self._h, repeats, C.byref(f), C.byref(s)))
        return f.value, s.value

    def linearize_bytes(self) -> int:
        return int(self._lib.sslam_batch_linearize_bytes(self._h))

    def info(self, key: str) -> float:
        v = C.c_double(0)
        _check(self._lib, self._lib.sslam_batch_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def set_profiling(self, on: bool):
        _check(self._lib, self._lib.sslam_batch_set_profiling(self._h, 1 if on else 0))

    def kernel_time(self, name: str):
        ms = C.c_double(0); n = C.c_int64(0)
        _check(self._lib, self._lib.sslam_batch_kernel_time(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value
