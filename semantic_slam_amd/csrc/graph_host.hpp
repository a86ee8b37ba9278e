// Host-side graph container + batch compiler for the MI355X ps_graph_slam backend.
// Mirrors what g2o::SparseOptimizer holds for the reference's GraphSLAM
// (reference include/ps_graph_slam/graph_slam.hpp:147) as plain arrays.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace sslam {

enum { VT_SE3 = 0, VT_POINT = 1, VT_PLANE = 2 };
enum { ET_SE3 = 0, ET_SE3_POINT = 1, ET_SE3_PLANE = 2, ET_POINT_POINT = 3 };   // 3: g2o::EdgePointXYZ (graph_slam.cpp:168-180)
// unary position priors on a VertexSE3 (hdl_graph_slam's EdgeSE3PriorXY / EdgeSE3PriorXYZ; graph_slam.hpp:115-126, commented out in the
// reference): evj = -1, the measurement is the position (2 / 3 doubles), the information matrix 2 x 2 / 3 x 3
enum { ET_SE3_PRIOR_XY = 4, ET_SE3_PRIOR_XYZ = 5, kEdgeTypes = 6 };
// storage classes of the device batch: what an edge couples decides the kernel that reads it
enum { EC_SE3 = 0, EC_LANDMARK = 1, EC_POINT_POINT = 2, EC_PRIOR = 3, kEdgeClasses = 4 };

// What an edge type IS, in one place: the C-ABI checks, the g2o reader / writer, the batch compile and the traffic model all read this table.
// A new type that fits an existing storage class is a row here and an sslam_graph_add_edge_* wrapper.
struct EdgeType {
  const char* tag;   // g2o row: tag, vertex id(s), `extra_ints` zeros, nz doubles of z, upper triangle of the d x d information matrix
  int extra_ints;    // EDGE_SE3_TRACKXYZ carries a parameter id (always 0) behind its vertex ids
  int nz, d;         // doubles of the measurement, dimension of the error / information matrix
  int vt_i, vt_j;    // vertex type of each end; vt_j = -1: unary (evj = -1)
  int cls;           // storage class EC_*
  int lin_bytes;     // bytes one edge moves in a Jacobian build (sslam_batch_linearize_bytes)
};
constexpr EdgeType kEdgeType[kEdgeTypes] = {
  {"EDGE_SE3:QUAT", 0, 7, 6, VT_SE3, VT_SE3, EC_SE3, 344 + 288},
  {"EDGE_SE3_TRACKXYZ", 1, 3, 3, VT_SE3, VT_POINT, EC_LANDMARK, 160 + 144},
  {"EDGE_SE3_PLANE", 0, 4, 3, VT_SE3, VT_PLANE, EC_LANDMARK, 176 + 144},   // row format of the in-tree EdgeSE3Plane::write (edge_se3_plane.hpp:40-47)
  {"EDGE_POINTXYZ", 0, 3, 3, VT_POINT, VT_POINT, EC_POINT_POINT, 8 + 24 + 48 + 48 + 72},
  {"EDGE_SE3_PRIORXY", 0, 2, 2, VT_SE3, -1, EC_PRIOR, 80},                  // hdl_graph_slam's EdgeSE3PriorXY(Z)::write: vertex, z, upper triangle
  {"EDGE_SE3_PRIORXYZ", 0, 3, 3, VT_SE3, -1, EC_PRIOR, 80},                 // (80: z 24, Omega 48, dim 4, slot 4)
};
// columns of a storage class's SoA payload: the widest measurement / information matrix of its types (narrower ones are zero-padded)
constexpr int class_nz(int cls) { int n = 0; for (const EdgeType& t : kEdgeType) if (t.cls == cls && t.nz > n) n = t.nz; return n; }
constexpr int class_d(int cls) { int n = 0; for (const EdgeType& t : kEdgeType) if (t.cls == cls && t.d > n) n = t.d; return n; }
constexpr int upper_len(int d) { return d * (d + 1) / 2; }

// upper triangle (row by row) of the D x D matrix whose leading d x d block is the row-major W and whose other entries are zero -> u;
// element q of u goes to u[q * stride]
inline void pack_upper(const double* W, int d, double* u, int D, size_t stride = 1) {
  size_t q = 0;
  for (int r = 0; r < D; ++r) for (int c = r; c < D; ++c) u[(q++) * stride] = (r < d && c < d) ? W[r * d + c] : 0.0;
}
inline void pack_upper(const double* W, int d, double* u) { pack_upper(W, d, u, d); }
// ... and back: the symmetric d x d row-major W of an upper triangle
inline void unpack_upper(const double* u, int d, double* W) {
  int q = 0;
  for (int r = 0; r < d; ++r) for (int c = r; c < d; ++c) { W[r * d + c] = u[q]; W[c * d + r] = u[q]; ++q; }
}

// threads per workgroup of the edge-parallel / scalar-row kernels (the latter a multiple of 6 and 64): the batch compile sizes the grids
constexpr int kEdgeChunk = 256;
constexpr int kRowChunk = 192;

// one graph's ranges in the concatenated arrays of a batch
struct GraphSeg {
  int prow0, nprow;  // active pose rows  [prow0, prow0+nprow)
  int lrow0, nlrow;  // active landmark rows
  int eo0, neo;      // SE3 edges
  int el0, nel;      // landmark edges
  int pose0, npose;  // all SE3 vertices (incl. fixed)
  int lm0, nlm;      // all landmark vertices
  int ell0, nell;    // point-point edges (g2o::EdgePointXYZ)
  int ep0, nep;      // position priors (EdgeSE3PriorXY / EdgeSE3PriorXYZ)
};

struct Options {
  int solver = 1;            // 0 PCG, 1 sparse block Cholesky
  double pcg_tol = 1e-10;    // relative residual ||r|| / ||b||
  int pcg_max_iters = 20000;
  double dcs_phi = 0.0;      // > 0: g2o::RobustKernelDCS(delta = phi) on the landmark edges (quirk B1: off by default)
  int speculative = 1;       // 1 / 2: a single small graph runs the damping trials of an LM iteration side by side in one launch (1, the default since
                             // round 5: once a trial has been rejected and while the lanes fit the chip; 2: always); same results, bitwise; 0: off
  int fused = 1;             // small batches: factor + both solves + the halves of a damping trial in one dependency-driven launch (k_chol_flow); 0: the stand-alone kernels (same results, bitwise)
};

struct HostGraph {
  int device = 0;
  std::vector<int> vtype, vfixed;
  std::vector<double> est;  // 7 per vertex
  std::vector<int> etype, evi, evj;
  std::vector<double> meas;  // 7 per edge
  std::vector<double> info;  // 36 per edge (leading d*d used, row-major)
  // per-edge robust kernels (sslam_graph_set_edge_robust_kernel): kind 0..7 (SSLAM_ROBUST_*) and width delta per edge.  Edge DATA like meas /
  // info, not structure: a change bumps robust_version, which a batch compares at its next upload.
  std::vector<unsigned char> rk_kind;
  std::vector<double> rk_delta;
  int n_robust = 0;                // edges with kind != 0
  uint64_t robust_version = 0;
  Options opt;
  uint64_t structure_version = 0;  // bumped on every add_*
  int nv() const { return (int)vtype.size(); }
  int ne() const { return (int)etype.size(); }
};

inline int vertex_dim(int t) { return t == VT_SE3 ? 6 : 3; }
inline int vertex_est_len(int t) { return t == VT_SE3 ? 7 : (t == VT_POINT ? 3 : 4); }

// g2o initializeOptimization ordering: non-fixed vertices that own >= 1 edge get
// consecutive scalar offsets by id (a unary prior is an edge of its vertex).  Returns the total dimension.
inline int hessian_indices(const HostGraph& g, std::vector<int>& hidx) {
  const int nv = g.nv();
  std::vector<char> has(nv, 0);
  for (int k = 0; k < g.ne(); ++k) { has[g.evi[k]] = 1; if (g.evj[k] >= 0) has[g.evj[k]] = 1; }
  hidx.assign(nv, -1);
  int off = 0;
  for (int v = 0; v < nv; ++v)
    if (!g.vfixed[v] && has[v]) { hidx[v] = off; off += vertex_dim(g.vtype[v]); }
  return off;
}

}  // namespace sslam
