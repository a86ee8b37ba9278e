// HIP kernels of the ps_graph_slam backend for gfx950 (wave64, FP64).
//
// Layout (one device-resident *batch* of B independent graphs, all arrays concatenated by graph):
//   pose[NP][8]   t(3) q(4) pad            lm[NL][4]   point xyz,pad | plane n,d
//   unknown vector x:  [ pose rows: 6 each | landmark rows: 3 each ]   (global over the batch)
//   H values:   Hpp_diag[nPr][36] | Hll_diag[nLr][9] | Hpp_off[nPP][36] | Hpl[nPL][18]   (row-major)
//   edges: structure-of-arrays, SE3 edges and landmark edges separately, grouped by graph
// Reference semantics restated: g2o BlockSolver::buildSystem / computeActiveErrors /
// OptimizationAlgorithmLevenberg behind ps_graph_slam::GraphSLAM::optimize
// (reference src/ps_graph_slam/graph_slam.cpp:182-219).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "graph_host.hpp"   // GraphSeg, kEdgeChunk, kRowChunk
#include "sslam_math.hpp"

namespace sslam {

struct LmState {
  double lambda, nu, cur_chi, tmp_chi, rho, scale, chi_before, max_diag;
  long long pcg_iters;
  int q, iter, status, in_trial, active, accept, trials, solve_failed;
  int lin, pad0;   // lin: the graph starts a new LM iteration at the next step (its system is rebuilt)
};

// Device view of a batch (plain pointers; passed by value to kernels).
struct BatchView {
  int B, nPr, nLr, nPose, nLm, nEo, nEl, maxRowChunks, maxEdgeChunks;
  const GraphSeg* seg;
  LmState* lm;
  // estimates
  double* pose;        // current
  double* lmk;         // current
  double* pose_trial;
  double* lmk_trial;
  const int* pose_row; // [nPose] -> pose row or -1
  const int* lm_row;   // [nLm]   -> landmark row or -1
  const int* prow_pose;  // [nPr] -> pose index
  const int* lrow_lm;    // [nLr] -> landmark index
  const int* prow_graph; // [nPr]
  const int* prow_perm;  // [nPr] thread -> pose row of k_linearize_rowthread: the rows of a graph ordered by their slot counts (EdgeSE3 slots, then
                         //       landmark slots), so that the lanes of a wave walk slot lists of the same shape (round 6)
  const int* lrow_graph; // [nLr]
  const unsigned char* lm_kind;  // [nLm] VT_POINT / VT_PLANE
  // edges
  const int* eo_i; const int* eo_j; const double* eo_z; const double* eo_w; const int* eo_blk;  // eo_blk: off block idx*2 + swap, or -1
  const int* el_p; const int* el_l; const double* el_z; const double* el_w; const int* el_blk;
  // point-point edges (g2o::EdgePointXYZ, reference graph_slam.cpp:168-180): e = (p_b - p_a) - z, Jacobians -I / +I
  int nEll, nLL;                       // edges; unique landmark-landmark blocks
  const int* ell_a; const int* ell_b;  // landmark indices
  const double* ell_z; const double* ell_w;   // SoA: z[3][nEll], upper triangle of Omega [6][nEll]
  const int* ell_id;                   // graph-local edge id (edge-sharded mode)
  const int* llslot_ptr; const int2* llslot_rec;   // per landmark row: {edge, side (0: first vertex, 1: second)}
  const int* llblk_ptr; const int* llblk_edge;     // per landmark-landmark block: its edges
  double* Hll_off;                     // [nLL][9], block (row a < row b) = sum over its edges of -Omega
  // H
  double* Hpp_diag; double* Hll_diag; double* Hpp_off; double* Hpl; double* bvec;
  // plane landmarks (round 6): error and central-difference Jacobians of every EdgeSE3Plane, evaluated ONCE per linearisation by
  // k_plane_jacobians (a thread per (edge, perturbation)) -- [nEl][30] = {e 3 | J_l 3x3 | J_i 3x6}; nullptr when the batch has no plane
  double* pj;
  int64_t h_total;  // doubles in the H allocation
  // row adjacency for SpMV (rows = pose rows then landmark rows)
  const int* adj_ptr; const int* adj_blk; const int* adj_x; const unsigned char* adj_fmt;
  // gather-form Jacobian build: (row, incident edge) slots
  const int* pslot_ptr;                             // [nPr+1]
  const int4* pslot_rec;                            // [slots] {edge, kind, pose i | pose, pose j | landmark}; kind 0: SE3 edge, self = i; 1: SE3, self = j; 2: landmark edge
  const int* lslot_ptr; const int* lslot_edge;      // [nLr+1], landmark-side slots (edge index into el_*)
  int nDupEo, nDupEl; const int* dup_eo; const int* dup_el;  // non-owner edges of shared off-diagonal blocks
  // edge-sharded mode (one graph's edges split across ranks, SURVEY 8e mode E): a rank builds the partial normal equations of the
  // edges whose graph-local id lies in [shard_lo[g], shard_hi[g]); the partial [H || b] arrays are summed with one all-reduce
  const int* eo_id; const int* el_id;        // graph-local edge id of every SE3 / landmark edge
  const int* shard_lo; const int* shard_hi;  // [B]
  double dcs_phi = 0.0;                      // > 0: RobustKernelDCS on the landmark edges (chi2 uses rho[0], Omega is scaled by rho[1])
  // PCG vectors
  double* x; double* r; double* z; double* p; double* q; double* Minv;  // Minv: [nPr*36 | nLr*9]
  double* part_a; double* part_b; double* part_c;  // [B*maxChunks] partial sums
  double* rz;       // [2][B]
  double* bb;       // [B]
  int* pcg_done;    // [2][B] double-buffered by iteration parity
  int* pcg_fail;    // [B]
  int* flags;       // [0] any_in_trial, [1] all_pcg_done
  // position priors (hdl_graph_slam's EdgeSE3PriorXY / EdgeSE3PriorXYZ, unary on a VertexSE3): e = t(X) - z on the first ep_dim components,
  // J = [R | 0] -> only the pose's diagonal block and rhs.  SoA, grouped by graph in edge order: z[3][nEp], upper triangle of Omega [6][nEp]
  // (the third row / column zero for an XY prior)
  int nEp, nEpRows;
  const int* ep_pose; const int* ep_dim; const double* ep_z; const double* ep_w;
  const int* ep_id;                                  // graph-local edge id (edge-sharded mode)
  const int* ep_row; const int* ep_ptr; const int* ep_edge;   // [nEpRows] pose rows that carry priors, CSR over them: their priors in edge order
  // per-edge robust kernels (sslam_graph_set_edge_robust_kernel): kind (SSLAM_ROBUST_*, 0 = none) and width delta of every edge, next to each
  // class's Omega.  All eight pointers are nullptr when no edge of the batch has a kernel of its own; the host then launches the <RK = false>
  // instantiations, which are the kernels as they were before per-edge kernels existed.
  const unsigned char* eo_rk; const unsigned char* el_rk; const unsigned char* ell_rk; const unsigned char* ep_rk;
  const double* eo_rd; const double* el_rd; const double* ell_rd; const double* ep_rd;
};

// g2o::RobustKernelDCS::robustify: rho[1], the factor on Omega; rho[0] = rho[1] * e2
__device__ __forceinline__ double dcs_rho1(double phi, double e2) {
  const double scale = (2.0 * phi) / (phi + e2);
  return scale >= 1.0 ? 1.0 : scale * scale;
}
// Per-edge robust kernels, g2o semantics (BaseEdge::robustInformation): e2 = e^T Omega e -> rho0 (the edge's chi2 term) and rho1 (the factor
// on Omega in H and b).  The table of include/sslam.h; g2o's second-order term rho[2] stays out, as upstream.  Only the <RK = true>
// instantiations call this: FP64 sqrt / log / exp are multi-instruction sequences on CDNA and do not belong in the kernel-free build.
enum { RK_NONE = 0, RK_HUBER = 1, RK_PSEUDOHUBER = 2, RK_CAUCHY = 3, RK_WELSCH = 4, RK_FAIR = 5, RK_SATURATED = 6, RK_DCS = 7 };
__device__ __forceinline__ void robust_rho(int kind, double d, double e2, double& rho0, double& rho1) {
  const double d2 = d * d;
  rho0 = e2; rho1 = 1.0;
  switch (kind) {
    case RK_HUBER:
      if (e2 > d2) { const double s = sqrt(e2); rho0 = 2.0 * d * s - d2; rho1 = d / s; }
      break;
    case RK_PSEUDOHUBER: {
      const double a = sqrt(1.0 + e2 / d2);
      rho0 = 2.0 * d2 * (a - 1.0); rho1 = 1.0 / a;
    } break;
    case RK_CAUCHY: {
      const double a = 1.0 + e2 / d2;
      rho0 = d2 * log(a); rho1 = 1.0 / a;
    } break;
    case RK_WELSCH: {
      const double a = exp(-e2 / d2);
      rho0 = d2 * (1.0 - a); rho1 = a;
    } break;
    case RK_FAIR: {
      const double a = sqrt(e2) / d;
      rho0 = 2.0 * d2 * (a - log1p(a)); rho1 = 1.0 / (1.0 + a);
    } break;
    case RK_SATURATED:
      if (e2 > d2) { rho0 = d2; rho1 = 0.0; }
      break;
    case RK_DCS:
      rho1 = dcs_rho1(d, e2); rho0 = e2 * rho1;
      break;
    default: break;
  }
}
// e^T Omega e of EdgeSE3 k from the 21 upper-triangular entries of its Omega (SoA, stride n).  ONE form for every robust instantiation -- the
// two endpoint rows, a duplicate's off-diagonal block, the chi2 term, sslam_graph_edge_chi2 -- so that an edge at a Huber / Saturated
// threshold lands on the same side everywhere.
__device__ __forceinline__ double se3_e2(const double* __restrict__ w, int n, int k, const double ev[6]) {
  double e2 = 0;
  int q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) { e2 += (r == c ? 1.0 : 2.0) * w[(size_t)q * n + k] * (ev[r] * ev[c]); ++q; }
  return e2;
}
__device__ __forceinline__ double quad3(const double W[9], const double e[3]) {
  double c = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) c += e[r] * (W[r * 3 + 0] * e[0] + W[r * 3 + 1] * e[1] + W[r * 3 + 2] * e[2]);
  return c;
}
// The robust kernel an edge is under (kind 0: none; callers test it first, so an edge under none forms no e2).  rho0(e2) is the edge's chi2
// term and rho1(e2) the factor on its Omega in H and b, e2 = e^T Omega e of the UNMASKED Omega (se3_e2 / quad3): every rank of a sharded
// batch, both endpoint rows, a duplicate's block and the chi2 term see one value.  <RK = false>: only the DCS fallback exists, no sqrt / log / exp.
template <bool RK>
struct EdgeKernel {
  int kind;
  double delta;
  __device__ __forceinline__ void rho(double e2, double& rho0, double& rho1) const {
    if constexpr (RK) robust_rho(kind, delta, e2, rho0, rho1);
    else { rho1 = dcs_rho1(delta, e2); rho0 = e2 * rho1; }
  }
  __device__ __forceinline__ double rho0(double e2) const { double r0, r1; rho(e2, r0, r1); return r0; }
  __device__ __forceinline__ double rho1(double e2) const { double r0, r1; rho(e2, r0, r1); return r1; }
};
// The information-scaling rule, its ONE copy: edge k of a class (rk_of / rd_of: its kind and width arrays) is under its own kernel if it has one,
// else under DCS(dcs_phi) when dcs_phi > 0, else under none.  A pose-landmark edge passes V.dcs_phi; every other class passes 0.
template <bool RK>
__device__ __forceinline__ EdgeKernel<RK> info_scale(const unsigned char* __restrict__ rk_of, const double* __restrict__ rd_of, int k, double dcs_phi) {
  if constexpr (RK) {
    const int rk = rk_of[k];
    if (rk) return {rk, rd_of[k]};
  }
  return {dcs_phi > 0 ? RK_DCS : RK_NONE, dcs_phi};
}
// edge-sharded mode: this rank builds the edges of graph g whose id (id_of[k]) lies in [shard_lo[g], shard_hi[g]); the others count with Omega = 0
template <bool SHARD>
__device__ __forceinline__ bool in_shard(const BatchView& V, int g, const int* __restrict__ id_of, int k) {
  if constexpr (!SHARD) return true;
  else { const int id = id_of[k]; return V.shard_lo[g] <= id && id < V.shard_hi[g]; }
}

// ------------------------------------------------------------------------------------------
// deterministic workgroup reduction: wave shuffles, then a fixed-order sum of the wave partials
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* lds /* NT/64 doubles */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < NT / 64; ++k) s += lds[k];
  __syncthreads();
  return s;  // valid on thread 0
}
template <int NT>
__device__ __forceinline__ double block_max(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < NT / 64; ++k) s = fmax(s, lds[k]);
  __syncthreads();
  return s;
}
// fixed-order sum of n partials by one wave (all lanes get the result)
__device__ __forceinline__ double wave_sum_partials(const double* part, int n) {
  const int lane = threadIdx.x & 63;
  double s = 0;
  for (int k = lane; k < n; k += 64) s += part[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

__device__ __forceinline__ Pose load_pose(const double* a, int idx) {
  const double* p = a + (size_t)idx * 8;
  return Pose{{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}};
}
__device__ __forceinline__ void store_pose(double* a, int idx, const Pose& P) {
  double* p = a + (size_t)idx * 8;
  p[0] = P.t.x; p[1] = P.t.y; p[2] = P.t.z; p[3] = P.q.x; p[4] = P.q.y; p[5] = P.q.z; p[6] = P.q.w;
}
// symmetric 6x6 from 21 upper-triangular entries stored SoA with stride n: w[k*n + e]
__device__ __forceinline__ void load_sym6(const double* w, int n, int e, double W[36]) {
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) { const double v = w[(size_t)k * n + e]; W[r * 6 + c] = v; W[c * 6 + r] = v; ++k; }
}
__device__ __forceinline__ void load_sym3(const double* w, int n, int e, double W[9]) {
  int k = 0;
  for (int r = 0; r < 3; ++r)
    for (int c = r; c < 3; ++c) { const double v = w[(size_t)k * n + e]; W[r * 3 + c] = v; W[c * 3 + r] = v; ++k; }
}

// ---- edge errors: every edge class evaluates its error HERE, and takes its weight from info_scale above --------------------------------
// measurement of EdgeSE3 k (SoA z[7][n]: t, q)
__device__ __forceinline__ Pose load_meas_pose(const double* z, int n, int k) {
  return Pose{{z[0 * (size_t)n + k], z[1 * (size_t)n + k], z[2 * (size_t)n + k]},
              {z[3 * (size_t)n + k], z[4 * (size_t)n + k], z[5 * (size_t)n + k], z[6 * (size_t)n + k]}};
}
// the 4-double landmark record li of lmk (the current or the trial estimates): a point xyz, pad | a plane n, d
__device__ __forceinline__ Vec3 load_point(const double* lmk, int li) {
  const double* p = lmk + (size_t)li * 4;
  return Vec3{p[0], p[1], p[2]};
}
__device__ __forceinline__ Plane load_plane(const double* lmk, int li) {
  const double* p = lmk + (size_t)li * 4;
  return Plane{{p[0], p[1], p[2]}, p[3]};
}
// measurement of pose-landmark edge k (SoA el_z[4][nEl])
__device__ __forceinline__ Vec3 el_meas_point(const BatchView& V, int k) {
  const size_t n = (size_t)V.nEl;
  return Vec3{V.el_z[0 * n + k], V.el_z[1 * n + k], V.el_z[2 * n + k]};
}
__device__ __forceinline__ Plane el_meas_plane(const BatchView& V, int k) {
  const size_t n = (size_t)V.nEl;
  return Plane{{V.el_z[0 * n + k], V.el_z[1 * n + k], V.el_z[2 * n + k]}, V.el_z[3 * n + k]};
}
// error of pose-landmark edge k seen from pose Xi, a point or a plane by the kind of its landmark
__device__ __forceinline__ void lm_edge_error(const BatchView& V, int k, const Pose& Xi, const double* lmk, double err[3]) {
  const int li = V.el_l[k];
  if (V.lm_kind[li] == VT_POINT) {
    PointLin L;
    point_error(Xi, load_point(lmk, li), el_meas_point(V, k), L);
    err[0] = L.e[0]; err[1] = L.e[1]; err[2] = L.e[2];
  } else {
    plane_error(Xi, load_plane(lmk, li), el_meas_plane(V, k), err);
  }
}
// error of point-point edge k (g2o::EdgePointXYZ): e = (p_b - p_a) - z
__device__ __forceinline__ void ll_edge_error(const BatchView& V, const double* lmk, int k, double err[3]) {
  const size_t n = (size_t)V.nEll;
  const double* pa = lmk + (size_t)V.ell_a[k] * 4;
  const double* pb = lmk + (size_t)V.ell_b[k] * 4;
#pragma unroll
  for (int r = 0; r < 3; ++r) err[r] = (pb[r] - pa[r]) - V.ell_z[r * n + k];
}

// ---- scalar-row helpers -------------------------------------------------------------------------
struct RowRef {
  int valid;  // inside the graph's range
  int is_pose;
  int row;    // pose row or landmark row (global)
  int r;      // component inside the block
  int xoff;   // offset in the unknown vector
  int base;   // xoff of component 0
};
__device__ __forceinline__ RowRef row_ref(const BatchView& V, const GraphSeg& sg, int e) {
  RowRef R;
  const int npd = sg.nprow * 6;
  R.valid = e < npd + sg.nlrow * 3;
  if (e < npd) {
    R.is_pose = 1; R.row = sg.prow0 + e / 6; R.r = e % 6; R.base = 6 * R.row;
  } else {
    const int u = e - npd;
    R.is_pose = 0; R.row = sg.lrow0 + u / 3; R.r = u % 3; R.base = 6 * V.nPr + 3 * R.row;
  }
  R.xoff = R.base + R.r;
  return R;
}

__device__ __forceinline__ int row_chunks(const GraphSeg& sg) { return (sg.nprow * 6 + sg.nlrow * 3 + kRowChunk - 1) / kRowChunk; }
__device__ __forceinline__ int edge_count(const GraphSeg& sg) { return sg.neo + sg.nel + sg.nell + sg.nep; }
__device__ __forceinline__ int edge_chunks(const GraphSeg& sg) { return (edge_count(sg) + kEdgeChunk - 1) / kEdgeChunk; }


// x [+] dx of one block row t (pose rows first, then landmark rows) of a graph that is in a trial -> the trial estimates
// (VertexSE3 / VertexPointXYZ / VertexPlane::oplus)
__device__ __forceinline__ void oplus_row(const BatchView& V, int t, const double* __restrict__ dx) {
  if (t < V.nPr) {
    const int g = V.prow_graph[t];
    if (!V.lm[g].in_trial) return;
    const int pi = V.prow_pose[t];
    double d[6];
    for (int k = 0; k < 6; ++k) d[k] = dx[6 * (size_t)t + k];
    store_pose(V.pose_trial, pi, se3_oplus(load_pose(V.pose, pi), d));
  } else if (t < V.nPr + V.nLr) {
    const int l = t - V.nPr;
    const int g = V.lrow_graph[l];
    if (!V.lm[g].in_trial) return;
    const int li = V.lrow_lm[l];
    const double* d = dx + 6 * (size_t)V.nPr + 3 * (size_t)l;
    const double* c = V.lmk + (size_t)li * 4;
    double* o = V.lmk_trial + (size_t)li * 4;
    if (V.lm_kind[li] == VT_POINT) {
      o[0] = c[0] + d[0]; o[1] = c[1] + d[1]; o[2] = c[2] + d[2]; o[3] = 0;
    } else {
      const double dv[3] = {d[0], d[1], d[2]};
      const Plane P = pl_oplus(Plane{{c[0], c[1], c[2]}, c[3]}, dv);
      o[0] = P.n.x; o[1] = P.n.y; o[2] = P.n.z; o[3] = P.d;
    }
  }
}

// an accepted trial becomes the estimate: block row t of its graph
__device__ __forceinline__ void commit_row(const BatchView& V, int t) {
  if (t < V.nPr) {
    const int g = V.prow_graph[t];
    if (!V.lm[g].accept) return;
    const int pi = V.prow_pose[t];
    for (int k = 0; k < 7; ++k) V.pose[(size_t)pi * 8 + k] = V.pose_trial[(size_t)pi * 8 + k];
  } else if (t < V.nPr + V.nLr) {
    const int l = t - V.nPr;
    const int g = V.lrow_graph[l];
    if (!V.lm[g].accept) return;
    const int li = V.lrow_lm[l];
    for (int k = 0; k < 4; ++k) V.lmk[(size_t)li * 4 + k] = V.lmk_trial[(size_t)li * 4 + k];
  }
}

// g2o OptimizationAlgorithmLevenberg: accept / reject one damping trial of a graph; one thread
__device__ __forceinline__ void lm_control_apply(LmState& S, double tchi, double sc, int solve_failed, int max_iters) {
  double tmp = tchi;
  double scale = sc + 1e-3;
  if (solve_failed) { tmp = INFINITY; scale = 1.0; S.solve_failed += 1; }
  const double rho = (S.cur_chi - tmp) / scale;
  S.tmp_chi = tmp; S.scale = scale; S.rho = rho; S.trials += 1;
  if (rho > 0 && isfinite(tmp)) {
    double a = 2 * rho - 1;
    double alpha = 1.0 - a * a * a;
    alpha = fmin(alpha, 2.0 / 3.0);
    const double sf = fmax(1.0 / 3.0, alpha);
    S.lambda *= sf; S.nu = 2; S.cur_chi = tmp; S.accept = 1;
  } else {
    S.lambda *= S.nu; S.nu *= 2; S.accept = 0;
  }
  S.q += 1;
  const int again = (rho < 0 && S.q < 10);
  S.in_trial = again;   // a rejected trial is repeated at the next step with the raised lambda
  if (!again) {
    S.iter += 1;
    if (S.q == 10 || rho == 0) { S.status = 1; S.active = 0; }
    else if (S.iter >= max_iters) { S.status = 0; S.active = 0; }
    else S.lin = 1;     // next step: new linearisation, new iteration
  }
}

// position prior k (batch index): its error e = t(X) - z (the first ep_dim components; the rest 0) and Omega
__device__ __forceinline__ void prior_error(const BatchView& V, int k, const Pose& X, double err[3], double W[9]) {
  const size_t n = V.nEp;
  const int dim = V.ep_dim[k];
  err[0] = X.t.x - V.ep_z[0 * n + k];
  err[1] = X.t.y - V.ep_z[1 * n + k];
  err[2] = dim == 3 ? X.t.z - V.ep_z[2 * n + k] : 0.0;
  load_sym3(V.ep_w, (int)n, k, W);
}
// its chi2 term.  Out of line: the persistent solver kernels inline edge_chi2, and the prior branch must not move their register budget.
__device__ __forceinline__ double prior_chi2(const BatchView& V, int k, const double* __restrict__ pose) {
  double err[3], W[9];
  prior_error(V, k, load_pose(pose, V.ep_pose[k]), err, W);
  return quad3(W, err);
}

// chi2 term of the graph-local edge e of graph segment sg (SE3 edges, then landmark edges, then point-point edges, then position priors;
// 0 beyond the last): g2o computeActiveErrors + the robust kernel's rho[0].  RK: the batch carries per-edge kernels.
// RAW: e^T Omega e, no kernel at all.
template <bool RK = false, bool RAW = false>
__device__ __forceinline__ double edge_chi2(const BatchView& V, const GraphSeg& sg, int e, const double* __restrict__ pose, const double* __restrict__ lmk) {
  double c = 0;
  if (e < sg.neo) {
    const int k = sg.eo0 + e;
    const Pose Xi = load_pose(pose, V.eo_i[k]), Xj = load_pose(pose, V.eo_j[k]);
    const int n = V.nEo;
    Se3Lin L;
    se3_error(Xi, Xj, load_meas_pose(V.eo_z, n, k), L);
    if constexpr (RK || RAW) {   // the e2 the robust linearisation forms (se3_e2), then the edge's own kernel
      c = se3_e2(V.eo_w, n, k, L.e);
      if constexpr (!RAW) { const auto K = info_scale<RK>(V.eo_rk, V.eo_rd, k, 0.0); if (K.kind) c = K.rho0(c); }
      return c;
    }
    double W[36];
    load_sym6(V.eo_w, n, k, W);
    for (int r = 0; r < 6; ++r) {
      double a = 0;
      for (int s = 0; s < 6; ++s) a += W[r * 6 + s] * L.e[s];
      c += L.e[r] * a;
    }
  } else if (e < sg.neo + sg.nel) {
    const int k = sg.el0 + (e - sg.neo);
    double err[3];
    lm_edge_error(V, k, load_pose(pose, V.el_p[k]), lmk, err);
    double W[9];
    load_sym3(V.el_w, V.nEl, k, W);
    for (int r = 0; r < 3; ++r) {
      double a = 0;
      for (int s = 0; s < 3; ++s) a += W[r * 3 + s] * err[s];
      c += err[r] * a;
    }
    if constexpr (!RAW) { const auto K = info_scale<RK>(V.el_rk, V.el_rd, k, V.dcs_phi); if (K.kind) c = K.rho0(c); }
  } else if (e < sg.neo + sg.nel + sg.nell) {
    const int k = sg.ell0 + (e - sg.neo - sg.nel);
    double err[3], W[9];
    ll_edge_error(V, lmk, k, err);
    load_sym3(V.ell_w, V.nEll, k, W);
    c = quad3(W, err);
    if constexpr (!RAW) { const auto K = info_scale<RK>(V.ell_rk, V.ell_rd, k, 0.0); if (K.kind) c = K.rho0(c); }
  } else if (e < edge_count(sg)) {
    const int k = sg.ep0 + (e - sg.neo - sg.nel - sg.nell);
    c = prior_chi2(V, k, pose);
    if constexpr (!RAW) { const auto K = info_scale<RK>(V.ep_rk, V.ep_rd, k, 0.0); if (K.kind) c = K.rho0(c); }
  }
  return c;
}
// the kernel that edge e of segment sg is under (edge_chi2's order of edges)
template <bool RK>
__device__ __forceinline__ EdgeKernel<RK> edge_kernel_of(const BatchView& V, const GraphSeg& sg, int e) {
  if (e < sg.neo) return info_scale<RK>(V.eo_rk, V.eo_rd, sg.eo0 + e, 0.0);
  if (e < sg.neo + sg.nel) return info_scale<RK>(V.el_rk, V.el_rd, sg.el0 + (e - sg.neo), V.dcs_phi);
  if (e < sg.neo + sg.nel + sg.nell) return info_scale<RK>(V.ell_rk, V.ell_rd, sg.ell0 + (e - sg.neo - sg.nel), 0.0);
  if (e < edge_count(sg)) return info_scale<RK>(V.ep_rk, V.ep_rd, sg.ep0 + (e - sg.neo - sg.nel - sg.nell), 0.0);
  return {RK_NONE, 0.0};
}

}  // namespace sslam
