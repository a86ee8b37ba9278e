// MI355X-native backend of ps_graph_slam::GraphSLAM — kernels, batch engine and C-ABI.
// See include/sslam.h for the boundary and DESIGN.md for the data layout / roofline accounting.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the library is bound at run time (rccl_api below)
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <thread>
#include <vector>

#include "../../include/sslam.h"
#include "graph_host.hpp"
#include "graph_kernels.hpp"
#include "sslam_common.hpp"
#include "graph_engine.hpp"
#include "chol_plan.hpp"

namespace sslam {

// =============================================================================================
// Kernels
// =============================================================================================

// ---- residual / chi2 (g2o computeActiveErrors): per-graph partial sums, deterministic ---------
template <bool RK>
__global__ __launch_bounds__(kEdgeChunk) void k_chi2(BatchView V, const double* __restrict__ pose,
                                                    const double* __restrict__ lmk, int mask_mode,
                                                    double* __restrict__ part) {
  __shared__ double red[kEdgeChunk / 64];
  const int g = blockIdx.y;
  const LmState& S = V.lm[g];
  if (mask_mode == 1 && !S.in_trial) return;
  if (mask_mode == 2 && !S.active) return;
  const GraphSeg sg = V.seg[g];
  const int e = blockIdx.x * kEdgeChunk + threadIdx.x;
  if (blockIdx.x * kEdgeChunk >= edge_count(sg)) return;
  const double c = edge_chi2<RK>(V, sg, e, pose, lmk);
  const double s = block_sum<kEdgeChunk>(c, red);
  if (threadIdx.x == 0) part[(size_t)g * V.maxEdgeChunks + blockIdx.x] = s;
}

// sslam_graph_edge_chi2: one thread per requested edge (loc: its graph-local index in edge_chi2's order) -> e^T Omega e, rho0 and rho1 of the
// kernel the edge is under, at the current estimates.  out: [3][n].  No atomics, no reduction.
template <bool RK>
__global__ __launch_bounds__(64) void k_edge_chi2(BatchView V, int g, const int* __restrict__ loc, int n, double* __restrict__ out) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const GraphSeg sg = V.seg[g];
  const int e = loc[t];
  const double e2 = edge_chi2<false, true>(V, sg, e, V.pose, V.lmk);
  double r0 = e2, r1 = 1.0;
  const auto K = edge_kernel_of<RK>(V, sg, e);
  if (K.kind) K.rho(e2, r0, r1);
  out[t] = e2; out[(size_t)n + t] = r0; out[2 * (size_t)n + t] = r1;
}

// off-diagonal block codes: >= 0 owner edge, <= -2 a further edge on the same vertex pair, -1 none
__device__ __forceinline__ int decode_blk(int code) { return code <= -2 ? -2 - code : code; }

// ---- Jacobian build (gather form, deterministic, no atomics): one THREAD per pose row ---------------
// No redundancy across lanes: a thread evaluates each incident edge once, keeps the 6x6 Jacobian of
// its own vertex in registers, streams the other vertex's columns for the off-diagonal block it
// owns, and accumulates the symmetric diagonal block (21 values) + b (6) in a thread-private LDS
// column (lane-contiguous layout -> conflict free), written to HBM once at the end.  All block stores
// are 16-byte (two doubles): half the write requests of scalar stores at a 288-byte lane stride.
constexpr int kRowThreads = 64;
__device__ __forceinline__ int tri21(int a, int c) { return a * 6 - (a * (a - 1)) / 2 + (c - a); }   // a <= c

__device__ __forceinline__ Pose load_pose16(const double* a, int idx) {   // four 16-byte loads of the 64-byte record
  const D2* p = reinterpret_cast<const D2*>(a + (size_t)idx * 8);
  const D2 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
  return Pose{{v0.a, v0.b, v1.a}, {v1.b, v2.a, v2.b, v3.a}};
}

// EdgeSE3Plane (reference include/g2o/edge_se3_plane.hpp:8-48; g2o's BaseBinaryEdge numeric Jacobian: central differences, delta 1e-9): 19
// evaluations of the error per edge -- the error itself, +/- delta on the six components of the pose and on the three of the plane -- each ~900
// FP64 instructions.  A thread per (edge, evaluation) -- a pair of + / - evaluations sits in neighbouring lanes and meets through one shuffle --
// at full occupancy, every evaluation done once; the row kernels read the 30 doubles (DESIGN.md section 5 has the timings).
constexpr int kPjDoubles = 30;   // {e 3 | J_l 3 x 3 row-major | J_i 3 x 6 row-major}
// Two regions of workgroups so that a wave runs ONE of the two perturbation paths (se3_oplus / pl_oplus: ~150 / ~300 instructions next to the
// ~400 of the error itself; mixed in one wave both would be paid by every lane): blocks [0, blocksA) hold fourteen
// lanes per edge -- lane 0 the error, lane 1 idle, lanes 2 + 2 d / 3 + 2 d the + / - evaluations of pose component d --, the blocks behind them
// six lanes per edge, the + / - evaluations of the three plane components.  A pair sits in neighbouring lanes (even lane counts per edge).
__global__ __launch_bounds__(256) void k_plane_jacobians(BatchView V, int blocksA) {
  const bool regA = (int)blockIdx.x < blocksA;
  const int per = regA ? 14 : 6;
  const long long t = (long long)(regA ? blockIdx.x : blockIdx.x - blocksA) * 256 + threadIdx.x;
  const long long e64 = t / per;
  const int j = (int)(t - e64 * per);
  const bool in = e64 < V.nEl;
  const int e = in ? (int)e64 : 0;
  const int pi = V.el_p[e], li = V.el_l[e];
  bool live = in && V.lm_kind[li] == VT_PLANE && !(regA && j == 1);
  if (live) {
    const int pr = V.pose_row[pi], lr = V.lm_row[li];
    const int g = pr >= 0 ? V.prow_graph[pr] : (lr >= 0 ? V.lrow_graph[lr] : -1);
    live = g >= 0 && V.lm[g].lin;
  }
  const double delta = 1e-9;
  double err[3] = {0, 0, 0};
  if (live) {
    // (loads spelled out: through load_plane / el_meas_plane the error contracts differently, 3e-10 of H after the central differences)
    const size_t n = (size_t)V.nEl;
    Pose Xi = load_pose(V.pose, pi);
    const double* lp = V.lmk + (size_t)li * 4;
    Plane pw{{lp[0], lp[1], lp[2]}, lp[3]};
    const Plane z{{V.el_z[0 * n + e], V.el_z[1 * n + e], V.el_z[2 * n + e]}, V.el_z[3 * n + e]};
    const double sd = (j & 1) ? -delta : delta;
    if (regA) {
      if (j >= 2) {
        const int d = (j - 2) >> 1;
        double dv[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) dv[q] = q == d ? sd : 0.0;
        Xi = se3_oplus(Xi, dv);
      }
    } else {
      const int d = j >> 1;
      double d3[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) d3[q] = q == d ? sd : 0.0;
      pw = pl_oplus(pw, d3);
    }
    plane_error(Xi, pw, z, err);
  }
  // the - evaluation of a pair sits one lane up
  const double m0 = __shfl_down(err[0], 1, 64), m1 = __shfl_down(err[1], 1, 64), m2 = __shfl_down(err[2], 1, 64);
  if (!live || (j & 1)) return;
  double* o = V.pj + (size_t)e * kPjDoubles;
  if (regA && j == 0) { o[0] = err[0]; o[1] = err[1]; o[2] = err[2]; return; }
  const double scalar = 1.0 / (2 * delta);
  const double c0 = scalar * (err[0] - m0), c1 = scalar * (err[1] - m1), c2 = scalar * (err[2] - m2);
  if (regA) { const int d = (j - 2) >> 1; o[12 + d] = c0; o[18 + d] = c1; o[24 + d] = c2; }
  else { const int d = j >> 1; o[3 + d] = c0; o[6 + d] = c1; o[9 + d] = c2; }
}

// Pose-row kernel: every slot (incident edge) of a row evaluated by the row's own thread, contributions summed in slot order.
// The kernel is bound by the life time of ONE wave per SIMD (both Jacobians 45, Omega 27, J^T Omega 36, an off-diagonal block 36 doubles live
// at once: 256 VGPRs + AGPRs) -- the instruction issue of a single FP64 wave plus the round trips it cannot overlap -- not by bytes,
// occupancy alone or the shape of its stores (DESIGN.md section 5 keeps the forms measured against it).  So nothing here may lengthen a
// live range: the 3 x 3 block algebra below stays written out.  PL: the batch holds plane landmarks.  SHARD: edge-sharded mode, an edge
// outside this rank's range counts with Omega = 0.  RK: the batch carries per-edge robust kernels; <RK = false> holds no code for them.
template <bool PL, bool SHARD, bool RK>
__global__ __launch_bounds__(kRowThreads, 1) void k_linearize_rowthread(BatchView V) {
  __shared__ double accD[27][kRowThreads];   // this row's diagonal block (upper triangle) and rhs: a thread-private LDS column, conflict free
  const int tid = threadIdx.x;
  const int slot_t = blockIdx.x * kRowThreads + tid;
  if (slot_t >= V.nPr) return;
  const int row = V.prow_perm[slot_t];   // (rows of equal slot counts share a wave)
  if (!V.lm[V.prow_graph[row]].lin) return;
#pragma unroll
  for (int k = 0; k < 27; ++k) accD[k][tid] = 0.0;
  const int s0 = V.pslot_ptr[row], s1 = V.pslot_ptr[row + 1];
  const int own = V.prow_pose[row];
  const int g = V.prow_graph[row];
  const Pose Xown = load_pose16(V.pose, own);   // this row's vertex: loaded once, reused by every slot
  for (int s = s0; s < s1; ++s) {
    const int4 rec = V.pslot_rec[s];
    const int e = rec.x, kind = rec.y & 15, ia = rec.z, ib = rec.w;
    if (kind != 2) {
      // EdgeSE3: both Jacobians are 2 x 2 block upper triangular in 3 x 3 blocks,
      //   J_i = [[-Ra, 2 Ra [tb]x], [0, Ci]],   J_j = [[Re, 0], [0, Fj]],
      // so J^T Omega J is formed from 3 x 3 products of the blocks (half the FMAs and a smaller live set than dense 6 x 6).
      const int n = V.nEo;
      const bool iside = (kind == 0);
      Se3Lin L;
      const Pose Xo = load_pose16(V.pose, iside ? ib : ia);
      const Pose Zm = load_meas_pose(V.eo_z, n, e);
      se3_error(iside ? Xown : Xo, iside ? Xo : Xown, Zm, L);
      double P[9], Q[9], R[9];   // Omega = [[P, Q], [Q^T, R]]
      // edge-sharded mode: an edge outside this rank's range contributes nothing (everything below is linear in Omega; the owner
      // of an off-diagonal block still writes it, as zeros)
      double mk = in_shard<SHARD>(V, g, V.eo_id, e) ? 1.0 : 0.0;
      auto w21 = [&](int q) { return V.eo_w[(size_t)q * n + e]; };
      const auto K = info_scale<RK>(V.eo_rk, V.eo_rd, e, 0.0);
      if (K.kind) mk *= K.rho1(se3_e2(V.eo_w, n, e, L.e));
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          P[r * 3 + c] = mk * w21(r <= c ? tri21(r, c) : tri21(c, r));
          Q[r * 3 + c] = mk * w21(tri21(r, 3 + c));
          R[r * 3 + c] = mk * w21(r <= c ? tri21(3 + r, 3 + c) : tri21(3 + c, 3 + r));
        }
      double A[9], B[9], Cc[9];   // own Jacobian [[A, B], [0, Cc]]  (B = 0 on the j side)
      if (iside) {
        const Vec3 tb = L.tb;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double r0 = L.Ra.m[r * 3], r1 = L.Ra.m[r * 3 + 1], r2 = L.Ra.m[r * 3 + 2];
          A[r * 3] = -r0; A[r * 3 + 1] = -r1; A[r * 3 + 2] = -r2;
          B[r * 3 + 0] = 2 * (r1 * tb.z - r2 * tb.y);     // Ra * (0, tz, -ty)
          B[r * 3 + 1] = 2 * (-r0 * tb.z + r2 * tb.x);    // Ra * (-tz, 0, tx)
          B[r * 3 + 2] = 2 * (r0 * tb.y - r1 * tb.x);     // Ra * (ty, -tx, 0)
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const Quat vk = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, 0.0};
          const Quat t = qmul(qmul(L.qa, vk), L.qb);
          Cc[0 * 3 + k] = -L.s * t.x; Cc[1 * 3 + k] = -L.s * t.y; Cc[2 * 3 + k] = -L.s * t.z;
        }
      }
      double E[9], F[9];          // J_j = [[E, 0], [0, F]]
      {
        const Mat3 Re = qmat(L.qe);
        const double w = L.s * L.qe.w, x = L.s * L.qe.x, y = L.s * L.qe.y, z = L.s * L.qe.z;
#pragma unroll
        for (int q = 0; q < 9; ++q) E[q] = Re.m[q];
        F[0] = w; F[1] = -z; F[2] = y; F[3] = z; F[4] = w; F[5] = -x; F[6] = -y; F[7] = x; F[8] = w;
      }
      if (!iside) {
#pragma unroll
        for (int q = 0; q < 9; ++q) { A[q] = E[q]; B[q] = 0.0; Cc[q] = F[q]; }
      }
      // M = J_self^T Omega = [[A^T P, A^T Q], [B^T P + C^T Q^T, B^T Q + C^T R]]
      double M11[9], M12[9], M21[9], M22[9];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double m11 = 0, m12 = 0, m21 = 0, m22 = 0;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            m11 += A[r * 3 + a] * P[r * 3 + c];
            m12 += A[r * 3 + a] * Q[r * 3 + c];
            m21 += Cc[r * 3 + a] * Q[c * 3 + r];
            m22 += Cc[r * 3 + a] * R[r * 3 + c];
          }
          if (iside) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { m21 += B[r * 3 + a] * P[r * 3 + c]; m22 += B[r * 3 + a] * Q[r * 3 + c]; }
          }
          M11[a * 3 + c] = m11; M12[a * 3 + c] = m12; M21[a * 3 + c] = m21; M22[a * 3 + c] = m22;
        }
      const int blk = iside ? V.eo_blk[e] : -1;
      if (blk >= 0) {   // owner of the off-diagonal block: J_i^T Omega J_j = [[M11 E, M12 F], [M21 E, M22 F]]
        double* O = V.Hpp_off + (size_t)(blk >> 1) * 36;
        const bool swapped = blk & 1;
        double o[36];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            double o11 = 0, o12 = 0, o21 = 0, o22 = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
              o11 += M11[a * 3 + r] * E[r * 3 + c]; o12 += M12[a * 3 + r] * F[r * 3 + c];
              o21 += M21[a * 3 + r] * E[r * 3 + c]; o22 += M22[a * 3 + r] * F[r * 3 + c];
            }
            o[a * 6 + c] = o11; o[a * 6 + 3 + c] = o12; o[(3 + a) * 6 + c] = o21; o[(3 + a) * 6 + 3 + c] = o22;
          }
        if (!swapped) {   // stored [row_i][row_j]
#pragma unroll
          for (int k = 0; k < 36; k += 2) store2(O + k, o[k], o[k + 1]);
        } else {          // stored transposed
#pragma unroll
          for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int a = 0; a < 6; a += 2) store2(O + c * 6 + a, o[a * 6 + c], o[(a + 1) * 6 + c]);
        }
      }
      // diagonal block J^T Omega J (upper triangle) and b -= J^T Omega e
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double d11 = 0, d12 = 0, d22 = 0;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            d11 += M11[a * 3 + r] * A[r * 3 + c];
            d12 += M12[a * 3 + r] * Cc[r * 3 + c];
            d22 += M22[a * 3 + r] * Cc[r * 3 + c];
          }
          if (iside) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { d12 += M11[a * 3 + r] * B[r * 3 + c]; d22 += M21[a * 3 + r] * B[r * 3 + c]; }
          }
          if (a <= c) { accD[tri21(a, c)][tid] += d11; accD[tri21(3 + a, 3 + c)][tid] += d22; }
          accD[tri21(a, 3 + c)][tid] += d12;
        }
        accD[21 + a][tid] -= M11[a * 3] * L.e[0] + M11[a * 3 + 1] * L.e[1] + M11[a * 3 + 2] * L.e[2] +
                             M12[a * 3] * L.e[3] + M12[a * 3 + 1] * L.e[4] + M12[a * 3 + 2] * L.e[5];
        accD[24 + a][tid] -= M21[a * 3] * L.e[0] + M21[a * 3 + 1] * L.e[1] + M21[a * 3 + 2] * L.e[2] +
                             M22[a * 3] * L.e[3] + M22[a * 3 + 1] * L.e[4] + M22[a * 3 + 2] * L.e[5];
      }
    } else {
      double err[3], Ji[18], Jl[9];   // Ji row-major 3x6, Jl row-major 3x3
      if (!PL || V.lm_kind[ib] == VT_POINT) {
        PointLin L;
        point_error(Xown, load_point(V.lmk, ib), el_meas_point(V, e), L);
        point_jacobians(L, Ji, Jl);
        err[0] = L.e[0]; err[1] = L.e[1]; err[2] = L.e[2];
      } else {
        // error and both Jacobians from k_plane_jacobians (fifteen 16-byte loads instead of nineteen evaluations)
        const D2* pj = reinterpret_cast<const D2*>(V.pj + (size_t)e * kPjDoubles);
        double v[kPjDoubles];
#pragma unroll
        for (int q = 0; q < kPjDoubles / 2; ++q) { const D2 w = pj[q]; v[2 * q] = w.a; v[2 * q + 1] = w.b; }
#pragma unroll
        for (int q = 0; q < 3; ++q) err[q] = v[q];
#pragma unroll
        for (int q = 0; q < 9; ++q) Jl[q] = v[3 + q];
#pragma unroll
        for (int q = 0; q < 18; ++q) Ji[q] = v[12 + q];
      }
      double W[9];
      load_sym3(V.el_w, V.nEl, e, W);
      const auto K = info_scale<RK>(V.el_rk, V.el_rd, e, V.dcs_phi);
      const double rho1 = K.kind ? K.rho1(quad3(W, err)) : 1.0;   // from the unmasked Omega: every rank scales its share alike
      // (the zero and scale loops stay written out, here and in the other kernels: as functions they change this kernel's instructions)
      if (!in_shard<SHARD>(V, g, V.el_id, e)) {
#pragma unroll
        for (int q = 0; q < 9; ++q) W[q] = 0.0;
      }
      if (K.kind) {
#pragma unroll
        for (int q = 0; q < 9; ++q) W[q] *= rho1;
      }
      double WJi[18], We[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        We[a] = W[a * 3 + 0] * err[0] + W[a * 3 + 1] * err[1] + W[a * 3 + 2] * err[2];
#pragma unroll
        for (int c = 0; c < 6; ++c) WJi[a * 6 + c] = W[a * 3 + 0] * Ji[c] + W[a * 3 + 1] * Ji[6 + c] + W[a * 3 + 2] * Ji[12 + c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int a = 0; a <= c; ++a) accD[tri21(a, c)][tid] += Ji[a] * WJi[c] + Ji[6 + a] * WJi[6 + c] + Ji[12 + a] * WJi[12 + c];
        accD[21 + c][tid] -= Ji[c] * We[0] + Ji[6 + c] * We[1] + Ji[12 + c] * We[2];
      }
      const int blk = V.el_blk[e];
      if (blk >= 0) {
        double WJl[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) WJl[a * 3 + c] = W[a * 3 + 0] * Jl[c] + W[a * 3 + 1] * Jl[3 + c] + W[a * 3 + 2] * Jl[6 + c];
        double o[18];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) o[a * 3 + c] = Ji[a] * WJl[c] + Ji[6 + a] * WJl[3 + c] + Ji[12 + a] * WJl[6 + c];
        double* O = V.Hpl + (size_t)blk * 18;
#pragma unroll
        for (int k = 0; k < 18; k += 2) store2(O + k, o[k], o[k + 1]);
      }
    }
  }
  double* P = V.Hpp_diag + (size_t)row * 36;
  double* Bv = V.bvec + (size_t)row * 6;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6; c += 2)
      store2(P + a * 6 + c, accD[a <= c ? tri21(a, c) : tri21(c, a)][tid], accD[a <= c + 1 ? tri21(a, c + 1) : tri21(c + 1, a)][tid]);
#pragma unroll
  for (int c = 0; c < 6; c += 2) store2(Bv + c, accD[21 + c][tid], accD[22 + c][tid]);
}

// Position priors (hdl_graph_slam's EdgeSE3PriorXY / EdgeSE3PriorXYZ): e = t(X) - z, J = [R | 0] with X <- X exp(delta), so a prior adds
// R^T Omega R to the upper-left 3 x 3 of its pose's diagonal block and -R^T Omega e to the first three entries of the rhs.  One thread per
// pose row that carries priors: the pose is read once, its priors summed in edge order, and the sums added onto the block and rhs that
// k_linearize_rowthread wrote before it in stream order.  No atomics: bitwise deterministic.  A separate launch (and only for a batch that
// has priors) rather than a slot kind of the row kernel, whose live set is what bounds it (comment above k_linearize_rowthread).
template <bool SHARD, bool RK>
__global__ __launch_bounds__(64) void k_linearize_priors(BatchView V) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= V.nEpRows) return;
  const int row = V.ep_row[t];
  const int g = V.prow_graph[row];
  if (!V.lm[g].lin) return;
  const Pose X = load_pose(V.pose, V.prow_pose[row]);
  const Mat3 R = qmat(X.q);
  double h[6] = {0, 0, 0, 0, 0, 0}, bb[3] = {0, 0, 0};   // upper triangle of the 3 x 3 block (tri3 order), rhs
  for (int s = V.ep_ptr[t]; s < V.ep_ptr[t + 1]; ++s) {
    const int k = V.ep_edge[s];
    double err[3], W[9];
    prior_error(V, k, X, err, W);
    const auto K = info_scale<RK>(V.ep_rk, V.ep_rd, k, 0.0);
    if (K.kind) {
      const double rho1 = K.rho1(quad3(W, err));
#pragma unroll
      for (int q = 0; q < 9; ++q) W[q] *= rho1;
    }
    if (!in_shard<SHARD>(V, g, V.ep_id, k)) {
#pragma unroll
      for (int q = 0; q < 9; ++q) W[q] = 0.0;
    }
    double M[9], We[3];   // M = R^T Omega (3 x 3), We = Omega e
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      We[a] = W[a * 3 + 0] * err[0] + W[a * 3 + 1] * err[1] + W[a * 3 + 2] * err[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) M[a * 3 + c] = R.m[0 * 3 + a] * W[0 * 3 + c] + R.m[1 * 3 + a] * W[1 * 3 + c] + R.m[2 * 3 + a] * W[2 * 3 + c];
    }
    int q = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int c = a; c < 3; ++c) h[q++] += M[a * 3 + 0] * R.m[0 * 3 + c] + M[a * 3 + 1] * R.m[1 * 3 + c] + M[a * 3 + 2] * R.m[2 * 3 + c];
      bb[a] -= R.m[0 * 3 + a] * We[0] + R.m[1 * 3 + a] * We[1] + R.m[2 * 3 + a] * We[2];
    }
  }
  double* P = V.Hpp_diag + (size_t)row * 36;
  double* Bv = V.bvec + (size_t)row * 6;
  int q = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int c = a; c < 3; ++c) {
      P[a * 6 + c] += h[q];
      if (c != a) P[c * 6 + a] += h[q];
      ++q;
    }
    Bv[a] += bb[a];
  }
}

// landmark rows: 16 lanes per landmark, each lane walks a strided subset of the incident edges,
// butterfly reduction in a fixed order.
// (Three things stay spelled out here, because each one alone, written through its helper, changes bytes of H: the point loads and
// ll_edge_error in the unsharded <PL = true> forms, 1e-20 of max |H|, and in_shard in the <SHARD = true> forms, 2e-18.)
template <bool PL, bool SHARD, bool RK>
__global__ __launch_bounds__(256) void k_linearize_lm_rows(BatchView V) {
  const int l = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int lane = threadIdx.x & 15;
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0;
  bool live = l < V.nLr;
  if (live && !V.lm[V.lrow_graph[l]].lin) live = false;
  if (live) {
    const int li = V.lrow_lm[l];
    const double* lp = V.lmk + (size_t)li * 4;
    const int n = V.nEl;
    const bool is_point = !PL || V.lm_kind[li] == VT_POINT;
    for (int s = V.lslot_ptr[l] + lane; s < V.lslot_ptr[l + 1]; s += 16) {
      const int e = V.lslot_edge[s];
      const Pose Xi = load_pose(V.pose, V.el_p[e]);
      double err[3], Jl[9];
      if (is_point) {
        PointLin L;
        point_error(Xi, Vec3{lp[0], lp[1], lp[2]}, Vec3{V.el_z[0 * (size_t)n + e], V.el_z[1 * (size_t)n + e], V.el_z[2 * (size_t)n + e]}, L);
        err[0] = L.e[0]; err[1] = L.e[1]; err[2] = L.e[2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) Jl[a * 3 + c] = L.R.m[c * 3 + a];
      } else {
        const double* pj = V.pj + (size_t)e * kPjDoubles;   // from k_plane_jacobians: {e | J_l | ...}
#pragma unroll
        for (int q = 0; q < 3; ++q) err[q] = pj[q];
#pragma unroll
        for (int q = 0; q < 9; ++q) Jl[q] = pj[3 + q];
      }
      double W[9];
      load_sym3(V.el_w, n, e, W);
      const auto K = info_scale<RK>(V.el_rk, V.el_rd, e, V.dcs_phi);
      if (K.kind) {
        const double rho1 = K.rho1(quad3(W, err));
#pragma unroll
        for (int q = 0; q < 9; ++q) W[q] *= rho1;
      }
      if (SHARD) {
        const int g = V.lrow_graph[l];
        if (!(V.el_id[e] >= V.shard_lo[g] && V.el_id[e] < V.shard_hi[g])) {
#pragma unroll
          for (int q = 0; q < 9; ++q) W[q] = 0.0;
        }
      }
      double WJ[9], We[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        We[a] = W[a * 3 + 0] * err[0] + W[a * 3 + 1] * err[1] + W[a * 3 + 2] * err[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) WJ[a * 3 + c] = W[a * 3 + 0] * Jl[c] + W[a * 3 + 1] * Jl[3 + c] + W[a * 3 + 2] * Jl[6 + c];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[a * 3 + c] += Jl[a] * WJ[c] + Jl[3 + a] * WJ[3 + c] + Jl[6 + a] * WJ[6 + c];
        acc[9 + a] -= Jl[a] * We[0] + Jl[3 + a] * We[1] + Jl[6 + a] * We[2];
      }
    }
  }
  if (live && V.nEll > 0) {
    // point-point edges of this landmark: J = -I on the first vertex, +I on the second  ->  H_ll += Omega, b -/+= Omega e
    const size_t n = V.nEll;
    for (int s = V.llslot_ptr[l] + lane; s < V.llslot_ptr[l + 1]; s += 16) {
      const int2 rec = V.llslot_rec[s];
      const int k = rec.x;
      const double* pa = V.lmk + (size_t)V.ell_a[k] * 4;
      const double* pb = V.lmk + (size_t)V.ell_b[k] * 4;
      double err[3], W[9];
#pragma unroll
      for (int r = 0; r < 3; ++r) err[r] = (pb[r] - pa[r]) - V.ell_z[r * n + k];
      load_sym3(V.ell_w, (int)n, k, W);
      const auto K = info_scale<RK>(V.ell_rk, V.ell_rd, k, 0.0);
      if (K.kind) {
        const double rho1 = K.rho1(quad3(W, err));
#pragma unroll
        for (int q = 0; q < 9; ++q) W[q] *= rho1;
      }
      if (SHARD) {
        const int g = V.lrow_graph[l];
        if (!(V.ell_id[k] >= V.shard_lo[g] && V.ell_id[k] < V.shard_hi[g])) {
#pragma unroll
          for (int q = 0; q < 9; ++q) W[q] = 0.0;
        }
      }
      const double sgn = rec.y ? -1.0 : 1.0;   // b = -J^T Omega e
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[a * 3 + c] += W[a * 3 + c];
        acc[9 + a] += sgn * (W[a * 3 + 0] * err[0] + W[a * 3 + 1] * err[1] + W[a * 3 + 2] * err[2]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    double v = acc[q];
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 1, 64);
    acc[q] = v;
  }
  if (live && lane == 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) V.Hll_diag[(size_t)l * 9 + q] = acc[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) V.bvec[(size_t)6 * V.nPr + (size_t)3 * l + q] = acc[9 + q];
  }
}

// landmark-landmark blocks of the point-point edges: block (a, b) = sum over the edges on that pair of J_a^T Omega J_b = -Omega
template <bool SHARD, bool RK>
__global__ __launch_bounds__(64) void k_linearize_ll(BatchView V) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= V.nLL) return;
  const int e0 = V.llblk_ptr[i], e1 = V.llblk_ptr[i + 1];
  const int g = V.lrow_graph[V.lm_row[V.ell_a[V.llblk_edge[e0]]]];
  if (!V.lm[g].lin) return;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int e = e0; e < e1; ++e) {
    const int k = V.llblk_edge[e];
    if (!in_shard<SHARD>(V, g, V.ell_id, k)) continue;
    double W[9];
    load_sym3(V.ell_w, V.nEll, k, W);
    const auto K = info_scale<RK>(V.ell_rk, V.ell_rd, k, 0.0);
    if (K.kind) {   // the same e2 from the same inputs as the two landmark rows of the edge form
      double err[3];
      ll_edge_error(V, V.lmk, k, err);
      const double rho1 = K.rho1(quad3(W, err));
#pragma unroll
      for (int q = 0; q < 9; ++q) W[q] *= rho1;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) acc[q] -= W[q];
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) V.Hll_off[(size_t)i * 9 + q] = acc[q];
}

// The duplicate lists (dup[0 .. n), edges whose off-diagonal block another edge owns) are ordered by block.  One past the end of the run that
// entry t heads, or t when its predecessor lies on the same block.  shift: the low bits of a block code outside its index (an SE3 block's swap bit).
__device__ __forceinline__ int dup_run_end(const int* __restrict__ dup, const int* __restrict__ blk_of, int shift, int n, int t) {
  auto blk = [&](int d) { return decode_blk(blk_of[dup[d]]) >> shift; };
  if (t >= n || (t > 0 && blk(t - 1) == blk(t))) return t;
  int d = t + 1;
  while (d < n && blk(d) == blk(t)) ++d;
  return d;
}

// Further edges on an already-owned vertex pair (e.g. a repeated loop closure): their off-diagonal contributions are added after the
// owners have written the blocks.  Thread t owns the run of duplicates that share a block with entry t and adds them serially, in edge order.
template <bool SHARD, bool RK>
__global__ void k_linearize_dups(BatchView V) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  for (int d = t, end = dup_run_end(V.dup_eo, V.eo_blk, 1, V.nDupEo, t); d < end; ++d) {
    const int k = V.dup_eo[d];
    const int pi = V.eo_i[k], pj = V.eo_j[k];
    const int g = V.prow_graph[V.pose_row[pi]];
    if (!V.lm[g].lin || !in_shard<SHARD>(V, g, V.eo_id, k)) continue;
    Se3Lin L;
    se3_error(load_pose(V.pose, pi), load_pose(V.pose, pj), load_meas_pose(V.eo_z, V.nEo, k), L);
    double Ji[36], Jj[36], W[36], WJ[36];
    se3_full_jacobians(L, Ji, Jj);
    load_sym6(V.eo_w, V.nEo, k, W);
    const auto K = info_scale<RK>(V.eo_rk, V.eo_rd, k, 0.0);
    if (K.kind) {
      const double rho1 = K.rho1(se3_e2(V.eo_w, V.nEo, k, L.e));
      for (int q = 0; q < 36; ++q) W[q] *= rho1;
    }
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) { double a = 0; for (int s = 0; s < 6; ++s) a += W[r * 6 + s] * Jj[s * 6 + c]; WJ[r * 6 + c] = a; }
    const int blk = decode_blk(V.eo_blk[k]);
    double* O = V.Hpp_off + (size_t)(blk >> 1) * 36;
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) {
      double a = 0; for (int s = 0; s < 6; ++s) a += Ji[s * 6 + r] * WJ[s * 6 + c];
      O[(blk & 1) ? c * 6 + r : r * 6 + c] += a;
    }
  }
  for (int d = t, end = dup_run_end(V.dup_el, V.el_blk, 0, V.nDupEl, t); d < end; ++d) {
    const int k = V.dup_el[d];
    const int pi = V.el_p[k], li = V.el_l[k];
    const int g = V.prow_graph[V.pose_row[pi]];
    if (!V.lm[g].lin || !in_shard<SHARD>(V, g, V.el_id, k)) continue;
    const Pose Xi = load_pose(V.pose, pi);
    const bool is_point = V.lm_kind[li] == VT_POINT;
    double err[3], Ji[18], Jl[9], W[9];
    if (is_point) {
      PointLin L;
      point_error(Xi, load_point(V.lmk, li), el_meas_point(V, k), L);
      point_jacobians(L, Ji, Jl);
      err[0] = L.e[0]; err[1] = L.e[1]; err[2] = L.e[2];
    } else {
      plane_jacobians(Xi, load_plane(V.lmk, li), el_meas_plane(V, k), Ji, Jl);
    }
    load_sym3(V.el_w, V.nEl, k, W);
    const auto K = info_scale<RK>(V.el_rk, V.el_rd, k, V.dcs_phi);
    if (K.kind) {
      if (!is_point) lm_edge_error(V, k, Xi, V.lmk, err);   // a plane's Jacobians are central differences: they leave no error behind
      const double rho1 = K.rho1(quad3(W, err));
      for (int q = 0; q < 9; ++q) W[q] *= rho1;
    }
    double WJl[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) WJl[r * 3 + c] = W[r * 3 + 0] * Jl[c] + W[r * 3 + 1] * Jl[3 + c] + W[r * 3 + 2] * Jl[6 + c];
    double* O = V.Hpl + (size_t)decode_blk(V.el_blk[k]) * 18;
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 3; ++c) O[r * 3 + c] += Ji[r] * WJl[c] + Ji[6 + r] * WJl[3 + c] + Ji[12 + r] * WJl[6 + c];
  }
}

// max diagonal entry per graph (lambda init = tau * max diag)
__global__ __launch_bounds__(kRowChunk) void k_maxdiag(BatchView V, double* __restrict__ part) {
  __shared__ double red[kRowChunk / 64];
  const int g = blockIdx.y;
  if (!V.lm[g].lin || V.lm[g].iter != 0) return;   // lambda is initialised from the first linearisation only
  const GraphSeg sg = V.seg[g];
  if (blockIdx.x * kRowChunk >= sg.nprow * 6 + sg.nlrow * 3) return;
  const RowRef R = row_ref(V, sg, blockIdx.x * kRowChunk + threadIdx.x);
  double d = 0;
  if (R.valid) d = fabs(R.is_pose ? V.Hpp_diag[(size_t)R.row * 36 + R.r * 7] : V.Hll_diag[(size_t)R.row * 9 + R.r * 4]);
  const double m = block_max<kRowChunk>(d, red);
  if (threadIdx.x == 0) part[(size_t)g * V.maxRowChunks + blockIdx.x] = m;
}

// One wave per graph, once per step.  A *step* is one damping trial: graphs flagged `lin` have just been re-linearised and
// start a new LM iteration (q = 0; lambda = tau * max diag on the very first one), the others are retrying the
// iteration they are in with the lambda k_lm_control raised.  The host never needs to know which is which.
__global__ void k_lm_begin_step(BatchView V, const double* __restrict__ part_maxdiag) {
  const int g = blockIdx.x;
  LmState& S = V.lm[g];
  if (!S.active) return;
  if (S.lin) {
    if (S.iter == 0) {
      const int n = row_chunks(V.seg[g]);
      double m = 0;
      for (int k = threadIdx.x; k < n; k += 64) m = fmax(m, part_maxdiag[(size_t)g * V.maxRowChunks + k]);
      for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
      if (threadIdx.x == 0) { S.max_diag = m; S.lambda = 1e-5 * m; S.nu = 2.0; }
    }
    if (threadIdx.x == 0) { S.q = 0; S.rho = 0; S.in_trial = 1; S.lin = 0; }
  }
  if (threadIdx.x == 0) S.accept = 0;
}

// initial chi2 -> cur_chi / chi_before.  Graphs with fewer than 10 edges are not optimised (graph_slam.cpp:184-186).
__global__ void k_lm_init(BatchView V, const double* __restrict__ part_chi, int min_edges) {
  const int g = blockIdx.x;
  LmState& S = V.lm[g];
  const GraphSeg sg = V.seg[g];
  const double c = wave_sum_partials(part_chi + (size_t)g * V.maxEdgeChunks, edge_chunks(sg));
  if (threadIdx.x == 0) {
    const bool few = edge_count(sg) < min_edges;   // position priors count: g2o counts graph->edges()
    S.cur_chi = c; S.chi_before = c; S.iter = 0; S.trials = 0; S.pcg_iters = 0;
    S.status = few ? -5 : 0; S.active = few ? 0 : 1; S.lin = few ? 0 : 1;
    S.in_trial = 0; S.accept = 0; S.lambda = 0; S.nu = 2; S.rho = 0; S.q = 0; S.solve_failed = 0;
  }
}

// invert (D + lambda I) per block row -> block-Jacobi preconditioner
template <int N>
__device__ __forceinline__ void spd_inverse(double* A /* N*N row-major, in-place */) {
  // Cholesky A = L L^T (lower in place), then inverse via triangular inverse
  double L[N * N];
  for (int i = 0; i < N * N; ++i) L[i] = 0;
  for (int j = 0; j < N; ++j) {
    double d = A[j * N + j];
    for (int k = 0; k < j; ++k) d -= L[j * N + k] * L[j * N + k];
    d = sqrt(d);
    L[j * N + j] = d;
    for (int i = j + 1; i < N; ++i) {
      double s = A[i * N + j];
      for (int k = 0; k < j; ++k) s -= L[i * N + k] * L[j * N + k];
      L[i * N + j] = s / d;
    }
  }
  // Linv (lower)
  double Li[N * N];
  for (int i = 0; i < N * N; ++i) Li[i] = 0;
  for (int j = 0; j < N; ++j) {
    Li[j * N + j] = 1.0 / L[j * N + j];
    for (int i = j + 1; i < N; ++i) {
      double s = 0;
      for (int k = j; k < i; ++k) s -= L[i * N + k] * Li[k * N + j];
      Li[i * N + j] = s / L[i * N + i];
    }
  }
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) {
      double s = 0;
      for (int k = (r > c ? r : c); k < N; ++k) s += Li[k * N + r] * Li[k * N + c];
      A[r * N + c] = s;
    }
}

__global__ __launch_bounds__(256) void k_precond(BatchView V) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < V.nPr) {
    const int g = V.prow_graph[t];
    if (!V.lm[g].in_trial) return;
    const double lam = V.lm[g].lambda;
    double A[36];
    for (int k = 0; k < 36; ++k) A[k] = V.Hpp_diag[(size_t)t * 36 + k];
    for (int k = 0; k < 6; ++k) A[k * 7] += lam;
    spd_inverse<6>(A);
    for (int k = 0; k < 36; ++k) V.Minv[(size_t)t * 36 + k] = A[k];
  } else if (t < V.nPr + V.nLr) {
    const int l = t - V.nPr;
    const int g = V.lrow_graph[l];
    if (!V.lm[g].in_trial) return;
    const double lam = V.lm[g].lambda;
    double A[9];
    for (int k = 0; k < 9; ++k) A[k] = V.Hll_diag[(size_t)l * 9 + k];
    for (int k = 0; k < 3; ++k) A[k * 4] += lam;
    spd_inverse<3>(A);
    for (int k = 0; k < 9; ++k) V.Minv[(size_t)V.nPr * 36 + (size_t)l * 9 + k] = A[k];
  }
}

// z = Minv * r for the block this scalar row belongs to (rvec staged in LDS by the caller)
__device__ __forceinline__ double apply_minv(const BatchView& V, const RowRef& R, const double* lds_r, int lds_base) {
  double z = 0;
  if (R.is_pose) {
    const double* M = V.Minv + (size_t)R.row * 36 + R.r * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) z += M[c] * lds_r[lds_base + c];
  } else {
    const double* M = V.Minv + (size_t)V.nPr * 36 + (size_t)R.row * 9 + R.r * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) z += M[c] * lds_r[lds_base + c];
  }
  return z;
}

// ---- Schur complement on the landmark block (solver 2, BASELINE.json north_star "Schur-complement + PCG") ------------------------
// PCG runs on the reduced pose system  S = (Hpp + lambda I) - Hpl (Hll + lambda I)^-1 Hlp  without ever forming it: for a vector v
// whose landmark part is  v_l = -(Hll + lambda I)^-1 Hlp v_p,  the pose rows of (H + lambda I) v are S v_p and its landmark rows
// vanish, so the full-space SpMV / update kernels are reused as they are.  One thread per landmark (its 3 x 3 inverse is the
// block-Jacobi preconditioner's, k_precond):
//   mode 0: v_l = -(Hll + lambda I)^-1 (Hlp v_p)
//   mode 1: v_l = -(Hll + lambda I)^-1 b_l and v_p = 0   (then the pose rows of (H + lambda I) v are  -Hpl (Hll + lambda I)^-1 b_l)
//   mode 2: v_l += (Hll + lambda I)^-1 b_l               (the landmarks' back-substitution:  x_l = (Hll + lambda I)^-1 (b_l - Hlp x_p))
__global__ __launch_bounds__(256) void k_schur_lm(BatchView V, double* v, int mode, int parity) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < V.nLr) {
    const int l = t, g = V.lrow_graph[l];
    if (!V.lm[g].in_trial) return;
    if (mode == 0 && V.pcg_done[parity * V.B + g]) return;
    const double* M = V.Minv + (size_t)V.nPr * 36 + (size_t)l * 9;
    const size_t base = (size_t)6 * V.nPr + (size_t)3 * l;
    double s[3] = {0, 0, 0};
    if (mode == 0) {
      const int arow = V.nPr + l;
      const double* Hbase = V.Hpp_diag;
      for (int a = V.adj_ptr[arow]; a < V.adj_ptr[arow + 1]; ++a) {   // a landmark row has pose neighbours only: blocks stored [pose][landmark]
        const double* Bk = Hbase + V.adj_blk[a];
        const double* pn = v + V.adj_x[a];
#pragma unroll
        for (int c = 0; c < 6; ++c) { s[0] += Bk[c * 3] * pn[c]; s[1] += Bk[c * 3 + 1] * pn[c]; s[2] += Bk[c * 3 + 2] * pn[c]; }
      }
    } else {
      s[0] = V.bvec[base]; s[1] = V.bvec[base + 1]; s[2] = V.bvec[base + 2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double m = M[r * 3] * s[0] + M[r * 3 + 1] * s[1] + M[r * 3 + 2] * s[2];
      if (mode == 2) v[base + r] += m; else v[base + r] = -m;
    }
  } else if (mode == 1 && t < V.nLr + V.nPr) {
    const int row = t - V.nLr;
    if (!V.lm[V.prow_graph[row]].in_trial) return;
#pragma unroll
    for (int c = 0; c < 6; ++c) v[(size_t)6 * row + c] = 0.0;
  }
}
__global__ void k_pcg_reset(BatchView V) {   // before the right-hand-side SpMV of the Schur path: flags of the previous solve are stale
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < V.B) { const int d = V.lm[g].in_trial ? 0 : 1; V.pcg_done[g] = d; V.pcg_done[V.B + g] = d; }
}

// PCG start: x = 0, r = b, z = Minv r, p = z; partials of r.z and b.b  (schur: r_p = b_p + q_p with q from the right-hand-side SpMV, r_l = 0)
__global__ __launch_bounds__(kRowChunk) void k_pcg_init(BatchView V, int schur) {
  __shared__ double red[kRowChunk / 64];
  __shared__ double lr[kRowChunk];
  const int g = blockIdx.y;
  if (!V.lm[g].in_trial) return;
  const GraphSeg sg = V.seg[g];
  if (blockIdx.x * kRowChunk >= sg.nprow * 6 + sg.nlrow * 3) return;
  const RowRef R = row_ref(V, sg, blockIdx.x * kRowChunk + threadIdx.x);
  double rv = 0;
  if (R.valid) rv = !schur ? V.bvec[R.xoff] : (R.is_pose ? V.bvec[R.xoff] + V.q[R.xoff] : 0.0);
  lr[threadIdx.x] = rv;
  __syncthreads();
  double zv = 0;
  if (R.valid) {
    zv = apply_minv(V, R, lr, threadIdx.x - R.r);
    V.x[R.xoff] = 0; V.r[R.xoff] = rv; V.z[R.xoff] = zv; V.p[R.xoff] = zv;
  }
  const double s1 = block_sum<kRowChunk>(rv * zv, red);
  const double s2 = block_sum<kRowChunk>(rv * rv, red);
  if (threadIdx.x == 0) {
    V.part_a[(size_t)g * V.maxRowChunks + blockIdx.x] = s1;
    V.part_b[(size_t)g * V.maxRowChunks + blockIdx.x] = s2;
  }
}
__global__ void k_pcg_init2(BatchView V) {
  const int g = blockIdx.x;
  if (!V.lm[g].in_trial) { if (threadIdx.x == 0) { V.pcg_done[g] = 1; V.pcg_done[V.B + g] = 1; } return; }
  const int n = row_chunks(V.seg[g]);
  const double rz = wave_sum_partials(V.part_a + (size_t)g * V.maxRowChunks, n);
  const double bb = wave_sum_partials(V.part_b + (size_t)g * V.maxRowChunks, n);
  if (threadIdx.x == 0) {
    V.rz[g] = rz; V.rz[V.B + g] = rz; V.bb[g] = bb;
    V.pcg_fail[g] = 0;
    const int d = (bb == 0.0 || !(rz > 0)) ? 1 : 0;
    V.pcg_done[g] = d; V.pcg_done[V.B + g] = d;
    if (!(bb == 0.0) && !(rz > 0)) V.pcg_fail[g] = 1;
  }
}

// q = (H + lambda I) p, partial p.q      (block-sparse symmetric SpMV in gather form)
__global__ __launch_bounds__(kRowChunk) void k_spmv(BatchView V, int parity) {
  __shared__ double red[kRowChunk / 64];
  const int g = blockIdx.y;
  if (V.pcg_done[parity * V.B + g]) return;
  const GraphSeg sg = V.seg[g];
  if (blockIdx.x * kRowChunk >= sg.nprow * 6 + sg.nlrow * 3) return;
  const RowRef R = row_ref(V, sg, blockIdx.x * kRowChunk + threadIdx.x);
  double acc = 0, pv = 0;
  if (R.valid) {
    const double* __restrict__ p = V.p;
    pv = p[R.xoff];
    acc = V.lm[g].lambda * pv;
    int arow;
    if (R.is_pose) {
      const double* D = V.Hpp_diag + (size_t)R.row * 36 + R.r * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc += D[c] * p[R.base + c];
      arow = R.row;
    } else {
      const double* D = V.Hll_diag + (size_t)R.row * 9 + R.r * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc += D[c] * p[R.base + c];
      arow = V.nPr + R.row;
    }
    const int a0 = V.adj_ptr[arow], a1 = V.adj_ptr[arow + 1];
    const double* Hbase = V.Hpp_diag;  // all H blocks live in one allocation; adj_blk is an offset from its start
    for (int a = a0; a < a1; ++a) {
      const double* Bk = Hbase + V.adj_blk[a];
      const double* pn = p + V.adj_x[a];
      const int fmt = V.adj_fmt[a];
      if (fmt == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) acc += Bk[R.r * 6 + c] * pn[c];
      } else if (fmt == 1) {
#pragma unroll
        for (int c = 0; c < 6; ++c) acc += Bk[c * 6 + R.r] * pn[c];
      } else if (fmt == 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc += Bk[R.r * 3 + c] * pn[c];
      } else if (fmt == 4) {       // landmark-landmark block, this row first
#pragma unroll
        for (int c = 0; c < 3; ++c) acc += Bk[R.r * 3 + c] * pn[c];
      } else if (fmt == 5) {       // landmark-landmark block, this row second
#pragma unroll
        for (int c = 0; c < 3; ++c) acc += Bk[c * 3 + R.r] * pn[c];
      } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) acc += Bk[c * 3 + R.r] * pn[c];
      }
    }
    V.q[R.xoff] = acc;
  }
  const double s = block_sum<kRowChunk>(pv * acc, red);
  if (threadIdx.x == 0) V.part_a[(size_t)g * V.maxRowChunks + blockIdx.x] = s;
}

// alpha = rz / pq ; x += alpha p ; r -= alpha q ; z = Minv r ; partials of r.z, r.r
__global__ __launch_bounds__(kRowChunk) void k_pcg_update(BatchView V, int parity) {
  __shared__ double red[kRowChunk / 64];
  __shared__ double lr[kRowChunk];
  __shared__ double s_alpha;
  const int g = blockIdx.y;
  if (V.pcg_done[parity * V.B + g]) return;
  const GraphSeg sg = V.seg[g];
  if (blockIdx.x * kRowChunk >= sg.nprow * 6 + sg.nlrow * 3) return;
  if (threadIdx.x < 64) {
    const double pq = wave_sum_partials(V.part_a + (size_t)g * V.maxRowChunks, row_chunks(sg));
    if (threadIdx.x == 0) s_alpha = V.rz[parity * V.B + g] / pq;
  }
  __syncthreads();
  const double alpha = s_alpha;
  const RowRef R = row_ref(V, sg, blockIdx.x * kRowChunk + threadIdx.x);
  double rv = 0;
  if (R.valid) {
    V.x[R.xoff] += alpha * V.p[R.xoff];
    rv = V.r[R.xoff] - alpha * V.q[R.xoff];
    V.r[R.xoff] = rv;
  }
  lr[threadIdx.x] = rv;
  __syncthreads();
  double zv = 0;
  if (R.valid) { zv = apply_minv(V, R, lr, threadIdx.x - R.r); V.z[R.xoff] = zv; }
  const double s1 = block_sum<kRowChunk>(rv * zv, red);
  const double s2 = block_sum<kRowChunk>(rv * rv, red);
  if (threadIdx.x == 0) {
    V.part_b[(size_t)g * V.maxRowChunks + blockIdx.x] = s1;
    V.part_c[(size_t)g * V.maxRowChunks + blockIdx.x] = s2;  // (part_a is still being read by other blocks)
  }
}

// beta = rz_new / rz ; p = z + beta p ; convergence bookkeeping (flags double-buffered by parity so
// that no block of a launch can observe a flag written by another block of the same launch)
__global__ __launch_bounds__(kRowChunk) void k_pcg_pupdate(BatchView V, int parity, double tol2, int max_iters) {
  __shared__ double s_beta;
  const int g = blockIdx.y;
  int* done_in = V.pcg_done + parity * V.B;
  int* done_out = V.pcg_done + (parity ^ 1) * V.B;
  if (done_in[g]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) done_out[g] = 1;
    return;
  }
  const GraphSeg sg = V.seg[g];
  if (blockIdx.x * kRowChunk >= sg.nprow * 6 + sg.nlrow * 3) return;
  if (threadIdx.x < 64) {
    const int n = row_chunks(sg);
    const double rzn = wave_sum_partials(V.part_b + (size_t)g * V.maxRowChunks, n);
    const double rr = wave_sum_partials(V.part_c + (size_t)g * V.maxRowChunks, n);
    if (threadIdx.x == 0) {
      const double rzo = V.rz[parity * V.B + g];
      s_beta = rzn / rzo;
      if (blockIdx.x == 0) {
        V.rz[(parity ^ 1) * V.B + g] = rzn;
        LmState& S = V.lm[g];
        S.pcg_iters += 1;
        int d = 0;
        if (!(rr > tol2 * V.bb[g])) d = 1;                 // converged (or NaN)
        if (!isfinite(rr) || !isfinite(rzn) || !(rzn > 0)) { d = 1; if (!(rr <= tol2 * V.bb[g])) V.pcg_fail[g] = 1; }
        done_out[g] = d;
      }
    }
  }
  __syncthreads();
  const double beta = s_beta;
  const RowRef R = row_ref(V, sg, blockIdx.x * kRowChunk + threadIdx.x);
  if (R.valid) V.p[R.xoff] = V.z[R.xoff] + beta * V.p[R.xoff];
}

__global__ void k_pcg_alldone(BatchView V, int parity) {
  // one workgroup; flags[1] = 1 iff every graph's PCG is finished
  __shared__ int s_any;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  for (int g = threadIdx.x; g < V.B; g += blockDim.x)
    if (!V.pcg_done[parity * V.B + g]) s_any = 1;
  __syncthreads();
  if (threadIdx.x == 0) V.flags[1] = s_any ? 0 : 1;
}

// trial estimate = current [+] dx  (VertexSE3 / VertexPointXYZ / VertexPlane oplus)
__global__ __launch_bounds__(256) void k_oplus(BatchView V, const double* __restrict__ dx) { oplus_row(V, blockIdx.x * blockDim.x + threadIdx.x, dx); }

// partial sums of dx . (lambda dx + b)   (denominator of the LM gain ratio)
__global__ __launch_bounds__(kRowChunk) void k_scale(BatchView V, const double* __restrict__ dx) {
  __shared__ double red[kRowChunk / 64];
  const int g = blockIdx.y;
  if (!V.lm[g].in_trial) return;
  const GraphSeg sg = V.seg[g];
  if (blockIdx.x * kRowChunk >= sg.nprow * 6 + sg.nlrow * 3) return;
  const RowRef R = row_ref(V, sg, blockIdx.x * kRowChunk + threadIdx.x);
  double v = 0;
  if (R.valid) { const double d = dx[R.xoff]; v = d * (V.lm[g].lambda * d + V.bvec[R.xoff]); }
  const double s = block_sum<kRowChunk>(v, red);
  if (threadIdx.x == 0) V.part_a[(size_t)g * V.maxRowChunks + blockIdx.x] = s;
}

// g2o OptimizationAlgorithmLevenberg accept / reject, one wave per graph
__global__ void k_lm_control(BatchView V, const double* __restrict__ part_chi, int max_iters) {
  const int g = blockIdx.x;
  LmState& S = V.lm[g];
  if (!S.in_trial) return;
  const double tchi = wave_sum_partials(part_chi + (size_t)g * V.maxEdgeChunks, edge_chunks(V.seg[g]));
  const double sc = wave_sum_partials(V.part_a + (size_t)g * V.maxRowChunks, row_chunks(V.seg[g]));
  if (threadIdx.x != 0) return;
  lm_control_apply(S, tchi, sc, V.pcg_fail[g], max_iters);
}

// an accepted trial becomes the estimate (commit_row for every block row): four lanes per pose (64 B with its pad), two per landmark (32 B),
// 16 bytes each -- a wave moves 1 KB of consecutive bytes per instruction (one thread per row with seven 8-byte loads 64 B apart ran at
// 1.7 TB/s: 0.21 ms of the 512-graph step)
__global__ __launch_bounds__(256) void k_commit(BatchView V) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 4 * V.nPr) {
    const int r = t >> 2, q = t & 3;
    if (!V.lm[V.prow_graph[r]].accept) return;
    const size_t pi = (size_t)V.prow_pose[r];
    reinterpret_cast<D2*>(V.pose + pi * 8)[q] = reinterpret_cast<const D2*>(V.pose_trial + pi * 8)[q];
  } else if (t < 4 * V.nPr + 2 * V.nLr) {
    const int u = t - 4 * V.nPr, l = u >> 1, q = u & 1;
    if (!V.lm[V.lrow_graph[l]].accept) return;
    const size_t li = (size_t)V.lrow_lm[l];
    reinterpret_cast<D2*>(V.lmk + li * 4)[q] = reinterpret_cast<const D2*>(V.lmk_trial + li * 4)[q];
  }
}
__global__ void k_set_trial_all(BatchView V, double lambda) {  // used by the solve() hook
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < V.B) { V.lm[g].in_trial = 1; V.lm[g].lambda = lambda; V.lm[g].active = 1; }
}
__global__ void k_set_trial_each(BatchView V, const double* __restrict__ lambda) {  // sslam_batch_solve: every graph its own damping; lambda < 0: the graph sits out
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < V.B) { const int on = lambda[g] >= 0 ? 1 : 0; V.lm[g].in_trial = on; V.lm[g].lambda = on ? lambda[g] : 0.0; V.lm[g].active = on; }
}

}  // namespace sslam

// =============================================================================================
// Host engine
// =============================================================================================
namespace sslam {

// RCCL is bound with dlopen when the edge-sharded mode is first used, not at link time: a host program that already carries its
// own copy (PyTorch ships one) must end up with ONE librccl in the process, and the single-GPU path must not depend on it at all.
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok() const { return lib && GetUniqueId && CommInitRank && CommDestroy && AllReduce && GetErrorString; }
};
static RcclApi& rccl_api() {
  static RcclApi api;
  if (!api.lib) {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);   // an already loaded copy with this soname is reused
      if (api.lib) break;
    }
    if (api.lib) {
      api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
      api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
      api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce");
      api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    }
  }
  return api;
}
void batch_comm_destroy(void* comm) { if (comm && rccl_api().ok()) (void)rccl_api().CommDestroy((ncclComm_t)comm); }

std::string& last_error_ref() {
  static thread_local std::string e;
  return e;
}

// A host table -> the device array behind a BatchView field (out of the handle's arena, where it travels with the one flush below, or an
// allocation and copy of its own).  T and U differ in name only (std::array<int, 4> on the host, int4 on the device).
template <class T, class U>
static int upload_table(Batch& b, const std::vector<T>& h, const U*& field) {
  static_assert(sizeof(T) == sizeof(U), "host and device records must have one layout");
  T* p = nullptr;
  const int rc = dev_upload(b, h, &p);
  field = reinterpret_cast<const U*>(p);
  return rc;
}

// The tables of batch_compile -> device, the work arrays of the solvers next to them, BatchView filled in; one flush.
static int batch_upload(Batch& b, BatchTables&& T) {
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  if (!b.stream) SSLAM_HIP_TRY(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
  const EdgeClassTab &EO = T.cls[EC_SE3], &EL = T.cls[EC_LANDMARK], &ELL = T.cls[EC_POINT_POINT], &EP = T.cls[EC_PRIOR];
  const int B = (int)b.graphs.size(), nPr = T.nPr(), nLr = T.nLr(), maxRow = T.max_row_chunks, maxEdge = T.max_edge_chunks;
  BatchView& V = b.V;
  memset(&V, 0, sizeof V);
  V.B = B; V.nPr = nPr; V.nLr = nLr; V.nPose = (int)T.pose_row.size(); V.nLm = (int)T.lm_row.size();
  V.nEo = EO.n(); V.nEl = EL.n(); V.nEll = ELL.n(); V.nLL = (int)T.llblk.size(); V.nEp = EP.n(); V.nEpRows = (int)T.ep_row.size();
  V.nDupEo = (int)T.dup_eo.size(); V.nDupEl = (int)T.dup_el.size();
  V.maxRowChunks = maxRow; V.maxEdgeChunks = maxEdge;
  V.h_total = T.h_total;
  V.dcs_phi = b.graphs[0]->opt.dcs_phi;
  int rc = 0;
  auto up = [&](const auto& vec, auto& field) { if (!rc) rc = upload_table(b, vec, field); };
  up(T.seg, V.seg); up(T.pose_row, V.pose_row); up(T.lm_row, V.lm_row); up(T.prow_pose, V.prow_pose); up(T.lrow_lm, V.lrow_lm);
  up(T.prow_graph, V.prow_graph); up(T.lrow_graph, V.lrow_graph); up(T.lm_kind, V.lm_kind); up(T.prow_perm, V.prow_perm);
  up(EO.a, V.eo_i); up(EO.b, V.eo_j); up(EO.z, V.eo_z); up(EO.w, V.eo_w); up(EO.blk, V.eo_blk); up(EO.id, V.eo_id);
  up(EL.a, V.el_p); up(EL.b, V.el_l); up(EL.z, V.el_z); up(EL.w, V.el_w); up(EL.blk, V.el_blk); up(EL.id, V.el_id);
  up(ELL.a, V.ell_a); up(ELL.b, V.ell_b); up(ELL.z, V.ell_z); up(ELL.w, V.ell_w); up(ELL.id, V.ell_id);
  up(T.adj_ptr, V.adj_ptr); up(T.adj_blk, V.adj_blk); up(T.adj_x, V.adj_x); up(T.adj_fmt, V.adj_fmt);
  up(T.pslot_ptr, V.pslot_ptr); up(T.pslot_rec, V.pslot_rec); up(T.lslot_ptr, V.lslot_ptr); up(T.lslot_edge, V.lslot_edge);
  up(T.llslot_ptr, V.llslot_ptr); up(T.llslot_rec, V.llslot_rec); up(T.llblk_ptr, V.llblk_ptr); up(T.llblk_edge, V.llblk_edge);
  up(T.dup_eo, V.dup_eo); up(T.dup_el, V.dup_el); up(T.shard_lo, V.shard_lo); up(T.shard_hi, V.shard_hi);
  if (EP.n() > 0) {   // a batch without priors uploads nothing for them
    up(EP.a, V.ep_pose); up(EP.dim, V.ep_dim); up(EP.z, V.ep_z); up(EP.w, V.ep_w); up(EP.id, V.ep_id);
    up(T.ep_row, V.ep_row); up(T.ep_ptr, V.ep_ptr); up(T.ep_edge, V.ep_edge);
  }
  if (rc) return rc;
  // the system and the work vectors of the solvers (zero-filled)
  auto alloc = [&](size_t n, auto& p) { if (!rc) rc = dev_alloc(b, n, &p); };
  double* H = nullptr;
  const size_t dim = (size_t)6 * nPr + (size_t)3 * nLr;
  const size_t h_even = ((size_t)T.h_total + 1) & ~(size_t)1;   // b right behind H (16-byte aligned): [H || b] is one all-reduce buffer
  alloc(h_even + dim, H);
  if (T.has_planes) alloc((size_t)std::max(V.nEl, 1) * kPjDoubles, V.pj);
  alloc((size_t)V.nPose * 8, V.pose); alloc((size_t)V.nPose * 8, V.pose_trial); alloc((size_t)V.nLm * 4, V.lmk); alloc((size_t)V.nLm * 4, V.lmk_trial);
  alloc(dim, V.x); alloc(dim, V.r); alloc(dim, V.z); alloc(dim, V.p); alloc(dim, V.q);
  alloc((size_t)nPr * 36 + (size_t)nLr * 9, V.Minv);
  alloc((size_t)B * maxRow, V.part_a); alloc((size_t)B * maxRow, V.part_b); alloc((size_t)B * maxRow, V.part_c);
  alloc((size_t)B * maxRow, b.d_part_m); alloc((size_t)B * maxEdge, b.d_part_e);
  alloc((size_t)2 * B, V.rz); alloc((size_t)B, V.bb); alloc((size_t)2 * B, V.pcg_done); alloc((size_t)B, V.pcg_fail); alloc((size_t)4, V.flags);
  alloc((size_t)B, V.lm);
  if (rc) return rc;
  V.Hpp_diag = H; V.Hll_diag = H + T.hll_base; V.Hpp_off = H + T.hpp_off_base; V.Hpl = H + T.hpl_base; V.Hll_off = H + T.hll_off_base;
  V.bvec = H + h_even;
  b.hb_doubles = (int64_t)(h_even + dim);
  if (b.arena && b.arena->flush(b.stream)) return set_error(SSLAM_ERR_HIP, "upload of the batch tables failed");
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  b.T = std::move(static_cast<BatchMaps&>(T));   // the batch keeps the host's part; the rest is on the device now
  b.versions.resize(B);
  for (int g = 0; g < B; ++g) b.versions[g] = b.graphs[g]->structure_version;
  b.uploaded = false;
  b.robust_synced = false; b.has_robust = false;
  return 0;
}

// batch_compile, and the one thing it cannot express: H is addressed with int32 block offsets
static int batch_compile_checked(const std::vector<HostGraph*>& graphs, BatchTables& T) {
  T = batch_compile(graphs);
  if (T.h_total >= (int64_t)1 << 31) return set_error(SSLAM_ERR_INVALID, "batch too large: H has %lld doubles (int32 block offsets)", (long long)T.h_total);
  return 0;
}
static int batch_build(Batch& b) {
  BatchTables T;
  if (const int rc = batch_compile_checked(b.graphs, T)) return rc;
  return batch_upload(b, std::move(T));
}

// Per-edge robust kernels are edge data: when a graph's kernels changed since this batch last looked (robust_version), the kind / delta arrays
// of the four edge classes are written again -- no table, no plan, no structure is touched.  A batch none of whose edges has a kernel holds
// null pointers and runs the <RK = false> kernels.  Their memory does not come from a handle's arena (whose blocks travel with one flush at
// build time): a kernel may arrive long after the batch was built.
static int batch_sync_robust(Batch& b) {
  uint64_t ver = 0;
  int any = 0;
  for (const HostGraph* G : b.graphs) { ver += G->robust_version; any += G->n_robust; }
  if (b.robust_synced && ver == b.robust_ver) return 0;
  BatchView& V = b.V;
  if (any) {
    // device order is class order: by graph, then by edge id (batch_tables.hpp)
    std::vector<unsigned char> kind[kEdgeClasses];
    std::vector<double> delta[kEdgeClasses];
    for (const HostGraph* G : b.graphs)
      for (int k = 0; k < G->ne(); ++k) { const int c = kEdgeType[G->etype[k]].cls; kind[c].push_back(G->rk_kind[k]); delta[c].push_back(G->rk_delta[k]); }
    for (int c = 0; c < kEdgeClasses; ++c) {
      if (kind[c].empty()) { kind[c].push_back(0); delta[c].push_back(0.0); }
      if (!b.d_rk[c]) {
        void* p = nullptr;
        SSLAM_HIP_TRY(hipMalloc(&p, kind[c].size())); b.allocs.push_back(p); b.d_rk[c] = (unsigned char*)p;
        SSLAM_HIP_TRY(hipMalloc(&p, delta[c].size() * sizeof(double))); b.allocs.push_back(p); b.d_rd[c] = (double*)p;
      }
      SSLAM_HIP_TRY(hipMemcpyAsync(b.d_rk[c], kind[c].data(), kind[c].size(), hipMemcpyHostToDevice, b.stream));
      SSLAM_HIP_TRY(hipMemcpyAsync(b.d_rd[c], delta[c].data(), delta[c].size() * sizeof(double), hipMemcpyHostToDevice, b.stream));
    }
    SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));   // (the host vectors go out of scope)
    V.eo_rk = b.d_rk[EC_SE3]; V.el_rk = b.d_rk[EC_LANDMARK]; V.ell_rk = b.d_rk[EC_POINT_POINT]; V.ep_rk = b.d_rk[EC_PRIOR];
    V.eo_rd = b.d_rd[EC_SE3]; V.el_rd = b.d_rd[EC_LANDMARK]; V.ell_rd = b.d_rd[EC_POINT_POINT]; V.ep_rd = b.d_rd[EC_PRIOR];
  } else {
    V.eo_rk = V.el_rk = V.ell_rk = V.ep_rk = nullptr;
    V.eo_rd = V.el_rd = V.ell_rd = V.ep_rd = nullptr;
  }
  b.has_robust = any != 0;
  b.robust_ver = ver; b.robust_synced = true;
  return 0;
}

static int batch_upload_estimates(Batch& b) {
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  if (int rc = batch_sync_robust(b)) return rc;
  const size_t np = (size_t)b.V.nPose * 8, nl = (size_t)b.V.nLm * 4;
  std::vector<double> fallback;
  double* stage = reinterpret_cast<double*>(b.pin->get((np + nl) * sizeof(double)));   // page-locked: four asynchronous copies, no staged blits
  if (!stage) { fallback.assign(np + nl, 0.0); stage = fallback.data(); }
  std::fill(stage, stage + np + nl, 0.0);
  double* pose = stage; double* lmk = stage + np;
  for (size_t g = 0; g < b.graphs.size(); ++g) {
    const HostGraph& G = *b.graphs[g];
    for (int v = 0; v < G.nv(); ++v) {
      const double* e = &G.est[(size_t)v * 7];
      if (G.vtype[v] == VT_SE3) { double* o = &pose[(size_t)b.T.v2pose[g][v] * 8]; for (int k = 0; k < 7; ++k) o[k] = e[k]; }
      else { double* o = &lmk[(size_t)b.T.v2lm[g][v] * 4]; for (int k = 0; k < (G.vtype[v] == VT_POINT ? 3 : 4); ++k) o[k] = e[k]; }
    }
  }
  if (np) {
    SSLAM_HIP_TRY(hipMemcpyAsync(b.V.pose, pose, np * 8, hipMemcpyHostToDevice, b.stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(b.V.pose_trial, pose, np * 8, hipMemcpyHostToDevice, b.stream));
  }
  if (nl) {
    SSLAM_HIP_TRY(hipMemcpyAsync(b.V.lmk, lmk, nl * 8, hipMemcpyHostToDevice, b.stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(b.V.lmk_trial, lmk, nl * 8, hipMemcpyHostToDevice, b.stream));
  }
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  b.uploaded = true;
  return 0;
}

static int batch_download_estimates(Batch& b) {
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  const size_t np = (size_t)b.V.nPose * 8, nl = (size_t)b.V.nLm * 4;
  std::vector<double> fallback;
  double* stage = reinterpret_cast<double*>(b.pin->get((np + nl) * sizeof(double)));
  if (!stage) { fallback.assign(np + nl, 0.0); stage = fallback.data(); }
  double* pose = stage; double* lmk = stage + np;
  if (np) SSLAM_HIP_TRY(hipMemcpyAsync(pose, b.V.pose, np * 8, hipMemcpyDeviceToHost, b.stream));
  if (nl) SSLAM_HIP_TRY(hipMemcpyAsync(lmk, b.V.lmk, nl * 8, hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  for (size_t g = 0; g < b.graphs.size(); ++g) {
    HostGraph& G = *b.graphs[g];
    for (int v = 0; v < G.nv(); ++v) {
      double* e = &G.est[(size_t)v * 7];
      if (G.vtype[v] == VT_SE3) { const double* o = &pose[(size_t)b.T.v2pose[g][v] * 8]; for (int k = 0; k < 7; ++k) e[k] = o[k]; }
      else { const double* o = &lmk[(size_t)b.T.v2lm[g][v] * 4]; for (int k = 0; k < (G.vtype[v] == VT_POINT ? 3 : 4); ++k) e[k] = o[k]; }
    }
  }
  return 0;
}

// a few device bytes -> host through the batch's page-locked staging buffer; synchronises the stream
static int read_device(Batch& b, void* host, const void* dev, size_t bytes) {
  char* stage = b.pin->get(bytes);
  SSLAM_HIP_TRY(hipMemcpyAsync(stage ? (void*)stage : host, dev, bytes, hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  if (stage) memcpy(host, stage, bytes);
  return 0;
}

static inline dim3 row_grid(const Batch& b) { return dim3(b.V.maxRowChunks, b.V.B); }
static inline dim3 edge_grid(const Batch& b) { return dim3(b.V.maxEdgeChunks, b.V.B); }
static inline int vert_blocks(const Batch& b) { return std::max(1, (b.V.nPr + b.V.nLr + 255) / 256); }

static int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(SSLAM_ERR_HIP, "launch %s: %s", what, hipGetErrorString(e));
  return 0;
}

// f(std::bool_constant<v>) for a run-time bool: how a launch picks a kernel's bool template arguments
template <class F>
static void with_bool(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }

// The launches of one linearisation into the H and b arrays of V.  PL: the batch holds plane landmarks; SHARD: edge-sharded mode; RK: the
// batch carries per-edge robust kernels.  Stream order matters: the priors and the duplicates add onto what the row kernels wrote.
template <bool PL, bool SHARD, bool RK>
static void launch_linearize(Batch& b, const BatchView& V) {
  if (PL && V.nEl > 0) {
    const long long bA = ((long long)V.nEl * 14 + 255) / 256, bB = ((long long)V.nEl * 6 + 255) / 256;
    hipLaunchKernelGGL(k_plane_jacobians, dim3((unsigned)(bA + bB)), dim3(256), 0, b.stream, V, (int)bA);
  }
  if (V.nPr > 0) hipLaunchKernelGGL((k_linearize_rowthread<PL, SHARD, RK>), dim3((V.nPr + kRowThreads - 1) / kRowThreads), dim3(kRowThreads), 0, b.stream, V);
  if (V.nEpRows > 0) hipLaunchKernelGGL((k_linearize_priors<SHARD, RK>), dim3((V.nEpRows + 63) / 64), dim3(64), 0, b.stream, V);
  if (V.nLr > 0) hipLaunchKernelGGL((k_linearize_lm_rows<PL, SHARD, RK>), dim3((V.nLr + 15) / 16), dim3(256), 0, b.stream, V);
  if (V.nLL > 0) hipLaunchKernelGGL((k_linearize_ll<SHARD, RK>), dim3((V.nLL + 63) / 64), dim3(64), 0, b.stream, V);
  if (V.nDupEo + V.nDupEl > 0) hipLaunchKernelGGL((k_linearize_dups<SHARD, RK>), dim3((std::max(V.nDupEo, V.nDupEl) + 63) / 64), dim3(64), 0, b.stream, V);
}

// BlockSolver::buildSystem for the active graphs of the batch
static int batch_linearize(Batch& b) {
  ScopedTimer t(b, "linearize");
  b.V.dcs_phi = b.graphs[0]->opt.dcs_phi;   // read live like pcg_tol / solver: an option set after the batch was built must not be ignored
  const BatchView& V = b.V;
  const auto launch = [&](auto sh, const BatchView& Vl) {
    with_bool(b.T.has_planes, [&](auto pl) {
      with_bool(b.has_robust, [&](auto rk) { launch_linearize<decltype(pl)::value, decltype(sh)::value, decltype(rk)::value>(b, Vl); });
    });
  };
  if (!b.sharded) {
    launch(std::false_type{}, V);
    return launch_check("linearize");
  }
  // edge-sharded mode: the rank-partial system is built in its own buffer and summed OUT OF PLACE into [H || b].  A graph that does not
  // re-linearise in this step (a rejected trial being retried, a finished graph) keeps its old partial system there, so the sum over
  // ranks is again the system it already had: the all-reduce is idempotent for it.  (Summing in place would multiply the H of such a
  // graph by `world` on every step: the damping of a retried trial would fall instead of rising.)
  BatchView Vp = V;
  Vp.Hpp_diag = b.d_hb_part; Vp.Hll_diag = b.d_hb_part + b.T.hll_base; Vp.Hpp_off = b.d_hb_part + b.T.hpp_off_base;
  Vp.Hpl = b.d_hb_part + b.T.hpl_base; Vp.Hll_off = b.d_hb_part + b.T.hll_off_base; Vp.bvec = b.d_hb_part + (V.bvec - V.Hpp_diag);
  launch(std::true_type{}, Vp);
  if (b.comm) {
    // the partial [H || b] arrays of all ranks -> their sum on every rank: ONE all-reduce over xGMI (RCCL), in stream order;
    // everything after it (solve, update, chi2, LM control) runs replicated and bit-identical on all ranks
    const ncclResult_t r = rccl_api().AllReduce(b.d_hb_part, V.Hpp_diag, (size_t)b.hb_doubles, ncclDouble, ncclSum, (ncclComm_t)b.comm, b.stream);
    if (r != ncclSuccess) return set_error(SSLAM_ERR_HIP, "ncclAllReduce of the normal equations: %s", rccl_api().GetErrorString(r));
    b.allreduce_calls++;
  } else {   // no communicator (single-device parity hook): the partial system is what the caller reads
    SSLAM_HIP_TRY(hipMemcpyAsync(V.Hpp_diag, b.d_hb_part, (size_t)b.hb_doubles * sizeof(double), hipMemcpyDeviceToDevice, b.stream));
  }
  return launch_check("linearize");
}

static int pcg_solve(Batch& b) {
  const Options& opt = b.graphs[0]->opt;
  const BatchView& V = b.V;
  if (opt.solver == 2 && V.nLL > 0)
    return set_error(SSLAM_ERR_UNSUPPORTED, "solver 2 (Schur complement on the landmark block) needs a block-diagonal landmark block: the graph holds point-point edges");
  { ScopedTimer t(b, "precond");
    hipLaunchKernelGGL(k_precond, dim3(vert_blocks(b)), dim3(256), 0, b.stream, V); }
  const bool schur = opt.solver == 2;
  const dim3 lm_grid((V.nLr + V.nPr + 255) / 256);
  if (schur) {   // reduced right-hand side  b_p - Hpl (Hll + lambda I)^-1 b_l  through one SpMV
    hipLaunchKernelGGL(k_pcg_reset, dim3((V.B + 63) / 64), dim3(64), 0, b.stream, V);
    hipLaunchKernelGGL(k_schur_lm, lm_grid, dim3(256), 0, b.stream, V, V.p, 1, 0);
    hipLaunchKernelGGL(k_spmv, row_grid(b), dim3(kRowChunk), 0, b.stream, V, 0);
  }
  hipLaunchKernelGGL(k_pcg_init, row_grid(b), dim3(kRowChunk), 0, b.stream, V, schur ? 1 : 0);
  hipLaunchKernelGGL(k_pcg_init2, dim3(V.B), dim3(64), 0, b.stream, V);
  const double tol2 = opt.pcg_tol * opt.pcg_tol;
  int it = 0;
  const int check_every = 32;
  while (it < opt.pcg_max_iters) {
    for (int k = 0; k < check_every && it < opt.pcg_max_iters; ++k, ++it) {
      const int parity = it & 1;
      if (schur) hipLaunchKernelGGL(k_schur_lm, lm_grid, dim3(256), 0, b.stream, V, V.p, 0, parity);
      { ScopedTimer t(b, "spmv");
        hipLaunchKernelGGL(k_spmv, row_grid(b), dim3(kRowChunk), 0, b.stream, V, parity); }
      { ScopedTimer t(b, "pcg_update");
        hipLaunchKernelGGL(k_pcg_update, row_grid(b), dim3(kRowChunk), 0, b.stream, V, parity);
        hipLaunchKernelGGL(k_pcg_pupdate, row_grid(b), dim3(kRowChunk), 0, b.stream, V, parity, tol2, opt.pcg_max_iters); }
    }
    hipLaunchKernelGGL(k_pcg_alldone, dim3(1), dim3(256), 0, b.stream, V, it & 1);
    int flag = 0;
    if (int rc2 = read_device(b, &flag, V.flags + 1, sizeof(int))) return rc2;
    b.harvest();
    if (flag) break;
  }
  if (schur) hipLaunchKernelGGL(k_schur_lm, lm_grid, dim3(256), 0, b.stream, V, V.x, 2, 0);
  return launch_check("pcg");
}

static int batch_solve(Batch& b) {
  // (H + lambda I) dx = b for every graph with in_trial set; result in V.x
  if (b.graphs[0]->opt.solver == 0 || b.graphs[0]->opt.solver == 2) return pcg_solve(b);
  int rc;
  if (!b.chol) {
    static const bool timing = getenv("SSLAM_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = chol_plan_build(b))) return rc;
    if (timing) fprintf(stderr, "[timing] cholesky plan build %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  if (chol_plan_flow(b)) return chol_solve_flow(b);
  if ((rc = chol_factor_and_forward(b))) return rc;
  return chol_backward(b);
}

static int batch_chi2(Batch& b, const double* pose, const double* lmk, int mask_mode) {
  ScopedTimer t(b, "chi2");
  b.V.dcs_phi = b.graphs[0]->opt.dcs_phi;
  if (b.has_robust) hipLaunchKernelGGL(k_chi2<true>, edge_grid(b), dim3(kEdgeChunk), 0, b.stream, b.V, pose, lmk, mask_mode, b.d_part_e);
  else hipLaunchKernelGGL(k_chi2<false>, edge_grid(b), dim3(kEdgeChunk), 0, b.stream, b.V, pose, lmk, mask_mode, b.d_part_e);
  return launch_check("chi2");
}

constexpr int kStepChunk = 8;   // LM steps enqueued between two looks at the per-graph state
// the per-graph LM states -> host, through the page-locked staging buffer (synchronises the stream)
// The system at the current estimates: the estimates go up if the device's are stale, every graph gets its chi2 and a fresh LM state, and
// (lin) the undamped H and b are built.
static int batch_system_at_estimates(Batch& b, bool lin = true) {
  int rc;
  if (!b.uploaded && (rc = batch_upload_estimates(b))) return rc;
  if ((rc = batch_chi2(b, b.V.pose, b.V.lmk, 0))) return rc;
  hipLaunchKernelGGL(k_lm_init, dim3(b.V.B), dim3(64), 0, b.stream, b.V, b.d_part_e, 0);
  return lin ? batch_linearize(b) : 0;
}
static int read_lm_state(Batch& b, std::vector<LmState>& st) { return read_device(b, st.data(), b.V.lm, sizeof(LmState) * (size_t)b.V.B); }

static int batch_optimize(Batch& b, int max_iters, sslam_opt_stats* out) {
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  const auto t0 = std::chrono::steady_clock::now();
  const BatchView& V = b.V;
  int rc;
  if (!b.uploaded && (rc = batch_upload_estimates(b))) return rc;
  if ((rc = batch_chi2(b, V.pose, V.lmk, 0))) return rc;
  hipLaunchKernelGGL(k_lm_init, dim3(V.B), dim3(64), 0, b.stream, V, b.d_part_e, 10);
  std::vector<LmState> st(V.B);
  // The LM control flow (accept / reject, retry with a larger lambda, terminate) lives on the device: the host enqueues
  // generic steps in chunks and only looks at the per-graph state between chunks -- no synchronisation per trial.
  // Every graph needs at least (max_iters - iter) more steps; rejected trials add steps, which later chunks supply.
  // Small batches whose plan runs factor + solves in one dependency-driven launch (k_chol_flow): the rest of a damping trial in two more
  // launches (k_lm_begin_small / k_lm_end_small) -- same sums, same order, same results as the stand-alone kernels
  bool flow_steps = false;
  {
    if (b.graphs[0]->opt.fused && b.graphs[0]->opt.solver == 1 && !b.sharded && !b.profiling) {
      if (!b.chol && (rc = chol_plan_build(b))) return rc;
      flow_steps = chol_plan_flow(b);
    }
  }
  // a batch with per-edge robust kernels takes the <RK = true> forms of the persistent kernels, which were compiled apart so that the plain
  // forms stay what they were; should the device hold fewer of them than the grids were sized for, the lanes are left out (the LM halves
  // then run as k_lm_begin_small / k_lm_end_small<RK> around the single-launch solve: chol_lm_step_flow) -- same results, bitwise
  const bool spec_steps = flow_steps && chol_spec_mode(b) && chol_plan_spec(b) && (!b.has_robust || chol_plan_spec_rk(b));
  long long budget = 10LL * std::max(max_iters, 0) + 8;    // hard bound: <= 10 trials per iteration
  int need = max_iters;
  if ((rc = chol_set_active(b, nullptr))) return rc;
  struct CompactGuard { Batch& b; ~CompactGuard() { (void)chol_set_active(b, nullptr); } } compact_guard{b};   // every exit leaves the launches sized for all graphs
  std::vector<char> act(V.B, 1);
  int n_act = V.B;
  static const bool chunk_timing = getenv("SSLAM_TIMING") != nullptr;
  bool looked = false;   // st holds the state after the last enqueued step
  while (need > 0 && budget > 0) {
    const int chunk = (int)std::min<long long>(std::min(need, kStepChunk), budget);
    const auto tq0 = std::chrono::steady_clock::now();
    for (int sidx = 0; sidx < chunk; ++sidx) {
      if ((rc = batch_linearize(b))) return rc;
      if (spec_steps) { if ((rc = chol_lm_step_spec(b, max_iters))) return rc; continue; }
      if (flow_steps) { if ((rc = chol_lm_step_flow(b, max_iters))) return rc; continue; }
      hipLaunchKernelGGL(k_maxdiag, row_grid(b), dim3(kRowChunk), 0, b.stream, V, b.d_part_m);
      hipLaunchKernelGGL(k_lm_begin_step, dim3(V.B), dim3(64), 0, b.stream, V, b.d_part_m);
      if ((rc = batch_solve(b))) return rc;
      { ScopedTimer t(b, "oplus");
        hipLaunchKernelGGL(k_oplus, dim3(vert_blocks(b)), dim3(256), 0, b.stream, V, V.x); }
      if ((rc = batch_chi2(b, V.pose_trial, V.lmk_trial, 1))) return rc;
      hipLaunchKernelGGL(k_scale, row_grid(b), dim3(kRowChunk), 0, b.stream, V, V.x);
      hipLaunchKernelGGL(k_lm_control, dim3(V.B), dim3(64), 0, b.stream, V, b.d_part_e, max_iters);
      hipLaunchKernelGGL(k_commit, dim3(std::max(1, (4 * V.nPr + 2 * V.nLr + 255) / 256)), dim3(256), 0, b.stream, V);
    }
    budget -= chunk;
    const auto tq1 = std::chrono::steady_clock::now();
    if ((rc = read_lm_state(b, st))) return rc;
    looked = true;
    if (chunk_timing && V.B == 1)
      fprintf(stderr, "[timing] LM chunk: %d steps enqueued in %.3f ms, waited %.3f ms more; iteration %d trials %d active %d\n", chunk,
              std::chrono::duration<double, std::milli>(tq1 - tq0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq1).count(),
              st[0].iter, st[0].trials, st[0].active);
    b.harvest();
    need = 0;
    int na = 0;
    for (int g = 0; g < V.B; ++g) {
      act[g] = st[g].active ? 1 : 0; na += act[g];
      if (!st[g].active) continue;
      // a graph in a streak of rejected trials ends its iteration -- at convergence, its optimisation -- after at most 10 - q more of
      // them: enqueue exactly those (g2o's LM ends every optimisation of the orchestrator with ten rejected trials; a full chunk
      // behind each look cost 4-6 idle steps per tick).  An accepted trial in between: the next look supplies more steps.
      // (small batches only: on a large batch every look is a host round trip for all graphs, and short chunks in the endgame cost the
      // 512-graph stream group 12 % -- 25.0k vs 28.5k iterations/s)
      const int streak_left = (V.B < 8 && st[g].in_trial && st[g].q > 0) ? std::max(1, 10 - st[g].q) : kStepChunk;
      need = std::max(need, std::min(max_iters - st[g].iter, streak_left));
    }
    // the graphs that are still iterating only ever shrink: once half of the batch is done, the factor / solve launches are sized
    // for the rest (a retry by three graphs then costs three graphs' pieces, not the dispatch of everybody's)
    static const bool timing = getenv("SSLAM_TIMING") != nullptr;
    if (timing && V.B > 1) fprintf(stderr, "[timing] LM chunk of %d steps done: %d of %d graphs still active, %d more iterations needed\n", chunk, na, V.B, need);
    if (need > 0 && na < n_act && 2 * na <= V.B) {
      const auto tc = std::chrono::steady_clock::now();
      if ((rc = chol_set_active(b, &act))) return rc;
      n_act = na;
      if (timing) fprintf(stderr, "[timing] launches resized for %d active graphs in %.3f ms\n", na, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count());
    }
  }
  if ((rc = chol_set_active(b, nullptr))) return rc;
  if (!looked && (rc = read_lm_state(b, st))) return rc;   // (nothing was enqueued after the loop's last look)
  b.harvest();
  if ((rc = launch_check("optimize"))) return rc;
  if ((rc = chol_flow_check(b))) return rc;
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int worst = 0;
  for (int g = 0; g < V.B; ++g) {
    sslam_opt_stats& o = out[g];
    memset(&o, 0, sizeof o);
    o.iterations = st[g].iter; o.trials = st[g].trials; o.status = st[g].status;
    o.chi2_before = st[g].chi_before; o.chi2_after = st[g].cur_chi; o.lambda = st[g].lambda;
    o.seconds = secs; o.solver_iterations = st[g].pcg_iters;
    if (st[g].status != SSLAM_ERR_TOO_FEW_EDGES && !std::isfinite(st[g].cur_chi)) { o.status = SSLAM_ERR_NUMERIC; worst = SSLAM_ERR_NUMERIC; }
  }
  if (worst) return set_error(worst, "non-finite chi2 after optimisation");
  return 0;
}

}  // namespace sslam

// =============================================================================================
// C-ABI
// =============================================================================================
using namespace sslam;

struct sslam_graph {
  HostGraph g;
  DevArena arena;                // device memory of the batch below, kept across structure rebuilds (declared first: destroyed last)
  PinnedScratch pin;             // page-locked staging of the batch's small copies, kept across rebuilds as well
  hipStream_t stream = nullptr;  // the handle's stream, handed to every batch it builds (a stream create / destroy pair per tick costs more
                                 // than optimising a small graph)
  std::unique_ptr<Batch> batch;  // batch of one, rebuilt when the structure changes
  bool linearized = false;
  ~sslam_graph() {
    batch.reset();               // synchronises the stream
    if (stream) { (void)hipSetDevice(g.device); (void)hipStreamSynchronize(stream); persist_forget_stream(g.device, stream); (void)hipStreamDestroy(stream); }
  }
};
struct sslam_batch {
  Batch b;
  // Stream group (sslam_batch_create_streams): the graphs split into contiguous parts, every part a batch of its own with its own HIP
  // stream, optimised from its own host thread.  A batch marches batch-synchronously through the depths of its graphs' elimination trees
  // and through its LM trial rounds; parts that are out of phase with one another fill the chip while one of them is at the narrow top
  // of its trees or in the LM endgame with a few graphs left.  `b` is unused in a group handle.
  std::vector<sslam_batch*> parts;
  std::vector<int> part0;      // first graph of every part, then n
  ~sslam_batch() { for (sslam_batch* p : parts) delete p; }
};

// run f(part, index) for every part of a group handle, one host thread per part (f = nullptr-safe single batches never come here);
// the first failing part's status and message are handed to the calling thread
template <class F>
static int for_each_part(sslam_batch* h, bool threaded, F f) {
  const int K = (int)h->parts.size();
  std::vector<int> rcs(K, 0);
  std::vector<std::string> errs(K);
  if (threaded) {
    std::vector<std::thread> th;
    for (int k = 0; k < K; ++k)
      th.emplace_back([&, k] { rcs[k] = f(h->parts[k], k); if (rcs[k]) errs[k] = last_error_ref(); });
    for (auto& t : th) t.join();
  } else {
    for (int k = 0; k < K; ++k) { rcs[k] = f(h->parts[k], k); if (rcs[k]) errs[k] = last_error_ref(); }
  }
  for (int k = 0; k < K; ++k) if (rcs[k]) return set_error(rcs[k], "part %d of the stream group: %s", k, errs[k].c_str());
  return 0;
}

static int ensure_batch(sslam_graph* h) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return set_error(SSLAM_ERR_NO_DEVICE, "no HIP device visible (%s); the product has no CPU fallback", hipGetErrorString(e));
  if (h->g.device < 0 || h->g.device >= n) return set_error(SSLAM_ERR_NO_DEVICE, "device %d out of range (%d visible)", h->g.device, n);
  if (!h->batch || h->batch->versions.empty() || h->batch->versions[0] != h->g.structure_version) {
    static const bool timing = getenv("SSLAM_TIMING") != nullptr;
    const auto tr0 = std::chrono::steady_clock::now();
    h->batch.reset();                              // the old batch synchronises its stream; its arrays belong to the arena
    SSLAM_HIP_TRY(hipSetDevice(h->g.device));
    h->arena.reset();
    if (timing) fprintf(stderr, "[timing] rebuild: release of the old batch + arena reset %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count());
    h->batch.reset(new Batch());
    h->batch->arena = &h->arena;
    h->batch->pin = &h->pin;
    h->batch->device = h->g.device;
    if (!h->stream) SSLAM_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->batch->stream = h->stream; h->batch->own_stream = false;
    h->batch->graphs = {&h->g};
    int rc = batch_build(*h->batch);
    if (rc) { h->batch.reset(); return rc; }
    h->linearized = false;
  }
  return 0;
}

extern "C" {

const char* sslam_last_error(void) { return last_error_ref().c_str(); }

int sslam_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// page-locked host memory for buffers that travel to the device asynchronously (the clouds of sslam_seg_submit_batch): a caller that
// does not link HIP itself gets it here
void* sslam_pinned_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
    set_error(SSLAM_ERR_NO_DEVICE, "hipHostMalloc of %zu bytes failed (no HIP device?)", bytes);
    return nullptr;
  }
  return p;
}
void sslam_pinned_free(void* p) { if (p) (void)hipHostFree(p); }

sslam_graph* sslam_graph_create(int device) {
  sslam_graph* h = new sslam_graph();
  h->g.device = device;
  return h;
}
void sslam_graph_destroy(sslam_graph* g) { delete g; }

static int add_vertex(sslam_graph* h, int type, const double* est, int n, int fixed) {
  if (!h || !est) return set_error(SSLAM_ERR_INVALID, "null argument");
  HostGraph& G = h->g;
  const int id = G.nv();
  G.vtype.push_back(type);
  G.vfixed.push_back(fixed);
  for (int k = 0; k < 7; ++k) G.est.push_back(k < n ? est[k] : 0.0);
  G.structure_version++;
  return id;
}
int sslam_graph_add_vertex_se3(sslam_graph* h, const double t_q[7], int fixed) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null graph");
  if (fixed < 0) fixed = (h->g.nv() == 0) ? 1 : 0;  // graph_slam.cpp:109-111
  return add_vertex(h, VT_SE3, t_q, 7, fixed ? 1 : 0);
}
int sslam_graph_add_vertex_point(sslam_graph* h, const double p[3]) { return add_vertex(h, VT_POINT, p, 3, 0); }
int sslam_graph_add_vertex_plane(sslam_graph* h, const double n_d[4]) {
  if (!n_d) return set_error(SSLAM_ERR_INVALID, "null argument");
  const double nn = std::sqrt(n_d[0] * n_d[0] + n_d[1] * n_d[1] + n_d[2] * n_d[2]);
  if (!(nn > 0)) return set_error(SSLAM_ERR_INVALID, "plane normal has zero length");
  const double p[4] = {n_d[0] / nn, n_d[1] / nn, n_d[2] / nn, n_d[3] / nn};  // Plane3D::fromVector normalises
  return add_vertex(h, VT_PLANE, p, 4, 0);
}

// j = -1 for a unary edge (position prior); measurement length, information dimension and vertex types are the type's (kEdgeType)
static int add_edge(sslam_graph* h, int type, int i, int j, const double* z, const double* info) {
  if (!h || !z || !info) return set_error(SSLAM_ERR_INVALID, "null argument");
  HostGraph& G = h->g;
  const EdgeType& et = kEdgeType[type];
  const int nz = et.nz, d = et.d;
  if (et.vt_j < 0) {
    if (i < 0 || i >= G.nv() || j != -1) return set_error(SSLAM_ERR_INVALID, "prior vertex id %d invalid", i);
  } else if (i < 0 || j < 0 || i >= G.nv() || j >= G.nv() || i == j) return set_error(SSLAM_ERR_INVALID, "edge vertex ids (%d,%d) invalid", i, j);
  if (G.vtype[i] != et.vt_i) return set_error(SSLAM_ERR_INVALID, "vertex %d has the wrong type for this edge", i);
  if (et.vt_j >= 0 && G.vtype[j] != et.vt_j) return set_error(SSLAM_ERR_INVALID, "vertex %d has the wrong type for this edge", j);
  // only the upper triangle of the information matrix travels to the device: an asymmetric one would be symmetrised silently
  double amax = 0;
  for (int k = 0; k < d * d; ++k) { if (!std::isfinite(info[k])) return set_error(SSLAM_ERR_INVALID, "information matrix has a non-finite entry"); amax = std::max(amax, std::fabs(info[k])); }
  for (int r = 0; r < d; ++r)
    for (int c = r + 1; c < d; ++c)
      if (std::fabs(info[r * d + c] - info[c * d + r]) > 1e-9 * amax)
        return set_error(SSLAM_ERR_INVALID, "information matrix is not symmetric (entries (%d,%d) and (%d,%d) differ)", r, c, c, r);
  const int id = G.ne();
  G.etype.push_back(type); G.evi.push_back(i); G.evj.push_back(j);
  for (int k = 0; k < 7; ++k) G.meas.push_back(k < nz ? z[k] : 0.0);
  for (int k = 0; k < 36; ++k) G.info.push_back(k < d * d ? info[k] : 0.0);
  G.rk_kind.push_back(0); G.rk_delta.push_back(0.0);
  G.structure_version++;
  return id;
}
int sslam_graph_add_edge_se3(sslam_graph* h, int i, int j, const double z[7], const double info[36]) {
  return add_edge(h, ET_SE3, i, j, z, info);
}
int sslam_graph_add_edge_se3_point(sslam_graph* h, int i, int l, const double z[3], const double info[9]) {
  return add_edge(h, ET_SE3_POINT, i, l, z, info);
}
int sslam_graph_add_edge_se3_plane(sslam_graph* h, int i, int l, const double z[4], const double info[9]) {
  if (!z) return set_error(SSLAM_ERR_INVALID, "null argument");
  const double nn = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  if (!(nn > 0)) return set_error(SSLAM_ERR_INVALID, "plane normal has zero length");
  const double p[4] = {z[0] / nn, z[1] / nn, z[2] / nn, z[3] / nn};
  return add_edge(h, ET_SE3_PLANE, i, l, p, info);
}

int sslam_graph_add_edge_point_point(sslam_graph* h, int l1, int l2, const double z[3], const double info[9]) {
  return add_edge(h, ET_POINT_POINT, l1, l2, z, info);
}

int sslam_graph_add_edge_se3_prior_xyz(sslam_graph* h, int v, const double z[3], const double info[9]) {
  return add_edge(h, ET_SE3_PRIOR_XYZ, v, -1, z, info);
}
int sslam_graph_add_edge_se3_prior_xy(sslam_graph* h, int v, const double z[2], const double info[4]) {
  return add_edge(h, ET_SE3_PRIOR_XY, v, -1, z, info);
}

int sslam_graph_num_vertices(const sslam_graph* h) { return h ? h->g.nv() : SSLAM_ERR_INVALID; }
int sslam_graph_num_edges(const sslam_graph* h) { return h ? h->g.ne() : SSLAM_ERR_INVALID; }

int sslam_graph_get_vertex(const sslam_graph* h, int id, double* out) {
  if (!h || !out || id < 0 || id >= h->g.nv()) return set_error(SSLAM_ERR_INVALID, "bad vertex id %d", id);
  const int n = vertex_est_len(h->g.vtype[id]);
  for (int k = 0; k < n; ++k) out[k] = h->g.est[(size_t)id * 7 + k];
  return n;
}
int sslam_graph_set_vertex(sslam_graph* h, int id, const double* in) {
  if (!h || !in || id < 0 || id >= h->g.nv()) return set_error(SSLAM_ERR_INVALID, "bad vertex id %d", id);
  const int n = vertex_est_len(h->g.vtype[id]);
  for (int k = 0; k < n; ++k) h->g.est[(size_t)id * 7 + k] = in[k];
  if (h->batch) h->batch->uploaded = false;
  h->linearized = false;
  return n;
}
int sslam_graph_hessian_index(sslam_graph* h, int id) {
  if (!h || id < 0 || id >= h->g.nv()) return set_error(SSLAM_ERR_INVALID, "bad vertex id %d", id);
  std::vector<int> hidx;
  hessian_indices(h->g, hidx);
  return hidx[id];
}

int sslam_graph_set_option(sslam_graph* h, const char* key, double value) {
  if (!h || !key) return set_error(SSLAM_ERR_INVALID, "null argument");
  Options& o = h->g.opt;
  const std::string k(key);
  if (k == "solver") { if (value != 0 && value != 1 && value != 2) return set_error(SSLAM_ERR_INVALID, "solver: 0 block-Jacobi PCG, 1 sparse block Cholesky, 2 Schur complement on the landmarks + PCG (3, the window plan of round 3, was removed in round 5: 2-2.7x slower than 1)"); o.solver = (int)value; }
  else if (k == "robust_kernel_dcs") { if (!(value >= 0)) return set_error(SSLAM_ERR_INVALID, "robust_kernel_dcs: phi >= 0 (0 = no kernel)"); o.dcs_phi = value; if (h->batch) h->batch->V.dcs_phi = value; h->linearized = false; }
  else if (k == "fused_small_graph") o.fused = value != 0;
  else if (k == "speculative_trials") o.speculative = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
  else if (k == "pcg_tol") o.pcg_tol = value;
  else if (k == "pcg_max_iters") o.pcg_max_iters = (int)value;
  else if (k == "deterministic") { if (value == 0) return set_error(SSLAM_ERR_UNSUPPORTED, "the Jacobian build is always deterministic (gather form); the FP64-atomics variant was removed"); }
  else return set_error(SSLAM_ERR_INVALID, "unknown option '%s'", key);
  return 0;
}

// ---- per-edge robust kernels ---------------------------------------------------------------------
int sslam_graph_set_edge_robust_kernel(sslam_graph* h, int edge_id, int kind, double delta) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null graph");
  HostGraph& G = h->g;
  if (edge_id < 0 || edge_id >= G.ne()) return set_error(SSLAM_ERR_INVALID, "bad edge id %d", edge_id);
  if (kind < SSLAM_ROBUST_NONE || kind > SSLAM_ROBUST_DCS) return set_error(SSLAM_ERR_INVALID, "robust kernel kind %d: 0 .. 7 (SSLAM_ROBUST_*)", kind);
  if (kind != SSLAM_ROBUST_NONE && !(std::isfinite(delta) && delta > 0)) return set_error(SSLAM_ERR_INVALID, "robust kernel width must be finite and > 0");
  if (kind == SSLAM_ROBUST_NONE) delta = 0.0;
  G.n_robust += (kind != 0) - (G.rk_kind[edge_id] != 0);
  G.rk_kind[edge_id] = (unsigned char)kind; G.rk_delta[edge_id] = delta;
  G.robust_version++;   // a value change: structure_version, the batch tables and the symbolic factorisation stay
  if (h->batch) h->batch->uploaded = false;
  h->linearized = false;
  return 0;
}
int sslam_graph_get_edge_robust_kernel(const sslam_graph* h, int edge_id, int* kind, double* delta) {
  if (!h || edge_id < 0 || edge_id >= h->g.ne()) return set_error(SSLAM_ERR_INVALID, "bad edge id %d", edge_id);
  if (kind) *kind = h->g.rk_kind[edge_id];
  if (delta) *delta = h->g.rk_delta[edge_id];
  return 0;
}
int sslam_graph_edge_chi2(sslam_graph* h, const int* edge_ids, int n, double* e2_out, double* rho0_out, double* weight_out) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null graph");
  const HostGraph& G = h->g;
  if (!edge_ids) n = G.ne();   // all edges, in id order
  if (n < 0) return set_error(SSLAM_ERR_INVALID, "negative edge count");
  if (n == 0) return 0;
  // edge id -> graph-local index in the order of edge_chi2: SE3 edges, landmark edges, point-point edges, priors, each in id order
  std::vector<int> pos(G.ne());
  int cnt[kEdgeClasses] = {}, off[kEdgeClasses] = {};
  auto cls = [&](int k) { return kEdgeType[G.etype[k]].cls; };
  for (int k = 0; k < G.ne(); ++k) pos[k] = cnt[cls(k)]++;
  for (int c = 1; c < kEdgeClasses; ++c) off[c] = off[c - 1] + cnt[c - 1];
  std::vector<int> loc(n);
  for (int t = 0; t < n; ++t) {
    const int k = edge_ids ? edge_ids[t] : t;
    if (k < 0 || k >= G.ne()) return set_error(SSLAM_ERR_INVALID, "bad edge id %d", k);
    loc[t] = off[cls(k)] + pos[k];
  }
  int rc = ensure_batch(h);
  if (rc) return rc;
  Batch& b = *h->batch;
  if ((rc = batch_upload_estimates(b))) return rc;
  b.V.dcs_phi = G.opt.dcs_phi;
  int* d_loc = nullptr; double* d_out = nullptr;
  std::vector<double> out((size_t)3 * n);
  hipError_t e = hipMalloc((void**)&d_loc, (size_t)n * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, out.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpyAsync(d_loc, loc.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, b.stream);
  if (e == hipSuccess) {
    with_bool(b.has_robust, [&](auto rk) { hipLaunchKernelGGL(k_edge_chi2<decltype(rk)::value>, dim3((n + 63) / 64), dim3(64), 0, b.stream, b.V, 0, (const int*)d_loc, n, d_out); });
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, b.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
  if (d_loc) (void)hipFree(d_loc);
  if (d_out) (void)hipFree(d_out);
  if (e != hipSuccess) return set_error(SSLAM_ERR_HIP, "edge chi2: %s", hipGetErrorString(e));
  for (int t = 0; t < n; ++t) {
    if (e2_out) e2_out[t] = out[t];
    if (rho0_out) rho0_out[t] = out[(size_t)n + t];
    if (weight_out) weight_out[t] = out[2 * (size_t)n + t];
  }
  return 0;
}

int sslam_graph_optimize(sslam_graph* h, int max_iters, sslam_opt_stats* out) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null graph");
  sslam_opt_stats local;
  if (!out) out = &local;
  memset(out, 0, sizeof *out);
  if (h->g.ne() < 10) {  // graph_slam.cpp:184-186
    out->status = SSLAM_ERR_TOO_FEW_EDGES;
    return set_error(SSLAM_ERR_TOO_FEW_EDGES, "graph has %d edges (< 10): not optimised", h->g.ne());
  }
  static const bool timing = getenv("SSLAM_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  const bool reuse = h->batch && !h->batch->versions.empty() && h->batch->versions[0] == h->g.structure_version;   // ensure_batch rebuilds otherwise
  if (h->batch) h->batch->plan_build_ms = 0;   // (a call that failed after a rebuild must not leak its plan time into this one: round-5 ADVICE)
  int rc = ensure_batch(h);
  if (rc) { out->status = rc; return rc; }
  const double t1 = now();
  if ((rc = batch_upload_estimates(*h->batch))) return rc;
  const double t2 = now();
  if ((rc = batch_optimize(*h->batch, max_iters, out))) return rc;
  const double t3 = now();
  // what a structure change cost the host: batch tables (ensure_batch) + symbolic factorisation; exactly 0 when the structure was reused
  out->host_plan_us = (reuse && h->batch->plan_build_ms == 0) ? 0 : (int)std::lround(1e3 * ((reuse ? 0.0 : t1 - t0) + h->batch->plan_build_ms));
  h->batch->plan_build_ms = 0;
  h->linearized = false;
  rc = batch_download_estimates(*h->batch);
  if (timing) fprintf(stderr, "[timing] optimize: vertices %d edges %d | structure %.3f upload %.3f LM %.3f (iterations %d trials %d) download %.3f ms\n",
                      h->g.nv(), h->g.ne(), t1 - t0, t2 - t1, t3 - t2, out->iterations, out->trials, now() - t3);
  return rc;
}

int sslam_graph_chi2(sslam_graph* h, double* chi2) {
  if (!h || !chi2) return set_error(SSLAM_ERR_INVALID, "null argument");
  int rc = ensure_batch(h);
  if (rc) return rc;
  Batch& b = *h->batch;
  b.uploaded = false;   // a graph handle's host estimates are the truth: they always go up
  if ((rc = batch_system_at_estimates(b, false))) return rc;
  LmState s;
  if ((rc = read_device(b, &s, b.V.lm, sizeof s))) return rc;
  *chi2 = s.cur_chi;
  return 0;
}

static int do_linearize(sslam_graph* h) {
  int rc = ensure_batch(h);
  if (rc) return rc;
  Batch& b = *h->batch;
  b.uploaded = false;   // as in sslam_graph_chi2
  if ((rc = batch_system_at_estimates(b))) return rc;
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  b.harvest();
  h->linearized = true;
  return 0;
}

int sslam_graph_linearize(sslam_graph* h, int* dim, int64_t* nnz_upper, int32_t* rows, int32_t* cols, double* vals, double* bout) {
  if (!h || !dim || !nnz_upper) return set_error(SSLAM_ERR_INVALID, "null argument");
  int rc = ensure_batch(h);
  if (rc) return rc;
  Batch& b = *h->batch;
  std::vector<int> hidx;
  const int n = hessian_indices(h->g, hidx);
  *dim = n;
  const int nPr = b.V.nPr, nLr = b.V.nLr;
  const int64_t nnz = (int64_t)nPr * 21 + (int64_t)nLr * 6 + (int64_t)b.T.ppoff.size() * 36 + (int64_t)b.T.plblk.size() * 18 + (int64_t)b.T.llblk.size() * 9;
  *nnz_upper = nnz;
  if (!rows || !cols || !vals || !bout) return 0;
  if ((rc = do_linearize(h))) return rc;
  std::vector<double> H((size_t)b.V.h_total), bv((size_t)6 * nPr + (size_t)3 * nLr);
  SSLAM_HIP_TRY(hipMemcpy(H.data(), b.V.Hpp_diag, H.size() * 8, hipMemcpyDeviceToHost));
  SSLAM_HIP_TRY(hipMemcpy(bv.data(), b.V.bvec, bv.size() * 8, hipMemcpyDeviceToHost));
  auto prow_off = [&](int r) { return hidx[b.T.pose_vertex[b.T.prow_pose[r]]]; };
  auto lrow_off = [&](int r) { return hidx[b.T.lm_vertex[b.T.lrow_lm[r]]]; };
  int64_t q = 0;
  auto emit = [&](int R, int C, double v) { if (R > C) std::swap(R, C); rows[q] = R; cols[q] = C; vals[q] = v; ++q; };
  for (int r = 0; r < nPr; ++r) {
    const int o = prow_off(r);
    for (int a = 0; a < 6; ++a) { for (int c = a; c < 6; ++c) emit(o + a, o + c, H[(size_t)r * 36 + a * 6 + c]); bout[o + a] = bv[(size_t)6 * r + a]; }
  }
  for (int r = 0; r < nLr; ++r) {
    const int o = lrow_off(r);
    for (int a = 0; a < 3; ++a) { for (int c = a; c < 3; ++c) emit(o + a, o + c, H[(size_t)b.T.hll_base + (size_t)r * 9 + a * 3 + c]); bout[o + a] = bv[(size_t)6 * nPr + (size_t)3 * r + a]; }
  }
  for (size_t i = 0; i < b.T.ppoff.size(); ++i) {
    const int oa = prow_off(b.T.ppoff[i].first), oc = prow_off(b.T.ppoff[i].second);
    for (int a = 0; a < 6; ++a) for (int c = 0; c < 6; ++c) emit(oa + a, oc + c, H[(size_t)b.T.hpp_off_base + i * 36 + a * 6 + c]);
  }
  for (size_t i = 0; i < b.T.plblk.size(); ++i) {
    const int op = prow_off(b.T.plblk[i].first), ol = lrow_off(b.T.plblk[i].second);
    for (int a = 0; a < 6; ++a) for (int c = 0; c < 3; ++c) emit(op + a, ol + c, H[(size_t)b.T.hpl_base + i * 18 + a * 3 + c]);
  }
  for (size_t i = 0; i < b.T.llblk.size(); ++i) {   // emit() orders (row, column) into the upper triangle; the block is symmetric (-Omega)
    const int oa = lrow_off(b.T.llblk[i].first), oc = lrow_off(b.T.llblk[i].second);
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) {
      const double v = H[(size_t)b.T.hll_off_base + i * 9 + a * 3 + c];
      if (oa < oc) emit(oa + a, oc + c, v); else emit(oc + c, oa + a, v);
    }
  }
  return 0;
}

// internal <-> g2o ordering of the unknown vector
static void to_g2o_order(const sslam_graph* h, const std::vector<double>& xin, double* xout) {
  const Batch& b = *h->batch;
  std::vector<int> hidx;
  hessian_indices(h->g, hidx);
  for (int r = 0; r < b.V.nPr; ++r) { const int o = hidx[b.T.pose_vertex[b.T.prow_pose[r]]]; for (int a = 0; a < 6; ++a) xout[o + a] = xin[(size_t)6 * r + a]; }
  for (int r = 0; r < b.V.nLr; ++r) { const int o = hidx[b.T.lm_vertex[b.T.lrow_lm[r]]]; for (int a = 0; a < 3; ++a) xout[o + a] = xin[(size_t)6 * b.V.nPr + (size_t)3 * r + a]; }
}
static void from_g2o_order(const sslam_graph* h, const double* xin, std::vector<double>& xout) {
  const Batch& b = *h->batch;
  std::vector<int> hidx;
  hessian_indices(h->g, hidx);
  xout.assign((size_t)6 * b.V.nPr + (size_t)3 * b.V.nLr, 0.0);
  for (int r = 0; r < b.V.nPr; ++r) { const int o = hidx[b.T.pose_vertex[b.T.prow_pose[r]]]; for (int a = 0; a < 6; ++a) xout[(size_t)6 * r + a] = xin[o + a]; }
  for (int r = 0; r < b.V.nLr; ++r) { const int o = hidx[b.T.lm_vertex[b.T.lrow_lm[r]]]; for (int a = 0; a < 3; ++a) xout[(size_t)6 * b.V.nPr + (size_t)3 * r + a] = xin[o + a]; }
}

int sslam_graph_solve(sslam_graph* h, double lambda, double* x, int64_t* solver_iterations) {
  if (!h || !x) return set_error(SSLAM_ERR_INVALID, "null argument");
  int rc;
  if (!h->linearized && (rc = do_linearize(h))) return rc;
  Batch& b = *h->batch;
  hipLaunchKernelGGL(k_set_trial_all, dim3((b.V.B + 63) / 64), dim3(64), 0, b.stream, b.V, lambda);
  if ((rc = batch_solve(b))) return rc;
  std::vector<double> xi((size_t)6 * b.V.nPr + (size_t)3 * b.V.nLr);
  LmState s;
  int fail = 0;
  SSLAM_HIP_TRY(hipMemcpyAsync(xi.data(), b.V.x, xi.size() * 8, hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(&s, b.V.lm, sizeof s, hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(&fail, b.V.pcg_fail, sizeof fail, hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  if (solver_iterations) *solver_iterations = s.pcg_iters;
  to_g2o_order(h, xi, x);
  if ((rc = chol_flow_check(b))) return rc;   // a dependency wait of the single-launch solve that gave up (also raises `fail`)
  if (fail) return set_error(SSLAM_ERR_NUMERIC, "linear solve broke down");
  return 0;
}

int sslam_graph_oplus(sslam_graph* h, const double* dx) {
  if (!h || !dx) return set_error(SSLAM_ERR_INVALID, "null argument");
  int rc = ensure_batch(h);
  if (rc) return rc;
  Batch& b = *h->batch;
  if ((rc = batch_upload_estimates(b))) return rc;
  std::vector<double> xi;
  from_g2o_order(h, dx, xi);
  if (!xi.empty()) SSLAM_HIP_TRY(hipMemcpyAsync(b.V.x, xi.data(), xi.size() * 8, hipMemcpyHostToDevice, b.stream));
  hipLaunchKernelGGL(k_set_trial_all, dim3((b.V.B + 63) / 64), dim3(64), 0, b.stream, b.V, 0.0);
  hipLaunchKernelGGL(k_oplus, dim3(vert_blocks(b)), dim3(256), 0, b.stream, b.V, b.V.x);
  if (b.V.nPose) SSLAM_HIP_TRY(hipMemcpyAsync(b.V.pose, b.V.pose_trial, (size_t)b.V.nPose * 64, hipMemcpyDeviceToDevice, b.stream));
  if (b.V.nLm) SSLAM_HIP_TRY(hipMemcpyAsync(b.V.lmk, b.V.lmk_trial, (size_t)b.V.nLm * 32, hipMemcpyDeviceToDevice, b.stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  h->linearized = false;
  return batch_download_estimates(b);
}

// First unknown of vertex v of graph g in the batch's internal row order, -1: fixed or without edges.
static int vertex_xoff(const Batch& b, int g, int v) {
  if (b.graphs[g]->vtype[v] == VT_SE3) { const int r = b.T.pose_row[b.T.v2pose[g][v]]; return r < 0 ? -1 : 6 * r; }
  const int r = b.T.lm_row[b.T.v2lm[g][v]];
  return r < 0 ? -1 : 6 * b.V.nPr + 3 * r;
}

// The requests of chol_marginal_blocks for n (graph, row vertex, column vertex) triples at(k); slot[k]: the triple's place among them, -1:
// an end is fixed or without edges (its block is zeros, nothing is asked).
static std::vector<MarginalReq> marginal_requests(const Batch& b, size_t n, const std::function<std::array<int, 3>(size_t)>& at, std::vector<int>& slot) {
  std::vector<MarginalReq> mr;
  slot.assign(n, -1);
  for (size_t k = 0; k < n; ++k) {
    const std::array<int, 3> q = at(k);
    const int g = q[0], xr = vertex_xoff(b, g, q[1]), xc = vertex_xoff(b, g, q[2]);
    if (xr < 0 || xc < 0) continue;
    slot[k] = (int)mr.size();
    mr.push_back({xr, vertex_dim(b.graphs[g]->vtype[q[1]]), xc, vertex_dim(b.graphs[g]->vtype[q[2]])});
  }
  return mr;
}

// The flat factor of the undamped H of every graph of a linearised batch, what chol_marginal_blocks reads: through the single launch
// where the plan has one, else the launches per depth.  *bad: the first graph whose H is not positive definite, -1: none.
static int factor_undamped_flat(Batch& b, int* bad) {
  int rc;
  hipLaunchKernelGGL(k_set_trial_all, dim3((b.V.B + 63) / 64), dim3(64), 0, b.stream, b.V, 0.0);
  if (!b.chol && (rc = chol_plan_build(b))) return rc;
  if ((rc = chol_plan_flow(b) ? chol_factor_flat_flow(b) : chol_factor_and_forward(b, /*flat=*/true))) return rc;
  std::vector<int> fail((size_t)b.V.B, 0);
  if ((rc = read_device(b, fail.data(), b.V.pcg_fail, fail.size() * sizeof(int)))) return rc;
  if ((rc = chol_flow_check(b))) return rc;
  *bad = -1;
  for (int g = b.V.B - 1; g >= 0; --g) if (fail[g]) *bad = g;
  return 0;
}

// Blocks (row vertex vr, column vertex vc) of H^-1 at the current linearisation.  Direct solvers: the undamped H is factored once, then one
// wave per pair walks the elimination-tree paths of its two vertices (chol_marginal_blocks) -- no right-hand side matrix, no backward
// solve, and only the requested blocks cross PCIe.  PCG: the columns of H^-1 that belong to the requested column vertices are solved for
// one by one and the requested row blocks are read out of them.
// out: packed row-major d(vr) x d(vc) blocks, zeros for fixed / edge-less vertices.
static int marginal_blocks(sslam_graph* h, const std::vector<std::pair<int, int>>& pairs, double* out) {
  int rc;
  if ((rc = do_linearize(h))) return rc;  // undamped H at the current estimates
  Batch& b = *h->batch;
  for (auto& pr : pairs)
    if (pr.first < 0 || pr.first >= h->g.nv() || pr.second < 0 || pr.second >= h->g.nv()) return set_error(SSLAM_ERR_INVALID, "bad vertex id (%d, %d)", pr.first, pr.second);
  if (h->g.opt.solver != 0) {
    int bad;
    if ((rc = factor_undamped_flat(b, &bad))) return rc;
    if (bad >= 0) return set_error(SSLAM_ERR_NUMERIC, "H is not positive definite: no marginals");
    std::vector<int> slot;
    const std::vector<MarginalReq> mr = marginal_requests(b, pairs.size(), [&](size_t k) { return std::array<int, 3>{0, pairs[k].first, pairs[k].second}; }, slot);
    std::vector<double> Z(mr.size() * 36 + 1);
    if ((rc = chol_marginal_blocks(b, mr, Z.data()))) return rc;
    size_t o = 0;
    for (size_t k = 0; k < pairs.size(); ++k) {
      const int n = vertex_dim(h->g.vtype[pairs[k].first]) * vertex_dim(h->g.vtype[pairs[k].second]);
      for (int e = 0; e < n; ++e) out[o + e] = slot[k] < 0 ? 0.0 : Z[(size_t)slot[k] * 36 + e];
      o += (size_t)n;
    }
    return 0;
  }
  std::vector<int> hidx;
  const int dim = hessian_indices(h->g, hidx);
  // unique column vertices, their scalar columns
  std::vector<int> colv;
  for (auto& pr : pairs) if (hidx[pr.second] >= 0 && hidx[pr.first] >= 0) colv.push_back(pr.second);
  std::sort(colv.begin(), colv.end());
  colv.erase(std::unique(colv.begin(), colv.end()), colv.end());
  std::vector<int> col0(h->g.nv(), -1);   // first scalar column of a column vertex in X
  int nrhs = 0;
  for (int v : colv) { col0[v] = nrhs; nrhs += vertex_dim(h->g.vtype[v]); }
  const size_t idim = (size_t)6 * b.V.nPr + (size_t)3 * b.V.nLr;
  std::vector<double> X((size_t)nrhs * dim);   // [scalar column][g2o order]
  std::vector<double> rhs_g2o(dim, 0.0), rhs_int, xi(idim);
  for (int v : colv)
    for (int c = 0; c < vertex_dim(h->g.vtype[v]); ++c) {
      rhs_g2o[hidx[v] + c] = 1.0;
      from_g2o_order(h, rhs_g2o.data(), rhs_int);
      rhs_g2o[hidx[v] + c] = 0.0;
      SSLAM_HIP_TRY(hipMemcpyAsync(b.V.bvec, rhs_int.data(), rhs_int.size() * 8, hipMemcpyHostToDevice, b.stream));
      hipLaunchKernelGGL(k_set_trial_all, dim3((b.V.B + 63) / 64), dim3(64), 0, b.stream, b.V, 0.0);
      if ((rc = batch_solve(b))) return rc;
      SSLAM_HIP_TRY(hipMemcpyAsync(xi.data(), b.V.x, xi.size() * 8, hipMemcpyDeviceToHost, b.stream));
      SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
      to_g2o_order(h, xi, X.data() + (size_t)(col0[v] + c) * dim);
    }
  h->linearized = false;  // b was overwritten
  size_t o = 0;
  for (auto& pr : pairs) {
    const int vr = pr.first, vc = pr.second;
    const int dr = vertex_dim(h->g.vtype[vr]), dc = vertex_dim(h->g.vtype[vc]);
    for (int r = 0; r < dr; ++r)
      for (int c = 0; c < dc; ++c)
        out[o + r * dc + c] = (hidx[vr] < 0 || hidx[vc] < 0) ? 0.0 : X[(size_t)(col0[vc] + c) * dim + hidx[vr] + r];
    o += (size_t)dr * dc;
  }
  return 0;
}

int sslam_graph_marginals(sslam_graph* h, const int* ids, int n, double* out) {
  if (!h || !ids || !out || n < 0) return set_error(SSLAM_ERR_INVALID, "null argument");
  std::vector<std::pair<int, int>> pairs(n);
  for (int k = 0; k < n; ++k) pairs[k] = {ids[k], ids[k]};
  return marginal_blocks(h, pairs, out);
}

int sslam_graph_marginals_by_hessian_index(sslam_graph* h, const int* row_col, int n, double* out) {
  if (!h || !row_col || !out || n < 0) return set_error(SSLAM_ERR_INVALID, "null argument");
  std::vector<int> hidx;
  hessian_indices(h->g, hidx);
  std::unordered_map<int, int> vert_of;   // hessian index -> vertex id
  for (int v = 0; v < h->g.nv(); ++v) if (hidx[v] >= 0) vert_of[hidx[v]] = v;
  std::vector<std::pair<int, int>> pairs(n);
  for (int k = 0; k < n; ++k) {
    auto ir = vert_of.find(row_col[2 * k]), ic = vert_of.find(row_col[2 * k + 1]);
    if (ir == vert_of.end() || ic == vert_of.end())
      return set_error(SSLAM_ERR_INVALID, "(%d, %d) is not a pair of hessian indices of active vertices", row_col[2 * k], row_col[2 * k + 1]);
    pairs[k] = {ir->second, ic->second};
  }
  return marginal_blocks(h, pairs, out);
}

// ---- g2o text format (GraphSLAM::save, graph_slam.cpp:236-239; SURVEY §5 checkpoint row) ------
int sslam_graph_save_g2o(const sslam_graph* h, const char* path) {
  if (!h || !path) return set_error(SSLAM_ERR_INVALID, "null argument");
  FILE* f = fopen(path, "w");
  if (!f) return set_error(SSLAM_ERR_IO, "cannot open %s for writing", path);
  const HostGraph& G = h->g;
  fprintf(f, "PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1\n");
  for (int v = 0; v < G.nv(); ++v) {
    const double* e = &G.est[(size_t)v * 7];
    if (G.vtype[v] == VT_SE3) fprintf(f, "VERTEX_SE3:QUAT %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", v, e[0], e[1], e[2], e[3], e[4], e[5], e[6]);
    else if (G.vtype[v] == VT_POINT) fprintf(f, "VERTEX_TRACKXYZ %d %.17g %.17g %.17g\n", v, e[0], e[1], e[2]);
    else fprintf(f, "VERTEX_PLANE %d %.17g %.17g %.17g %.17g\n", v, e[0], e[1], e[2], e[3]);
    if (G.vfixed[v]) fprintf(f, "FIX %d\n", v);
  }
  for (int k = 0; k < G.ne(); ++k) {
    const EdgeType& et = kEdgeType[G.etype[k]];
    double u[21];
    pack_upper(&G.info[(size_t)k * 36], et.d, u);
    fprintf(f, "%s %d", et.tag, G.evi[k]);
    if (et.vt_j >= 0) fprintf(f, " %d", G.evj[k]);
    for (int c = 0; c < et.extra_ints; ++c) fprintf(f, " 0");
    for (int c = 0; c < et.nz; ++c) fprintf(f, " %.17g", G.meas[(size_t)k * 7 + c]);
    for (int c = 0; c < upper_len(et.d); ++c) fprintf(f, " %.17g", u[c]);
    fprintf(f, "\n");
  }
  fclose(f);
  return 0;
}

static const EdgeType* edge_type_of_tag(const std::string& tag) {
  for (const EdgeType& et : kEdgeType) if (tag == et.tag) return &et;
  return nullptr;
}
int sslam_graph_load_g2o(sslam_graph* h, const char* path) {
  if (!h || !path) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (h->g.nv() != 0) return set_error(SSLAM_ERR_INVALID, "load requires an empty graph");
  FILE* f = fopen(path, "r");
  if (!f) return set_error(SSLAM_ERR_IO, "cannot open %s", path);
  char tag[64];
  std::unordered_map<int, int> idmap;  // file id -> vertex id (ids must be dense & ordered for exact round trips)
  auto rd = [&](double* a, int n) { for (int k = 0; k < n; ++k) if (fscanf(f, "%lf", a + k) != 1) return false; return true; };
  int rc = 0;
  while (fscanf(f, "%63s", tag) == 1) {
    const std::string t(tag);
    if (t == "VERTEX_SE3:QUAT") { int id; double e[7]; if (fscanf(f, "%d", &id) != 1 || !rd(e, 7)) { rc = -1; break; } idmap[id] = add_vertex(h, VT_SE3, e, 7, 0); }
    else if (t == "VERTEX_TRACKXYZ") { int id; double e[3]; if (fscanf(f, "%d", &id) != 1 || !rd(e, 3)) { rc = -1; break; } idmap[id] = add_vertex(h, VT_POINT, e, 3, 0); }
    else if (t == "VERTEX_PLANE") { int id; double e[4]; if (fscanf(f, "%d", &id) != 1 || !rd(e, 4)) { rc = -1; break; } idmap[id] = add_vertex(h, VT_PLANE, e, 4, 0); }
    else if (t == "FIX") { int id; if (fscanf(f, "%d", &id) != 1 || !idmap.count(id)) { rc = -1; break; } h->g.vfixed[idmap[id]] = 1; }
    else if (const EdgeType* et = edge_type_of_tag(t)) {
      int id[2] = {0, -1}, skip;
      double z[7], u[21], W[36];
      bool ok = true;
      for (int c = 0; c < (et->vt_j >= 0 ? 2 : 1); ++c) ok = ok && fscanf(f, "%d", &id[c]) == 1 && idmap.count(id[c]);
      for (int c = 0; c < et->extra_ints; ++c) ok = ok && fscanf(f, "%d", &skip) == 1;
      if (!ok || !rd(z, et->nz) || !rd(u, upper_len(et->d))) { rc = -1; break; }
      unpack_upper(u, et->d, W);
      if (add_edge(h, (int)(et - kEdgeType), idmap[id[0]], et->vt_j >= 0 ? idmap[id[1]] : -1, z, W) < 0) { rc = -1; break; }
    } else {  // PARAMS_SE3OFFSET and unknown rows: skip to end of line
      int ch; while ((ch = fgetc(f)) != EOF && ch != '\n') {}
    }
  }
  fclose(f);
  if (rc) return set_error(SSLAM_ERR_IO, "parse error in %s near tag %s", path, tag);
  return 0;
}

// ---- batch API --------------------------------------------------------------------------------
static sslam_batch* batch_create_single(sslam_graph* const* graphs, int n);
sslam_batch* sslam_batch_create(sslam_graph* const* graphs, int n) {
  const char* e = getenv("SSLAM_BATCH_STREAMS");
  return sslam_batch_create_streams(graphs, n, e ? atoi(e) : 1);
}
sslam_batch* sslam_batch_create_streams(sslam_graph* const* graphs, int n, int n_streams) {
  if (!graphs || n <= 0) { set_error(SSLAM_ERR_INVALID, "empty batch"); return nullptr; }
  const int K = std::min(std::max(n_streams, 1), std::min(n, 64));
  if (K == 1) return batch_create_single(graphs, n);
  for (int i = 0; i < n; ++i) {   // the same rule as inside one batch, across the parts
    if (!graphs[i]) { set_error(SSLAM_ERR_INVALID, "null graph"); return nullptr; }
    const Options &oa = graphs[0]->g.opt, &ob = graphs[i]->g.opt;
    if (graphs[i]->g.device != graphs[0]->g.device || oa.solver != ob.solver || oa.pcg_tol != ob.pcg_tol || oa.pcg_max_iters != ob.pcg_max_iters || oa.dcs_phi != ob.dcs_phi) {
      set_error(SSLAM_ERR_INVALID, "batch graphs must share one device and their solver options (graph %d differs from graph 0)", i); return nullptr;
    }
  }
  sslam_batch* h = new sslam_batch();
  h->b.device = graphs[0]->g.device;
  // the parts are independent batches (own tables, allocations and stream): compiled on one host thread each, as they are optimised
  h->parts.assign(K, nullptr);
  std::vector<std::string> errs(K);
  std::vector<std::thread> th;
  for (int k = 0; k < K; ++k) {
    const int lo = (int)((int64_t)n * k / K), hi = (int)((int64_t)n * (k + 1) / K);
    h->part0.push_back(lo);
    th.emplace_back([&, k, lo, hi] { h->parts[k] = batch_create_single(graphs + lo, hi - lo); if (!h->parts[k]) errs[k] = last_error_ref(); });
  }
  for (auto& t : th) t.join();
  h->part0.push_back(n);
  for (int k = 0; k < K; ++k)
    if (!h->parts[k]) { last_error_ref() = errs[k]; delete h; return nullptr; }   // (deletes the parts that were built)
  return h;
}
static sslam_batch* batch_create_single(sslam_graph* const* graphs, int n) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { set_error(SSLAM_ERR_NO_DEVICE, "no HIP device visible; the product has no CPU fallback"); return nullptr; }
  sslam_batch* h = new sslam_batch();
  h->b.device = graphs[0]->g.device;
  for (int i = 0; i < n; ++i) {
    if (!graphs[i] || graphs[i]->g.device != h->b.device) { set_error(SSLAM_ERR_INVALID, "batch graphs must share one device"); delete h; return nullptr; }
    const Options &oa = graphs[0]->g.opt, &ob = graphs[i]->g.opt;   // one set of solver options drives the whole batch
    if (oa.solver != ob.solver || oa.pcg_tol != ob.pcg_tol || oa.pcg_max_iters != ob.pcg_max_iters || oa.dcs_phi != ob.dcs_phi) {
      set_error(SSLAM_ERR_INVALID, "batch graphs must share their solver options (graph %d differs from graph 0)", i); delete h; return nullptr;
    }
    h->b.graphs.push_back(&graphs[i]->g);
  }
  if (batch_build(h->b) != 0) { delete h; return nullptr; }
  return h;
}
void sslam_batch_destroy(sslam_batch* h) { delete h; }
// A batch is compiled for the structure its graphs had at sslam_batch_create; the graphs must outlive the batch and must
// not gain vertices / edges afterwards (estimates may change: sslam_graph_set_vertex + sslam_batch_upload).
static int batch_check(sslam_batch* h) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null batch");
  for (sslam_batch* p : h->parts) { const int rc = batch_check(p); if (rc) return rc; }
  const Batch& b = h->b;
  for (size_t g = 0; g < b.graphs.size(); ++g)
    if (b.versions[g] != b.graphs[g]->structure_version)
      return set_error(SSLAM_ERR_INVALID, "graph %zu of the batch gained vertices or edges after sslam_batch_create: create a new batch", g);
  return 0;
}
int sslam_batch_upload(sslam_batch* h) {
  const int rc = batch_check(h);
  if (rc) return rc;
  if (!h->parts.empty()) return for_each_part(h, false, [](sslam_batch* p, int) { return batch_upload_estimates(p->b); });
  return batch_upload_estimates(h->b);
}
int sslam_batch_download(sslam_batch* h) {
  const int rc = batch_check(h);
  if (rc) return rc;
  if (!h->parts.empty()) return for_each_part(h, false, [](sslam_batch* p, int) { return batch_download_estimates(p->b); });
  return batch_download_estimates(h->b);
}
int sslam_batch_optimize(sslam_batch* h, int max_iters, sslam_opt_stats* out) {
  if (!h || !out) return set_error(SSLAM_ERR_INVALID, "null argument");
  const int rc = batch_check(h);
  if (rc) return rc;
  if (!h->parts.empty())
    return for_each_part(h, true, [&](sslam_batch* p, int k) { return batch_optimize(p->b, max_iters, out + h->part0[k]); });
  return batch_optimize(h->b, max_iters, out);
}
// The requests of a batch call (marginals, gate) over the parts of a stream group; a plain batch is its own single part.
struct PartSplit {
  sslam_batch* h; const bool group; const int K, ng;   // K parts, ng graphs in the whole batch
  std::vector<std::vector<int>> src;   // per part: the requests it got, in call order
  explicit PartSplit(sslam_batch* h_) : h(h_), group(!h_->parts.empty()), K(group ? (int)h_->parts.size() : 1),
                                        ng(group ? h_->part0.back() : (int)h_->b.graphs.size()), src(K) {}
  Batch& batch(int p) const { return group ? h->parts[p]->b : h->b; }
  // request k (`what` in the message) names graph g of the batch: its part *p, the graph's index *gl there; k joins src[*p]
  int place(const char* what, int k, int g, int* p, int* gl) {
    if (g < 0 || g >= ng) return set_error(SSLAM_ERR_INVALID, "%s %d: graph index %d out of range (the batch holds %d graphs)", what, k, g, ng);
    *p = group ? (int)(std::upper_bound(h->part0.begin(), h->part0.end(), g) - h->part0.begin()) - 1 : 0;
    *gl = group ? g - h->part0[*p] : g;
    src[*p].push_back(k);
    return 0;
  }
  // f(p) for the parts one after the other, from the calling thread
  int run(const std::function<int(int)>& f) { return group ? for_each_part(h, false, [&](sslam_batch*, int p) { return f(p); }) : f(0); }
};
// ---- covariance blocks of the graphs of a batch -------------------------------------------------------------------------------
// What the path kernels (marginals, gate) cannot serve: the iterative solvers have no factor to walk, an edge shard only a partial H.
static int batch_direct_only(const Batch& b, const char* what) {
  const int solver = b.graphs[0]->opt.solver;
  if (solver == 0 || solver == 2) return set_error(SSLAM_ERR_UNSUPPORTED, "sslam_batch_%s: direct solvers only (solver %d)", what, solver);
  if (b.sharded) return set_error(SSLAM_ERR_UNSUPPORTED, "sslam_batch_%s is not available in the edge-sharded mode", what);
  return 0;
}
// The shared first half of batch_marginals and batch_gate: the flat factor of the undamped H of every graph at the estimates the device
// holds, then body() while the LM states are still borrowed.  `what` names the caller in the messages.
static int batch_with_flat_factor(Batch& b, const char* what, const std::function<int()>& body) {
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  int rc;
  if ((rc = chol_set_active(b, nullptr))) return rc;   // a stale compaction (an optimise that failed half way) must not leave graphs out
  const size_t lm_bytes = sizeof(LmState) * (size_t)b.V.B;
  if (!b.d_lm_save && (rc = dev_alloc(b, (size_t)b.V.B, &b.d_lm_save, false))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(b.d_lm_save, b.V.lm, lm_bytes, hipMemcpyDeviceToDevice, b.stream));
  struct Restore {   // the LM states go back on every return path
    Batch& b; size_t bytes;
    ~Restore() { (void)hipMemcpyAsync(b.V.lm, b.d_lm_save, bytes, hipMemcpyDeviceToDevice, b.stream); (void)hipStreamSynchronize(b.stream); b.harvest(); }
  } restore{b, lm_bytes};
  if ((rc = batch_system_at_estimates(b))) return rc;   // undamped H at the current estimates
  int bad;
  if ((rc = factor_undamped_flat(b, &bad))) return rc;
  if (bad >= 0) return set_error(SSLAM_ERR_NUMERIC, "H of graph %d of the batch is not positive definite: no %s", bad, what);
  return body();
}

// Blocks of H^-1 for (graph, row vertex, column vertex) requests of ONE batch (a part of a stream group): linearise once at the estimates the
// device holds, factor the undamped H flat (factor_undamped_flat, shared with the single-graph marginal_blocks), then one
// wave per request along the elimination-tree paths (chol_marginal_blocks).  The per-graph LM states are borrowed -- the linearisation wants
// every graph at the start of an iteration, the factorisation every graph in a trial at lambda 0 -- and put back; H, b, y and the factor
// are rebuilt by the first step of whatever runs next, the estimates are only read.  out: [n][36].
static int batch_marginals(Batch& b, const std::vector<std::array<int, 3>>& req, double* out) {
  if (req.empty()) return 0;
  if (const int rc = batch_direct_only(b, "marginals")) return rc;
  std::vector<int> slot;
  const std::vector<MarginalReq> mr = marginal_requests(b, req.size(), [&](size_t k) { return req[k]; }, slot);
  std::fill(out, out + req.size() * 36, 0.0);
  if (mr.empty()) return 0;
  return batch_with_flat_factor(b, "marginals", [&]() -> int {
    std::vector<double> Z(mr.size() * 36);
    if (const int rc = chol_marginal_blocks(b, mr, Z.data())) return rc;
    for (size_t k = 0; k < req.size(); ++k)
      if (slot[k] >= 0) std::copy(Z.begin() + (size_t)slot[k] * 36, Z.begin() + (size_t)slot[k] * 36 + 36, out + k * 36);
    return 0;
  });
}

int sslam_batch_marginals(sslam_batch* h, const int32_t* req, int n, double* out) {
  if (!h || n < 0 || (n > 0 && (!req || !out))) return set_error(SSLAM_ERR_INVALID, "null argument");
  int rc = batch_check(h);
  if (rc) return rc;
  if (n == 0) return 0;
  PartSplit S(h);
  // every request is checked before anything runs: a bad one leaves out_blocks unwritten
  std::vector<std::vector<std::array<int, 3>>> preq(S.K);
  std::vector<int> dr(n), dc(n);
  for (int k = 0; k < n; ++k) {
    const int g = req[3 * k], vr = req[3 * k + 1], vc = req[3 * k + 2];
    int p, gl;
    if ((rc = S.place("request", k, g, &p, &gl))) return rc;
    const HostGraph& G = *S.batch(p).graphs[gl];
    if (vr < 0 || vr >= G.nv() || vc < 0 || vc >= G.nv()) return set_error(SSLAM_ERR_INVALID, "request %d: bad vertex id (%d, %d) in graph %d", k, vr, vc, g);
    dr[k] = vertex_dim(G.vtype[vr]); dc[k] = vertex_dim(G.vtype[vc]);
    preq[p].push_back({gl, vr, vc});
  }
  std::vector<std::vector<double>> pz(S.K);
  if ((rc = S.run([&](int p) { pz[p].resize(preq[p].size() * 36 + 1); return batch_marginals(S.batch(p), preq[p], pz[p].data()); }))) return rc;
  std::vector<size_t> off(n + 1, 0);
  for (int k = 0; k < n; ++k) off[k + 1] = off[k] + (size_t)dr[k] * dc[k];
  for (int p = 0; p < S.K; ++p)
    for (size_t i = 0; i < S.src[p].size(); ++i) {
      const int k = S.src[p][i];
      std::copy(pz[p].begin() + i * 36, pz[p].begin() + i * 36 + (size_t)dr[k] * dc[k], out + off[k]);
    }
  return 0;
}
// ---- loop-closure gate: Mahalanobis distance of candidate edges ---------------------------------------------------------------------
// One candidate against its host graph, before anything runs.  k: its number in the call (messages).
static int gate_check(const HostGraph& G, int k, int kind, int vu, int vv, const double* z, const double* info) {
  if (kind != SSLAM_GATE_SE3 && kind != SSLAM_GATE_SE3_POINT) return set_error(SSLAM_ERR_INVALID, "candidate %d: unknown kind %d", k, kind);
  if (vu < 0 || vu >= G.nv() || vv < 0 || vv >= G.nv() || vu == vv) return set_error(SSLAM_ERR_INVALID, "candidate %d: vertex ids (%d, %d) invalid", k, vu, vv);
  if (G.vtype[vu] != VT_SE3 || G.vtype[vv] != (kind == SSLAM_GATE_SE3 ? VT_SE3 : VT_POINT))
    return set_error(SSLAM_ERR_INVALID, "candidate %d: a vertex of (%d, %d) has the wrong type for this kind of edge", k, vu, vv);
  const int nz = kind == SSLAM_GATE_SE3 ? 7 : 3, d = kind == SSLAM_GATE_SE3 ? 6 : 3;
  for (int i = 0; i < nz; ++i) if (!std::isfinite(z[i])) return set_error(SSLAM_ERR_INVALID, "candidate %d: the measurement has a non-finite entry", k);
  if (kind == SSLAM_GATE_SE3 && !(z[3] * z[3] + z[4] * z[4] + z[5] * z[5] + z[6] * z[6] > 0)) return set_error(SSLAM_ERR_INVALID, "candidate %d: quaternion of zero norm", k);
  if (info) for (int i = 0; i < d * d; ++i) if (!std::isfinite(info[i])) return set_error(SSLAM_ERR_INVALID, "candidate %d: the information matrix has a non-finite entry", k);
  return 0;
}
// the candidate's record for chol_gate_pairs, and its measurement in the kernel's layout (io: 44 doubles)
static GateReq gate_request(const Batch& b, int g, int kind, int vu, int vv, const double* z, const double* info, double* io) {
  const bool se3 = kind == SSLAM_GATE_SE3;
  std::fill(io, io + 44, 0.0);
  std::copy(z, z + (se3 ? 7 : 3), io);
  if (info) std::copy(info, info + (se3 ? 36 : 9), io + 8);
  return {vertex_xoff(b, g, vu), 6, vertex_xoff(b, g, vv), se3 ? 6 : 3, kind, b.T.v2pose[g][vu], se3 ? b.T.v2pose[g][vv] : b.T.v2lm[g][vv], info ? 1 : 0};
}
// d2, e and S of candidate k out of the kernel's record
static void gate_result(const double* io, int k, double* d2_out, double* e_out, double* cov_out) {
  d2_out[k] = io[0];
  if (e_out) std::copy(io + 1, io + 7, e_out + (size_t)k * 6);
  if (cov_out) std::copy(io + 8, io + 44, cov_out + (size_t)k * 36);
}
// The candidates of ONE batch (a part of a stream group): the flat factor as batch_marginals takes it, then one wave per candidate.
static int batch_gate(Batch& b, const std::vector<GateReq>& req, const double* in, double* out) {
  if (req.empty()) return 0;
  if (const int rc = batch_direct_only(b, "gate")) return rc;
  return batch_with_flat_factor(b, "gate", [&]() -> int { return chol_gate_pairs(b, req, in, out); });
}

int sslam_batch_gate(sslam_batch* h, const int32_t* cand, const double* z, const double* info, int n, double* d2_out, double* e_out, double* cov_out) {
  if (!h || n < 0 || (n > 0 && (!cand || !z || !d2_out))) return set_error(SSLAM_ERR_INVALID, "null argument");
  int rc = batch_check(h);
  if (rc) return rc;
  if (n == 0) return 0;
  PartSplit S(h);
  // every candidate is checked before anything runs: a bad one leaves the outputs unwritten
  std::vector<std::vector<GateReq>> preq(S.K);
  std::vector<std::vector<double>> pin(S.K), pout(S.K);
  for (int k = 0; k < n; ++k) {
    const int g = cand[4 * k], kind = cand[4 * k + 1], vu = cand[4 * k + 2], vv = cand[4 * k + 3];
    int p, gl;
    if ((rc = S.place("candidate", k, g, &p, &gl))) return rc;
    const Batch& pb = S.batch(p);
    const double *zk = z + (size_t)k * 7, *wk = info ? info + (size_t)k * 36 : nullptr;
    if ((rc = gate_check(*pb.graphs[gl], k, kind, vu, vv, zk, wk))) return rc;
    pin[p].resize(pin[p].size() + 44);
    preq[p].push_back(gate_request(pb, gl, kind, vu, vv, zk, wk, pin[p].data() + pin[p].size() - 44));
  }
  if ((rc = S.run([&](int p) { pout[p].resize(pin[p].size() + 1); return batch_gate(S.batch(p), preq[p], pin[p].data(), pout[p].data()); }))) return rc;
  for (int p = 0; p < S.K; ++p)
    for (size_t i = 0; i < S.src[p].size(); ++i) gate_result(pout[p].data() + i * 44, S.src[p][i], d2_out, e_out, cov_out);
  return 0;
}

// The single-graph handle: its batch of one, linearised at the host estimates as marginal_blocks does, then the same factor and kernel.
int sslam_graph_gate(sslam_graph* h, const int32_t* cand, const double* z, const double* info, int n, double* d2_out, double* e_out, double* cov_out) {
  if (!h || n < 0 || (n > 0 && (!cand || !z || !d2_out))) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (n == 0) return 0;
  int rc;
  for (int k = 0; k < n; ++k)
    if ((rc = gate_check(h->g, k, cand[3 * k], cand[3 * k + 1], cand[3 * k + 2], z + (size_t)k * 7, info ? info + (size_t)k * 36 : nullptr))) return rc;
  if (h->g.opt.solver == 0 || h->g.opt.solver == 2) return set_error(SSLAM_ERR_UNSUPPORTED, "sslam_graph_gate: direct solvers only (solver %d)", h->g.opt.solver);
  if ((rc = do_linearize(h))) return rc;  // undamped H at the current estimates
  Batch& b = *h->batch;
  int bad;
  if ((rc = factor_undamped_flat(b, &bad))) return rc;
  if (bad >= 0) return set_error(SSLAM_ERR_NUMERIC, "H is not positive definite: no gate");
  std::vector<GateReq> req;
  std::vector<double> in((size_t)n * 44), out((size_t)n * 44);
  for (int k = 0; k < n; ++k)
    req.push_back(gate_request(b, 0, cand[3 * k], cand[3 * k + 1], cand[3 * k + 2], z + (size_t)k * 7, info ? info + (size_t)k * 36 : nullptr, in.data() + (size_t)k * 44));
  if ((rc = chol_gate_pairs(b, req, in.data(), out.data()))) return rc;
  for (int k = 0; k < n; ++k) gate_result(out.data() + (size_t)k * 44, k, d2_out, e_out, cov_out);
  return 0;
}
// ---- one linear solve of every graph of a batch (parity hook) --------------------------------------------------------------------
// (H_g + lambda[g] I) x_g = b_g of ONE batch (a part of a stream group) at the estimates the device holds, through the launches the LM loop
// takes: the LM states are borrowed as batch_marginals borrows them, every graph gets its own damping (k_set_trial_each), and the graphs
// with lambda < 0 sit out as terminated graphs do in the LM endgame -- the launches are sized by chol_set_active with that mask.
// x: V.x in the batch's internal row order; iters / fail: per graph.
static int batch_solve_each(Batch& b, const double* lambda, std::vector<double>& x, std::vector<long long>& iters, std::vector<int>& fail) {
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  const int B = b.V.B;
  int rc;
  if (!b.uploaded && (rc = batch_upload_estimates(b))) return rc;
  if ((rc = chol_set_active(b, nullptr))) return rc;
  const size_t lm_bytes = sizeof(LmState) * (size_t)B;
  if (!b.d_lm_save && (rc = dev_alloc(b, (size_t)B, &b.d_lm_save, false))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(b.d_lm_save, b.V.lm, lm_bytes, hipMemcpyDeviceToDevice, b.stream));
  struct Restore {   // the LM states and the full launch ranges go back on every return path
    Batch& b; size_t bytes;
    ~Restore() {
      (void)chol_set_active(b, nullptr);
      (void)hipMemcpyAsync(b.V.lm, b.d_lm_save, bytes, hipMemcpyDeviceToDevice, b.stream); (void)hipStreamSynchronize(b.stream); b.harvest();
    }
  } restore{b, lm_bytes};
  if ((rc = batch_chi2(b, b.V.pose, b.V.lmk, 0))) return rc;
  hipLaunchKernelGGL(k_lm_init, dim3(B), dim3(64), 0, b.stream, b.V, b.d_part_e, 0);
  if ((rc = batch_linearize(b))) return rc;
  // the lambdas travel through the max-diagonal partials (B doubles at least), which nothing reads between here and the solve
  std::vector<char> mask((size_t)B);
  for (int g = 0; g < B; ++g) mask[g] = lambda[g] >= 0 ? 1 : 0;
  SSLAM_HIP_TRY(hipMemcpyAsync(b.d_part_m, lambda, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, b.stream));
  hipLaunchKernelGGL(k_set_trial_each, dim3((B + 63) / 64), dim3(64), 0, b.stream, b.V, b.d_part_m);
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));   // `lambda` is the caller's
  x.assign((size_t)6 * b.V.nPr + (size_t)3 * b.V.nLr, 0.0);
  iters.assign((size_t)B, 0); fail.assign((size_t)B, 0);
  if (std::find(mask.begin(), mask.end(), (char)1) == mask.end()) return launch_check("solve");   // nobody takes part: nothing to launch
  const int solver = b.graphs[0]->opt.solver;
  if (solver != 0 && solver != 2 && !b.chol && (rc = chol_plan_build(b))) return rc;   // chol_set_active needs the plan
  if ((rc = chol_set_active(b, &mask))) return rc;
  if ((rc = batch_solve(b))) return rc;
  std::vector<LmState> st((size_t)B);
  if (!x.empty()) SSLAM_HIP_TRY(hipMemcpyAsync(x.data(), b.V.x, x.size() * 8, hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipMemcpyAsync(fail.data(), b.V.pcg_fail, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, b.stream));
  if ((rc = read_lm_state(b, st))) return rc;
  for (int g = 0; g < B; ++g) { iters[g] = st[g].pcg_iters; if (!mask[g]) fail[g] = 0; }
  if ((rc = chol_set_active(b, nullptr))) return rc;
  if ((rc = launch_check("solve"))) return rc;
  return chol_flow_check(b);
}

int64_t sslam_batch_solve(sslam_batch* h, const double* lambda, double* x, int64_t capacity, int64_t* solver_iterations) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null batch");
  int rc = batch_check(h);
  if (rc) return rc;
  const bool group = !h->parts.empty();
  const int K = group ? (int)h->parts.size() : 1;
  auto part_batch = [&](int k) -> Batch& { return group ? h->parts[k]->b : h->b; };
  // every graph's unknowns in its own hessian-index order, one graph after the other
  std::vector<int64_t> goff;
  std::vector<std::vector<int>> hidx;
  int64_t total = 0;
  for (int k = 0; k < K; ++k)
    for (HostGraph* G : part_batch(k).graphs) {
      hidx.emplace_back();
      goff.push_back(total);
      total += hessian_indices(*G, hidx.back());
    }
  if (!x) return total;
  if (!lambda) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (capacity < total) return set_error(SSLAM_ERR_INVALID, "buffer of %lld doubles needed", (long long)total);
  for (int k = 0; k < K; ++k)
    if (part_batch(k).sharded) return set_error(SSLAM_ERR_UNSUPPORTED, "sslam_batch_solve is not available in the edge-sharded mode");
  std::vector<int> first(K + 1, 0);
  for (int k = 0; k < K; ++k) first[k + 1] = first[k] + (int)part_batch(k).graphs.size();
  for (int g = 0; g < first[K]; ++g)
    if (!(lambda[g] == lambda[g]) || std::isinf(lambda[g])) return set_error(SSLAM_ERR_INVALID, "lambda of graph %d is not finite", g);
  std::fill(x, x + total, 0.0);
  if (solver_iterations) std::fill(solver_iterations, solver_iterations + first[K], (int64_t)0);
  // the parts of a stream group one after the other, from the calling thread
  auto run = [&](int p) {
    Batch& b = part_batch(p);
    std::vector<double> xi;
    std::vector<long long> iters;
    std::vector<int> fail;
    int rc2 = batch_solve_each(b, lambda + first[p], xi, iters, fail);
    if (rc2) return rc2;
    for (int gl = 0; gl < (int)b.graphs.size(); ++gl) {
      const int g = first[p] + gl;
      if (!(lambda[g] >= 0)) continue;
      if (fail[gl]) return set_error(SSLAM_ERR_NUMERIC, "linear solve of graph %d of the batch broke down", g);
      if (solver_iterations) solver_iterations[g] = iters[gl];
      const HostGraph& G = *b.graphs[gl];
      double* xo = x + goff[g];
      for (int v = 0; v < G.nv(); ++v) {
        const int xr = vertex_xoff(b, gl, v), o = hidx[g][v];
        if (xr < 0 || o < 0) continue;
        const int d = vertex_dim(G.vtype[v]);
        for (int a = 0; a < d; ++a) xo[o + a] = xi[(size_t)xr + a];
      }
    }
    return 0;
  };
  if (group) rc = for_each_part(h, false, [&](sslam_batch*, int p) { return run(p); });
  else rc = run(0);
  return rc ? rc : total;
}
// ---- edge-sharded mode (SURVEY 8e mode E; BASELINE.json configs[4]): the edges of every graph of the batch are split
//      contiguously over the ranks, each rank builds the partial normal equations of its edges, ONE RCCL all-reduce of the
//      contiguous [H || b] buffer sums them, and the rest of the LM step runs replicated.
static int batch_set_shard(Batch& b, int rank, int world) {
  if (world < 1 || rank < 0 || rank >= world) return set_error(SSLAM_ERR_INVALID, "bad rank %d of %d", rank, world);
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  std::vector<int> lo(b.graphs.size()), hi(b.graphs.size());
  for (size_t g = 0; g < b.graphs.size(); ++g) {
    const int n = b.graphs[g]->ne();
    const int base = n / world, extra = n % world;
    lo[g] = rank * base + std::min(rank, extra);
    hi[g] = lo[g] + base + (rank < extra ? 1 : 0);
    if (world == 1) { lo[g] = 0; hi[g] = 0x7fffffff; }
  }
  SSLAM_HIP_TRY(hipMemcpyAsync((void*)b.V.shard_lo, lo.data(), lo.size() * sizeof(int), hipMemcpyHostToDevice, b.stream));
  SSLAM_HIP_TRY(hipMemcpyAsync((void*)b.V.shard_hi, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, b.stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  b.sharded = world > 1 || b.comm != nullptr;   // a forced single-rank communicator keeps the whole sharded path (masked kernels + all-reduce) on
  b.shard_rank = rank; b.shard_world = world;
  if (b.sharded && !b.d_hb_part) {
    int rc;
    if ((rc = dev_alloc(b, (size_t)b.hb_doubles, &b.d_hb_part))) return rc;
    SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  }
  return 0;
}
int sslam_comm_unique_id(char id_out[128]) {
  if (!id_out) return set_error(SSLAM_ERR_INVALID, "null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  if (!rccl_api().ok()) return set_error(SSLAM_ERR_UNSUPPORTED, "librccl.so could not be loaded: %s", dlerror());
  ncclUniqueId id;
  const ncclResult_t r = rccl_api().GetUniqueId(&id);
  if (r != ncclSuccess) return set_error(SSLAM_ERR_HIP, "ncclGetUniqueId: %s", rccl_api().GetErrorString(r));
  memcpy(id_out, &id, sizeof id);
  return 0;
}
int sslam_batch_comm_init(sslam_batch* h, const char id_in[128], int rank, int world) {
  if (!h || !id_in) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (!h->parts.empty()) return set_error(SSLAM_ERR_UNSUPPORTED, "not available on a stream group: the edge-sharded mode and the [H || b] read-back work on single-stream batches");
  Batch& b = h->b;
  int rc = batch_check(h);
  if (rc) return rc;
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  if (b.comm) { batch_comm_destroy(b.comm); b.comm = nullptr; }
  // world == 1 switches the mode off -- unless SSLAM_FORCE_COMM=1 asks for a single-rank communicator: the whole product path of the
  // mode (shard-masked kernels, ncclCommInitRank, the out-of-place ncclAllReduce on the batch's stream) then runs on one GPU
  const char* force = getenv("SSLAM_FORCE_COMM");
  if (world > 1 || (force && atoi(force) != 0)) {
    if (!rccl_api().ok()) return set_error(SSLAM_ERR_UNSUPPORTED, "librccl.so could not be loaded: %s", dlerror());
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof id);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = rccl_api().CommInitRank(&comm, world, id, rank);
    if (r != ncclSuccess) return set_error(SSLAM_ERR_HIP, "ncclCommInitRank(rank %d of %d): %s", rank, world, rccl_api().GetErrorString(r));
    b.comm = comm;
  }
  return batch_set_shard(b, rank, world);
}
int sslam_batch_set_edge_shard(sslam_batch* h, int rank, int world) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null batch");
  if (!h->parts.empty()) return set_error(SSLAM_ERR_UNSUPPORTED, "not available on a stream group: the edge-sharded mode and the [H || b] read-back work on single-stream batches");
  int rc = batch_check(h);
  if (rc) return rc;
  return batch_set_shard(h->b, rank, world);
}
int64_t sslam_batch_linearize_hb(sslam_batch* h, double* h_and_b, int64_t capacity) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null batch");
  if (!h->parts.empty()) return set_error(SSLAM_ERR_UNSUPPORTED, "not available on a stream group: the edge-sharded mode and the [H || b] read-back work on single-stream batches");
  Batch& b = h->b;
  if (!h_and_b) return b.hb_doubles;
  if (capacity < b.hb_doubles) return set_error(SSLAM_ERR_INVALID, "buffer of %lld doubles needed", (long long)b.hb_doubles);
  int rc = batch_check(h);
  if (rc) return rc;
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  if ((rc = batch_system_at_estimates(b))) return rc;
  SSLAM_HIP_TRY(hipMemcpyAsync(h_and_b, b.V.Hpp_diag, (size_t)b.hb_doubles * sizeof(double), hipMemcpyDeviceToHost, b.stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(b.stream));
  b.harvest();
  return b.hb_doubles;
}

int sslam_batch_time_linearize(sslam_batch* h, int repeats, double* ms_per_build) {
  if (!h || !ms_per_build || repeats <= 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (!h->parts.empty()) {   // the parts one after the other: their times add up to one build of every graph
    *ms_per_build = 0;
    return for_each_part(h, false, [&](sslam_batch* p, int) { double ms = 0; const int rc = sslam_batch_time_linearize(p, repeats, &ms); *ms_per_build += ms; return rc; });
  }
  Batch& b = h->b;
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  int rc;
  if ((rc = batch_system_at_estimates(b, false))) return rc;
  const bool prof = b.profiling;
  b.profiling = false;
  if ((rc = batch_linearize(b))) return rc;  // warm-up
  hipEvent_t e0, e1;
  SSLAM_HIP_TRY(hipEventCreate(&e0)); SSLAM_HIP_TRY(hipEventCreate(&e1));
  SSLAM_HIP_TRY(hipEventRecord(e0, b.stream));
  for (int k = 0; k < repeats; ++k) if ((rc = batch_linearize(b))) return rc;
  SSLAM_HIP_TRY(hipEventRecord(e1, b.stream));
  SSLAM_HIP_TRY(hipEventSynchronize(e1));
  float ms = 0;
  SSLAM_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  hipEventDestroy(e0); hipEventDestroy(e1);
  b.profiling = prof;
  *ms_per_build = (double)ms / repeats;
  return 0;
}
// one numeric factorisation (+ fused forward solve) and one backward solve of EVERY graph of the batch, `repeats` times: mean
// milliseconds by hipEvents on the batch's stream (the LM loop's own launches mix full and partial rounds)
int sslam_batch_time_solver(sslam_batch* h, int repeats, double* factor_ms, double* solve_ms) {
  if (!h || repeats <= 0 || !factor_ms || !solve_ms) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (!h->parts.empty()) {
    *factor_ms = *solve_ms = 0;
    return for_each_part(h, false, [&](sslam_batch* p, int) {
      double f = 0, v = 0; const int rc = sslam_batch_time_solver(p, repeats, &f, &v); *factor_ms += f; *solve_ms += v; return rc; });
  }
  Batch& b = h->b;
  if (b.graphs[0]->opt.solver == 0 || b.graphs[0]->opt.solver == 2) return set_error(SSLAM_ERR_UNSUPPORTED, "direct solvers only");
  SSLAM_HIP_TRY(hipSetDevice(b.device));
  int rc;
  if ((rc = chol_set_active(b, nullptr))) return rc;   // a stale compaction (an optimise that failed half way) must not shrink what is timed
  if ((rc = batch_system_at_estimates(b))) return rc;
  hipLaunchKernelGGL(k_set_trial_all, dim3((b.V.B + 63) / 64), dim3(64), 0, b.stream, b.V, 1.0);
  struct Restore {   // events and the profiling switch are put back on every return path
    Batch& b; bool prof; hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Restore() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); b.profiling = prof; }
  } guard{b, b.profiling};
  b.profiling = false;
  if ((rc = batch_solve(b))) return rc;   // warm-up (builds the plan)
  SSLAM_HIP_TRY(hipEventCreate(&guard.e[0])); SSLAM_HIP_TRY(hipEventCreate(&guard.e[1])); SSLAM_HIP_TRY(hipEventCreate(&guard.e[2]));
  hipEvent_t e0 = guard.e[0], e1 = guard.e[1], e2 = guard.e[2];
  double tf = 0, ts = 0;
  for (int k = 0; k < repeats; ++k) {
    SSLAM_HIP_TRY(hipEventRecord(e0, b.stream));
    if ((rc = chol_factor_and_forward(b))) return rc;
    SSLAM_HIP_TRY(hipEventRecord(e1, b.stream));
    if ((rc = chol_backward(b))) return rc;
    SSLAM_HIP_TRY(hipEventRecord(e2, b.stream));
    SSLAM_HIP_TRY(hipEventSynchronize(e2));
    float a = 0, c = 0;
    SSLAM_HIP_TRY(hipEventElapsedTime(&a, e0, e1)); SSLAM_HIP_TRY(hipEventElapsedTime(&c, e1, e2));
    tf += a; ts += c;
  }
  *factor_ms = tf / repeats; *solve_ms = ts / repeats;
  return 0;
}
int64_t sslam_batch_linearize_bytes(const sslam_batch* h) {
  if (!h) return 0;
  if (!h->parts.empty()) { int64_t t = 0; for (const sslam_batch* p : h->parts) t += sslam_batch_linearize_bytes(p); return t; }
  const Batch& b = h->b;
  // per edge its type's lin_bytes (kEdgeType) + 288*Np + 72*Nl + 48*Np + 24*Nl
  // position priors (k_linearize_priors): + 268 per pose row that carries one (pose 64, row and CSR entries 8 + 4, the 9 + 3 doubles of
  // H and b it adds to read 96 and written 96)
  int64_t bytes = 0;
  for (size_t g = 0; g < b.graphs.size(); ++g) {
    const HostGraph& G = *b.graphs[g];
    for (int k = 0; k < G.ne(); ++k) bytes += kEdgeType[G.etype[k]].lin_bytes;
  }
  bytes += (int64_t)b.V.nPr * (288 + 48) + (int64_t)b.V.nLr * (72 + 24) + (int64_t)b.V.nEpRows * 268;
  return bytes;
}
int sslam_batch_info(sslam_batch* h, const char* key, double* value) {
  if (!h || !key || !value) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (!h->parts.empty()) {   // sums over the parts; the depth of the plans is their maximum
    const std::string kk(key);
    if (kk == "streams") { *value = (double)h->parts.size(); return 0; }
    const bool least = kk == "front_groups_per_cu_leaf" || kk == "front_groups_per_cu_mid";   // (residency of the front launches: the parts' minimum)
    double acc = 0;
    for (sslam_batch* p : h->parts) {
      double v = 0;
      const int rc = sslam_batch_info(p, key, &v);
      if (rc) return rc;
      acc = kk == "factor_levels" ? std::max(acc, v) : (least ? (p == h->parts.front() ? v : std::min(acc, v)) : acc + v);
    }
    *value = acc;
    return 0;
  }
  if (std::string(key) == "streams") { *value = 1; return 0; }
  Batch& b = h->b;
  const std::string k(key);
  int rc;
  const bool per_cu = k == "front_groups_per_cu_leaf" || k == "front_groups_per_cu_mid";
  if ((k == "factor_lnz" || k == "factor_levels" || k == "factor_launches" || k == "factor_front" || k == "factor_bytes" || per_cu) && !b.chol && (rc = chol_plan_build(b))) return rc;
  const double dim = 6.0 * b.V.nPr + 3.0 * b.V.nLr;
  if (k == "factor_lnz") *value = (double)chol_plan_lnz(b);
  else if (k == "factor_levels") *value = (double)chol_plan_levels(b);
  else if (k == "factor_launches") *value = (double)chol_plan_launches(b);
  else if (k == "factor_front") *value = chol_plan_front(b) ? 1.0 : 0.0;
  else if (per_cu) *value = (double)chol_plan_front_per_cu(b, k == "front_groups_per_cu_mid");   // front workgroups a CU holds (0: no front tables)
  else if (k == "h_doubles") *value = (double)b.V.h_total;
  else if (k == "dim") *value = dim;
  else if (k == "allreduce_calls") *value = (double)b.allreduce_calls;
  else if (k == "compact_rounds") *value = (double)b.compact_rounds;   // chol_set_active calls that sized the launches by index lists
  else if (k == "lm_fused_launches") *value = (double)chol_plan_lm_launches(b, false);   // k_chol_flow launches that carried the halves of a damping trial
  else if (k == "lm_spec_rounds") *value = (double)chol_plan_lm_launches(b, true);       // k_chol_spec_round launches
  else if (k == "factor_bytes") *value = 8.0 * ((double)b.V.h_total + dim + (double)chol_plan_lnz(b) + dim);
  else return set_error(SSLAM_ERR_INVALID, "unknown info key '%s'", key);
  return 0;
}
int sslam_batch_set_profiling(sslam_batch* h, int enable) {
  if (!h) return set_error(SSLAM_ERR_INVALID, "null batch");
  for (sslam_batch* p : h->parts) sslam_batch_set_profiling(p, enable);
  h->b.profiling = enable != 0;
  h->b.timers.clear();
  return 0;
}
int sslam_batch_kernel_time(sslam_batch* h, const char* name, double* total_ms, int64_t* launches) {
  if (!h || !name) return set_error(SSLAM_ERR_INVALID, "null argument");
  if (!h->parts.empty()) {   // per-stream event times, summed: the parts' kernels overlap on the chip, so the sum exceeds the wall time
    double t = 0; int64_t n = 0;
    for (sslam_batch* p : h->parts) { double a = 0; int64_t c = 0; sslam_batch_kernel_time(p, name, &a, &c); t += a; n += c; }
    if (total_ms) *total_ms = t;
    if (launches) *launches = n;
    return 0;
  }
  auto it = h->b.timers.find(name);
  if (total_ms) *total_ms = it == h->b.timers.end() ? 0.0 : it->second.total_ms;
  if (launches) *launches = it == h->b.timers.end() ? 0 : it->second.launches;
  return 0;
}

// ---- plan introspection (host only, no device needed): the batch tables (batch_tables.hpp) and the symbolic Cholesky plan of a batch as
// flat arrays.  The same batch_compile as a device batch runs; only batch_upload is left out.
struct sslam_debug_plan { CholHost H; BatchTables T; };
void* sslam_debug_plan_create(sslam_graph* const* graphs, int n) {
  if (!graphs || n <= 0) { set_error(SSLAM_ERR_INVALID, "empty batch"); return nullptr; }
  std::vector<HostGraph*> gs;
  for (int i = 0; i < n; ++i) { if (!graphs[i]) { set_error(SSLAM_ERR_INVALID, "null graph"); return nullptr; } gs.push_back(&graphs[i]->g); }
  static const bool timing = getenv("SSLAM_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<sslam_debug_plan> P(new sslam_debug_plan());
  if (batch_compile_checked(gs, P->T) != 0) return nullptr;
  const auto t1 = std::chrono::steady_clock::now();
  SymIn in;
  chol_sym_input(P->T, in);
  CholOpts opt;
  opt.from_env();
  chol_opts_normalise(opt, n, P->T.nPr() + P->T.nLr());   // the plan chol_plan_build would execute, small-batch regime included
  if (chol_symbolic(in, opt, P->H)) { set_error(SSLAM_ERR_NUMERIC, "Cholesky plan: %s", P->H.error.c_str()); return nullptr; }
  if (timing) fprintf(stderr, "[timing] host plan: batch tables %.3f ms, symbolic Cholesky %.3f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  return P.release();
}
void sslam_debug_plan_destroy(void* p) { delete (sslam_debug_plan*)p; }
int64_t sslam_debug_plan_array(void* p, const char* name, void* out, int64_t cap_bytes) {
  if (!p || !name) return set_error(SSLAM_ERR_INVALID, "null argument");
  const CholHost& H = ((sslam_debug_plan*)p)->H;
  const BatchTables& T = ((sslam_debug_plan*)p)->T;
  const EdgeClassTab &EO = T.cls[EC_SE3], &EL = T.cls[EC_LANDMARK], &ELL = T.cls[EC_POINT_POINT], &EP = T.cls[EC_PRIOR];
  const std::string k(name);
  const void* src = nullptr; int64_t bytes = 0;
  int scal[17] = {H.ncol, H.nlevels, H.dim, H.B, H.npiece, (int)H.lnz, H.tail_lds_f, H.tail_lds_b, H.nt_leaf, H.nt_tail, (int)T.h_total,
                  T.nPr(), T.nLr(), (int)T.hll_base, (int)T.hpp_off_base, (int)T.hpl_base, (int)H.unz};
#define ARR(nm, vec) if (k == nm) { src = (vec).data(); bytes = (int64_t)(vec).size() * sizeof((vec)[0]); }
  ARR("col", H.col) ARR("blk", H.blk) ARR("upd", H.upd) ARR("item", H.item) ARR("mb", H.mb) ARR("ilv", H.ilv) ARR("piece", H.piece)
  ARR("lvl_ptr", H.lvl_ptr) ARR("lvl_cols", H.lvl_cols) ARR("plv_ptr", H.plv_ptr) ARR("plv_pieces", H.plv_pieces)
  ARR("ppoff", T.ppoff) ARR("plblk", T.plblk) ARR("tail_ptr", H.tail_ptr)
  ARR("asrc", H.asrc) ARR("usrc", H.usrc) ARR("fwd", H.fwd) ARR("uitem", H.uitem) ARR("umb", H.umb) ARR("tail_pieces", H.tail_pieces) ARR("plv_lds_f", H.plv_lds_f) ARR("plv_lds_b", H.plv_lds_b)
  ARR("rcol", H.rcol) ARR("rupd", H.rupd) ARR("plv_nt", H.plv_nt) ARR("plv_cls", H.plv_cls)
  ARR("fblob", H.fblob) ARR("fgrp", H.fgrp) ARR("plv_lds_ff", H.plv_lds_ff) ARR("flds", H.flds) ARR("col_comp", H.col_comp)
  // the batch tables, under the names of BatchTables; a storage class's arrays are <class>_{a, b, blk, id, z, w} with class eo, el, ell, ep
  ARR("seg", T.seg) ARR("pose_row", T.pose_row) ARR("lm_row", T.lm_row) ARR("prow_pose", T.prow_pose) ARR("lrow_lm", T.lrow_lm)
  ARR("prow_graph", T.prow_graph) ARR("lrow_graph", T.lrow_graph) ARR("pose_vertex", T.pose_vertex) ARR("lm_vertex", T.lm_vertex)
  ARR("lm_kind", T.lm_kind) ARR("prow_perm", T.prow_perm) ARR("llblk", T.llblk)
  ARR("eo_a", EO.a) ARR("eo_b", EO.b) ARR("eo_blk", EO.blk) ARR("eo_id", EO.id) ARR("eo_z", EO.z) ARR("eo_w", EO.w)
  ARR("el_a", EL.a) ARR("el_b", EL.b) ARR("el_blk", EL.blk) ARR("el_id", EL.id) ARR("el_z", EL.z) ARR("el_w", EL.w)
  ARR("ell_a", ELL.a) ARR("ell_b", ELL.b) ARR("ell_blk", ELL.blk) ARR("ell_id", ELL.id) ARR("ell_z", ELL.z) ARR("ell_w", ELL.w)
  ARR("ep_a", EP.a) ARR("ep_id", EP.id) ARR("ep_z", EP.z) ARR("ep_w", EP.w) ARR("ep_dim", EP.dim)
  ARR("pslot_ptr", T.pslot_ptr) ARR("pslot_rec", T.pslot_rec) ARR("lslot_ptr", T.lslot_ptr) ARR("lslot_edge", T.lslot_edge)
  ARR("llslot_ptr", T.llslot_ptr) ARR("llslot_rec", T.llslot_rec) ARR("llblk_ptr", T.llblk_ptr) ARR("llblk_edge", T.llblk_edge)
  ARR("dup_eo", T.dup_eo) ARR("dup_el", T.dup_el) ARR("ep_row", T.ep_row) ARR("ep_ptr", T.ep_ptr) ARR("ep_edge", T.ep_edge)
  ARR("adj_ptr", T.adj_ptr) ARR("adj_blk", T.adj_blk) ARR("adj_x", T.adj_x) ARR("adj_fmt", T.adj_fmt)
  ARR("shard_lo", T.shard_lo) ARR("shard_hi", T.shard_hi)
#undef ARR
  int fscal[4] = {H.front ? 1 : 0, (int)H.funz, H.tail_lds_ff, 0};   // front tables (front_plan.hpp): present, doubles of update matrices, LDS of the tail
  if (k == "fscalars") { src = fscal; bytes = sizeof fscal; }
  if (k == "scalars") { src = scal; bytes = sizeof scal; }
  static const char* known[] = {"col", "blk", "upd", "item", "mb", "ilv", "piece", "lvl_ptr", "lvl_cols", "plv_ptr", "plv_pieces", "ppoff", "plblk",
                                "tail_ptr", "tail_pieces", "plv_lds_f", "plv_lds_b", "scalars", "asrc", "usrc", "fwd", "uitem", "umb", "rcol", "rupd", "plv_nt", "plv_cls",
                                "fblob", "fgrp", "plv_lds_ff", "fscalars", "flds", "col_comp",
                                "seg", "pose_row", "lm_row", "prow_pose", "lrow_lm", "prow_graph", "lrow_graph", "pose_vertex", "lm_vertex", "lm_kind", "prow_perm", "llblk",
                                "eo_a", "eo_b", "eo_blk", "eo_id", "eo_z", "eo_w", "el_a", "el_b", "el_blk", "el_id", "el_z", "el_w",
                                "ell_a", "ell_b", "ell_blk", "ell_id", "ell_z", "ell_w", "ep_a", "ep_id", "ep_z", "ep_w", "ep_dim",
                                "pslot_ptr", "pslot_rec", "lslot_ptr", "lslot_edge", "llslot_ptr", "llslot_rec", "llblk_ptr", "llblk_edge",
                                "dup_eo", "dup_el", "ep_row", "ep_ptr", "ep_edge", "adj_ptr", "adj_blk", "adj_x", "adj_fmt", "shard_lo", "shard_hi"};
  bool ok = false;
  for (const char* q : known) ok |= (k == q);
  if (!ok) return set_error(SSLAM_ERR_INVALID, "unknown plan array '%s'", name);
  if (out && cap_bytes >= bytes && bytes > 0) memcpy(out, src, (size_t)bytes);
  return bytes;
}

}  // extern "C"
