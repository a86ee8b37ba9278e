// The path kernels: blocks of H^-1 (marginals) and the Mahalanobis gate of candidate edges, from the elimination-tree paths of the flat
// factor -- included by sslam_chol.hip after its device helpers.  Their requests are cut into rounds of records by path_rounds.hpp (the
// record layout, the placement rule and the scratch slices are written there); the round driver of sslam_chol.hip launches them.
#pragma once

namespace sslam {

// ------------------------------------------------------------------------------------------------
// Blocks of H^-1 = (L L^T)^-1 along elimination-tree paths (computeLandmarkMarginals, reference src/ps_graph_slam/graph_slam.cpp:221-234
// -> g2o MarginalCovarianceCholesky; sslam_batch_marginals).  Z(w, w) = E_w^T L^-T L^-1 E_w = Y^T Y with Y = L^-1 E_w, and Y is non-zero
// only on the PATH from w's column to the root of the elimination tree; every off-diagonal block of a column on that path has its row
// further up the same path (struct(k) is a subset of the ancestors of k).  marginal_path_forward: one wave walks the path bottom-up with a
// right-looking forward substitution: finalise Y_s = L_ss^-1 acc_s, then every block (i, path[s]) of the column subtracts L(i, s) Y_s from
// acc_i -- one lane per block, distinct rows, no conflicts, fixed order.  Work O(path^2) per vertex instead of two triangular solves over
// the whole factor per right-hand side column.  Needs the flat factor (chol_factor_and_forward(b, true)).
// cols: the P columns of the path; D = d(w); Y: P x 36; sD: the diagonal block of a step, 36; prec: {first block, blocks, diagonal offset,
// dim} P x int4; pyoff: y offsets P x int.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void marginal_path_forward(const CholView& C, const int* __restrict__ cols, int P, int D, double* Y, double* sD,
                                                      int4* prec, int* pyoff) {
  const int lane = threadIdx.x;
  const double* __restrict__ L = C.Lval;
  for (int t = lane; t < P; t += 64) {
    const ColMeta cm = C.col[cols[t]];
    prec[t] = make_int4(cm.b0, cm.nb, cm.base, cm.dim);
    pyoff[t] = cm.yoff;
  }
  for (int e = lane; e < P * 36; e += 64) Y[e] = 0.0;
  __syncthreads();
  if (lane < D) Y[lane * 6 + lane] = 1.0;   // E_w: identity in the vertex' own rows (path entry 0)
  __syncthreads();
  for (int s = 0; s < P; ++s) {
    const int4 pr = prec[s];
    const int da = pr.w;
    if (lane < da * da) sD[lane] = L[pr.z + lane];
    __syncthreads();
    if (lane < D) {   // one lane per right-hand side column: Y_s = L_ss^-1 acc_s
      double yv[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (i < da) {
          double a = Y[s * 36 + i * 6 + lane];
#pragma unroll
          for (int m = 0; m < 6; ++m) if (m < i) a -= sD[i * da + m] * yv[m];
          yv[i] = a / sD[i * da + i];
          Y[s * 36 + i * 6 + lane] = yv[i];
        }
      }
    }
    __syncthreads();
    for (int bq = lane; bq < pr.y - 1; bq += 64) {   // the blocks below the diagonal: acc_t -= L(t, s) Y_s
      const BlkMeta bm = C.blk[pr.x + 1 + bq];
      const int di = bm.info & 15;
      int lo = s + 1, hi = P - 1;                    // the row's place on the path (y offsets ascend along it)
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (pyoff[mid] < bm.yoff_row) lo = mid + 1; else hi = mid; }
      const double* Lb = L + bm.off;
      double* acc = Y + lo * 36;
      for (int i = 0; i < di; ++i) {
        double lrow[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) lrow[m] = m < da ? Lb[i * da + m] : 0.0;
        for (int c = 0; c < D; ++c) {
          double a = 0;
#pragma unroll
          for (int m = 0; m < 6; ++m) a += lrow[m] * Y[s * 36 + m * 6 + c];   // rows >= da of Y_s are zero
          acc[i * 6 + c] -= a;
        }
      }
    }
    __syncthreads();
  }
}

// Z(u, v) for (row vertex, column vertex) PAIRS, diagonal or not, and for paths of any length.  Z(u, v) = Y_u^T Y_v: the product runs over
// the columns the two paths share -- in a tree their common suffix, from the lowest common ancestor to the root (none when u and v lie
// in different components: zeros).  One wave per request: marginal_path_forward along path(u), then, for u != v, along path(v), then the
// sum over the suffix.  A request with u == v keeps ONE Y (the whole LDS budget for its one path).
// SCRATCH = false: Y and the path records in LDS [diagonal block 36 | Y: ylen x 36 | records ylen x int4 | y offsets ylen x int].
// SCRATCH = true: the same three arrays in the request's slice of a device buffer (req[7], in units of 16 bytes), for paths that LDS does
// not hold; only the diagonal block stays in LDS.  Same body, same order of operations: the two placements agree bitwise.  The wave is the
// whole workgroup, its lanes hand Y to one another between the phases of a step: the workgroup-scope release / acquire of __syncthreads()
// orders plain global stores and loads of one workgroup as it orders LDS (its waves share the CU's L1; the compiler waits for the stores
// before the barrier).
// req: the records of path_rounds.hpp, 8 ints per request (length 0 of path(v): u == v).  out: [requests][36], the leading d(u) x d(v)
// entries row-major.
// path_place: the three arrays of request q behind the `fixed` doubles of LDS (ylen entries each), or in its scratch slice (Pu + Pv each)
template <bool SCRATCH>
__device__ __forceinline__ void path_place(double* sm, int fixed, const int* __restrict__ q, int ylen, char* scratch, double*& Y, int4*& prec,
                                           int*& pyoff) {
  const int yl = SCRATCH ? q[1] + q[3] : ylen;
  Y = SCRATCH ? reinterpret_cast<double*>(scratch + (size_t)q[7] * 16) : sm + fixed;
  prec = reinterpret_cast<int4*>(Y + (size_t)yl * 36);
  pyoff = reinterpret_cast<int*>(prec + yl);
}

// Entry (a, c) of Ya^T Yb over n path entries, in path order
__device__ __forceinline__ double path_yty(const double* Ya, const double* Yb, int n, int a, int c) {
  double z = 0;
  for (int t = 0; t < n; ++t)
#pragma unroll
    for (int i = 0; i < 6; ++i) z += Ya[t * 36 + i * 6 + a] * Yb[t * 36 + i * 6 + c];
  return z;
}

template <bool SCRATCH>
__global__ __launch_bounds__(64) void k_chol_marginal_pairs(CholView C, const int* __restrict__ req, const int* __restrict__ path_cols,
                                                            double* __restrict__ out, int ylen, char* scratch) {
  extern __shared__ double sm[];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int* __restrict__ q = req + (size_t)r * 8;
  const int Pu = q[1], Pv = q[3], Du = q[4], Dv = q[5], nc = q[6];
  double* sD = sm;
  double* Y; int4* prec; int* pyoff;
  path_place<SCRATCH>(sm, 36, q, ylen, scratch, Y, prec, pyoff);
  marginal_path_forward(C, path_cols + q[0], Pu, Du, Y, sD, prec, pyoff);
  if (Pv > 0) marginal_path_forward(C, path_cols + q[2], Pv, Dv, Y + (size_t)Pu * 36, sD, prec + Pu, pyoff + Pu);
  // the common suffix: its first entry in either path (u == v: the whole path, nc == Pu)
  const double* Yu = Y + (size_t)(Pu - nc) * 36;
  const double* Yv = Pv > 0 ? Y + (size_t)(Pu + Pv - nc) * 36 : Yu;
  if (lane < Du * Dv) {
    const int rr = lane / Dv, cc = lane - rr * Dv;
    out[(size_t)r * 36 + lane] = path_yty(Yu, Yv, nc, rr, cc);
  }
}

// ------------------------------------------------------------------------------------------------
// Mahalanobis gate of candidate edges (sslam_batch_gate): d2 = e^T S^-1 e with S = Ju Zuu Ju^T + Ju Zuv Jv^T + Jv Zvu Ju^T + Jv Zvv Jv^T
// + Omega^-1, for an EdgeSE3 (u, v poses) or an EdgeSE3PointXYZ (u pose, v point) that is NOT in the graph.  One wave per candidate:
// marginal_path_forward along path(u) and along path(v), each ONCE; the three blocks Zuu, Zvv (whole paths) and Zuv (common suffix) out of
// the two Ys; e and the analytic Jacobians of sslam_math.hpp at the estimates the device holds; Omega^-1 and S^-1 e through 6 x 6 / 3 x 3
// Choleskys.  Only d2, e and S cross PCIe.
// A fixed or edge-less end has no column: its path has length 0, nothing of Y / prec / pyoff is touched for it and its blocks are zero.
// Placement as in k_chol_marginal_pairs, with a fixed LDS area after the diagonal block in both placements:
//   [diagonal block 36 | Zuu 36 | Zuv 36 | Zvv 36 | Ju 36 | Jv 36 | S 36 | Omega / its factor 36 | e 6, flags 2 | Y ... ]
// (the 6 x 6 areas hold rows of stride 6, S and Omega rows of stride d).  Same body, same order of operations: the placements agree bitwise.
// req: the records of path_rounds.hpp, kGateReq ints per candidate (length 0: no column), the payload {kind, index of u in pose, index of
// v in pose / lmk, Omega given}.  in: [candidates][kGateIO] = z 7, pad, Omega 36.  out: [candidates][kGateIO] = d2, e 6, pad, S 36.
// ------------------------------------------------------------------------------------------------
constexpr int kGateReq = 12, kGateIO = 44;
constexpr int kGateZuu = 36, kGateZuv = 72, kGateZvv = 108, kGateJu = 144, kGateJv = 180, kGateS = 216, kGateW = 252, kGateE = 288;
constexpr int kGateFixed = 296;   // doubles of the fixed LDS area, the diagonal block included

// in-place Cholesky of the d x d matrix A (rows of stride d, lower triangle read and written) by ONE lane; false: a pivot <= 0 or not finite
__device__ __forceinline__ bool gate_chol_small(double* A, int d) {
  for (int j = 0; j < d; ++j) {
    double p = A[j * d + j];
    for (int m = 0; m < j; ++m) p -= A[j * d + m] * A[j * d + m];
    if (!(p > 0.0) || !isfinite(p)) return false;
    p = sqrt(p);
    A[j * d + j] = p;
    for (int i = j + 1; i < d; ++i) {
      double a = A[i * d + j];
      for (int m = 0; m < j; ++m) a -= A[i * d + m] * A[j * d + m];
      A[i * d + j] = a / p;
    }
  }
  return true;
}

template <bool SCRATCH>
__global__ __launch_bounds__(64) void k_chol_gate_pairs(CholView C, const int* __restrict__ req, const int* __restrict__ path_cols,
                                                        const double* __restrict__ in, const double* __restrict__ pose,
                                                        const double* __restrict__ lmk, double* __restrict__ out, int ylen, char* scratch) {
  extern __shared__ double sm[];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int* __restrict__ q = req + (size_t)r * kGateReq;
  const int Pu = q[1], Pv = q[3], Du = q[4], Dv = q[5], nc = q[6];
  const bool se3 = q[8] == SSLAM_GATE_SE3, has_info = q[11] != 0;
  const int d = se3 ? 6 : 3;
  const double* __restrict__ zin = in + (size_t)r * kGateIO;
  double* o = out + (size_t)r * kGateIO;
  double* sD = sm;
  double* Y; int4* prec; int* pyoff;
  path_place<SCRATCH>(sm, kGateFixed, q, ylen, scratch, Y, prec, pyoff);
  for (int k = 36 + lane; k < kGateFixed; k += 64) sm[k] = 0.0;
  // 1. the two paths, each once; a side without a column is skipped whole
  if (Pu > 0) marginal_path_forward(C, path_cols + q[0], Pu, Du, Y, sD, prec, pyoff);
  if (Pv > 0) marginal_path_forward(C, path_cols + q[2], Pv, Dv, Y + (size_t)Pu * 36, sD, prec + Pu, pyoff + Pu);
  __syncthreads();
  // 2. Zuu, Zvv over the whole paths, Zuv over the common suffix (nc == 0: different components, or a side without a column)
  if (lane < 36) {
    const int a = lane / 6, c = lane - a * 6;
    const double* Yu = Y;
    const double* Yv = Y + (size_t)Pu * 36;
    sm[kGateZuu + lane] = a < Du && c < Du ? path_yty(Yu, Yu, Pu, a, c) : 0.0;
    sm[kGateZvv + lane] = a < Dv && c < Dv ? path_yty(Yv, Yv, Pv, a, c) : 0.0;
    sm[kGateZuv + lane] = a < Du && c < Dv ? path_yty(Yu + (size_t)(Pu - nc) * 36, Yv + (size_t)(Pv - nc) * 36, nc, a, c) : 0.0;
  }
  // 3. e and the Jacobians at the estimates the device holds
  const Pose Xu = load_pose(pose, q[9]);
  if (se3) {
    const Pose Xv = load_pose(pose, q[10]);
    const Pose Z{{zin[0], zin[1], zin[2]}, {zin[3], zin[4], zin[5], zin[6]}};
    Se3Lin L;
    se3_error(Xu, Xv, Z, L);
    L.Re = qmat(L.qe);
    if (lane < 12) {   // one lane per Jacobian column
      double col[6];
      if (lane < 6) se3_Ji_col(L, lane, col);
      else se3_Jj_col(L, lane - 6, col);
      double* J = sm + (lane < 6 ? kGateJu + lane : kGateJv + lane - 6);
#pragma unroll
      for (int i = 0; i < 6; ++i) J[i * 6] = col[i];
    } else if (lane == 12) {
#pragma unroll
      for (int i = 0; i < 6; ++i) sm[kGateE + i] = L.e[i];
    }
  } else {
    const double* lp = lmk + (size_t)q[10] * 4;
    PointLin L;
    point_error(Xu, Vec3{lp[0], lp[1], lp[2]}, Vec3{zin[0], zin[1], zin[2]}, L);
    if (lane == 0) {
      double Ji[18], Jl[9];
      point_jacobians(L, Ji, Jl);
#pragma unroll
      for (int k = 0; k < 18; ++k) sm[kGateJu + k] = Ji[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) sm[kGateJv + (k / 3) * 6 + k % 3] = Jl[k];
    } else if (lane == 12) {
#pragma unroll
      for (int i = 0; i < 3; ++i) sm[kGateE + i] = L.e[i];
    }
  }
  // 4. Omega^-1: Cholesky by one lane, then one lane per column of the inverse -> sD (free after the paths)
  if (has_info && lane < d * d) sm[kGateW + lane] = zin[8 + lane];
  __syncthreads();
  if (has_info && lane == 0) sm[kGateE + 6] = gate_chol_small(sm + kGateW, d) ? 1.0 : 0.0;
  __syncthreads();
  const bool w_ok = !has_info || sm[kGateE + 6] != 0.0;
  if (has_info && w_ok && lane < d) {
    const double* W = sm + kGateW;
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // L y = unit vector `lane`
      if (i < d) {
        double a = i == lane ? 1.0 : 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) if (m < i) a -= W[i * d + m] * x[m];
        x[i] = a / W[i * d + i];
      }
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {   // L^T x = y
      if (i < d) {
        double a = x[i];
#pragma unroll
        for (int m = 5; m >= 0; --m) if (m > i && m < d) a -= W[m * d + i] * x[m];
        x[i] = a / W[i * d + i];
        sD[i * d + lane] = x[i];
      }
    }
  }
  __syncthreads();
  // S by lanes < d * d; entry (r, c) and entry (c, r) run the same sums: S is symmetric to the bit
  if (lane < 36) {
    double s = 0;
    if (lane < d * d) {
      const int r0 = lane / d, c0 = lane - r0 * d;
      const int hi = r0 > c0 ? r0 : c0, lo = r0 > c0 ? c0 : r0;
      const double *Ju = sm + kGateJu, *Jv = sm + kGateJv;
      for (int a = 0; a < Du; ++a)
        for (int c = 0; c < Du; ++c) s += Ju[hi * 6 + a] * sm[kGateZuu + a * 6 + c] * Ju[lo * 6 + c];
      for (int a = 0; a < Du; ++a)
        for (int c = 0; c < Dv; ++c) s += Ju[hi * 6 + a] * sm[kGateZuv + a * 6 + c] * Jv[lo * 6 + c];
      for (int a = 0; a < Dv; ++a)
        for (int c = 0; c < Du; ++c) s += Jv[hi * 6 + a] * sm[kGateZuv + c * 6 + a] * Ju[lo * 6 + c];
      for (int a = 0; a < Dv; ++a)
        for (int c = 0; c < Dv; ++c) s += Jv[hi * 6 + a] * sm[kGateZvv + a * 6 + c] * Jv[lo * 6 + c];
      if (has_info && w_ok) s += sD[hi * d + lo];
      sm[kGateS + lane] = s;
    }
    o[8 + lane] = s;
  }
  __syncthreads();
  // 5. Cholesky of S, forward substitution, d2 = |L^-1 e|^2
  if (lane == 0) {
    double* S = sm + kGateS;
    double* y = sm + kGateW;
    double d2 = __longlong_as_double(0x7ff8000000000000ll);   // NaN: Omega or S broke down
    if (w_ok && gate_chol_small(S, d)) {
      d2 = 0;
      for (int i = 0; i < d; ++i) {
        double a = sm[kGateE + i];
        for (int m = 0; m < i; ++m) a -= S[i * d + m] * y[m];
        y[i] = a / S[i * d + i];
        d2 += y[i] * y[i];
      }
    }
    o[0] = d2;
    o[7] = 0.0;
  } else if (lane <= 6) {
    o[lane] = lane - 1 < d ? sm[kGateE + lane - 1] : 0.0;
  }
}


}  // namespace sslam
