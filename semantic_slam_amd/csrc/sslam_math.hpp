// Fixed-size FP64 geometry for the ps_graph_slam hot path on gfx950 (device + host).
//
// Restates the g2o types the reference instantiates:
//   VertexSE3 / EdgeSE3            <- reference src/ps_graph_slam/graph_slam.cpp:104-115,136-148
//   VertexPointXYZ / EdgeSE3PointXYZ (offset id 0 = identity, :75-83,150-166)
//   VertexPlane / EdgeSE3Plane     <- reference include/g2o/edge_se3_plane.hpp:8-48
// Poses are stored as translation + unit quaternion (x,y,z,w); increments are g2o's "MQT"
// minimal vectors [dt, dq_xyz] applied on the right:  X <- X * fromVectorMQT(d).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define SSLAM_HD __host__ __device__ __forceinline__

namespace sslam {

struct Vec3 {
  double x, y, z;
};
struct Quat {
  double x, y, z, w;
};
struct Pose {
  Vec3 t;
  Quat q;
};

SSLAM_HD Vec3 operator+(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
SSLAM_HD Vec3 operator-(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
SSLAM_HD Vec3 operator*(double s, Vec3 a) { return {s * a.x, s * a.y, s * a.z}; }
SSLAM_HD double dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
SSLAM_HD Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

SSLAM_HD Quat qmul(Quat a, Quat b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w,
          a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
SSLAM_HD Quat qconj(Quat a) { return {-a.x, -a.y, -a.z, a.w}; }

// 3x3 rotation matrix, row-major m[r*3+c]
struct Mat3 {
  double m[9];
};
SSLAM_HD Mat3 qmat(Quat q) {
  Mat3 R;
  const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z;
  const double xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z;
  const double wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
  R.m[0] = 1 - 2 * (yy + zz); R.m[1] = 2 * (xy - wz);     R.m[2] = 2 * (xz + wy);
  R.m[3] = 2 * (xy + wz);     R.m[4] = 1 - 2 * (xx + zz); R.m[5] = 2 * (yz - wx);
  R.m[6] = 2 * (xz - wy);     R.m[7] = 2 * (yz + wx);     R.m[8] = 1 - 2 * (xx + yy);
  return R;
}
SSLAM_HD Vec3 mul(const Mat3& R, Vec3 v) {
  return {R.m[0] * v.x + R.m[1] * v.y + R.m[2] * v.z, R.m[3] * v.x + R.m[4] * v.y + R.m[5] * v.z,
          R.m[6] * v.x + R.m[7] * v.y + R.m[8] * v.z};
}
SSLAM_HD Vec3 mulT(const Mat3& R, Vec3 v) {
  return {R.m[0] * v.x + R.m[3] * v.y + R.m[6] * v.z, R.m[1] * v.x + R.m[4] * v.y + R.m[7] * v.z,
          R.m[2] * v.x + R.m[5] * v.y + R.m[8] * v.z};
}
SSLAM_HD Vec3 qrot(Quat q, Vec3 v) { return mul(qmat(q), v); }

// VertexSE3::oplus
SSLAM_HD Pose se3_oplus(Pose X, const double d[6]) {
  const double w2 = 1.0 - (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  Quat dq;
  if (w2 < 0) dq = {0, 0, 0, 1};
  else dq = {d[3], d[4], d[5], sqrt(w2)};
  Pose Y;
  Y.t = X.t + qrot(X.q, Vec3{d[0], d[1], d[2]});
  Quat q = qmul(X.q, dq);
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  Y.q = {q.x / n, q.y / n, q.z / n, q.w / n};
  return Y;
}

// ---------------------------------------------------------------------------------------------
// EdgeSE3: e = toVectorMQT(Z^-1 * Xi^-1 * Xj).  Intermediate terms kept for the Jacobians.
struct Se3Lin {
  double e[6];
  Mat3 Ra;   // rotation of Z^-1
  Mat3 Re;   // rotation of E
  Vec3 tb;   // translation of Xi^-1 Xj
  Quat qa;   // Z^-1 rotation
  Quat qb;   // rotation of Xi^-1 Xj
  Quat qe;   // rotation of E (un-normalised sign)
  double s;  // +1 / -1 so that the reported quaternion has w >= 0
};

SSLAM_HD void se3_error(const Pose& Xi, const Pose& Xj, const Pose& Z, Se3Lin& L) {
  L.qa = qconj(Z.q);
  const Quat qii = qconj(Xi.q);
  L.tb = qrot(qii, Xj.t - Xi.t);
  L.qb = qmul(qii, Xj.q);
  L.Ra = qmat(L.qa);
  const Vec3 te = mul(L.Ra, L.tb - Z.t);
  L.qe = qmul(L.qa, L.qb);
  L.s = L.qe.w < 0 ? -1.0 : 1.0;
  L.e[0] = te.x; L.e[1] = te.y; L.e[2] = te.z;
  L.e[3] = L.s * L.qe.x; L.e[4] = L.s * L.qe.y; L.e[5] = L.s * L.qe.z;
}

// Column c (0..5) of d e / d delta_i, written to col[6].
//   translation rows: [-Ra | 2 Ra [tb]x];  rotation rows: [0 | -s * xyz(qa (e_k,0) qb)]
SSLAM_HD double pick3(int k, double a, double b, double c) { return k == 0 ? a : (k == 1 ? b : c); }
SSLAM_HD void se3_Ji_col(const Se3Lin& L, int c, double col[6]) {
  if (c < 3) {  // (no dynamic indexing: keeps the matrices in registers)
    col[0] = -pick3(c, L.Ra.m[0], L.Ra.m[1], L.Ra.m[2]);
    col[1] = -pick3(c, L.Ra.m[3], L.Ra.m[4], L.Ra.m[5]);
    col[2] = -pick3(c, L.Ra.m[6], L.Ra.m[7], L.Ra.m[8]);
    col[3] = col[4] = col[5] = 0;
  } else {
    const int k = c - 3;
    // column k of [tb]x
    Vec3 sk = k == 0 ? Vec3{0, L.tb.z, -L.tb.y} : (k == 1 ? Vec3{-L.tb.z, 0, L.tb.x} : Vec3{L.tb.y, -L.tb.x, 0});
    const Vec3 a = mul(L.Ra, sk);
    col[0] = 2 * a.x; col[1] = 2 * a.y; col[2] = 2 * a.z;
    const Quat vk = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, 0.0};
    const Quat t = qmul(qmul(L.qa, vk), L.qb);
    col[3] = -L.s * t.x; col[4] = -L.s * t.y; col[5] = -L.s * t.z;
  }
}
// Column c of d e / d delta_j:  [[Re, 0], [0, s (w I + [q_xyz]x)]]
SSLAM_HD void se3_Jj_col(const Se3Lin& L, int c, double col[6]) {
  if (c < 3) {
    col[0] = pick3(c, L.Re.m[0], L.Re.m[1], L.Re.m[2]);
    col[1] = pick3(c, L.Re.m[3], L.Re.m[4], L.Re.m[5]);
    col[2] = pick3(c, L.Re.m[6], L.Re.m[7], L.Re.m[8]);
    col[3] = col[4] = col[5] = 0;
  } else {
    const int k = c - 3;
    const double w = L.qe.w, x = L.qe.x, y = L.qe.y, z = L.qe.z;
    col[0] = col[1] = col[2] = 0;
    if (k == 0) { col[3] = L.s * w; col[4] = L.s * z; col[5] = -L.s * y; }
    else if (k == 1) { col[3] = -L.s * z; col[4] = L.s * w; col[5] = L.s * x; }
    else { col[3] = L.s * y; col[4] = -L.s * x; col[5] = L.s * w; }
  }
}
SSLAM_HD void se3_full_jacobians(Se3Lin& L, double Ji[36], double Jj[36]) {  // row-major 6x6
  L.Re = qmat(L.qe);
  for (int c = 0; c < 6; ++c) {
    double a[6], b[6];
    se3_Ji_col(L, c, a);
    se3_Jj_col(L, c, b);
    for (int r = 0; r < 6; ++r) { Ji[r * 6 + c] = a[r]; Jj[r * 6 + c] = b[r]; }
  }
}

// ---------------------------------------------------------------------------------------------
// EdgeSE3PointXYZ with identity sensor offset: e = Ri^T (p - ti) - z
struct PointLin {
  double e[3];
  Vec3 pc;
  Mat3 R;  // rotation of Xi
};
SSLAM_HD void point_error(const Pose& Xi, Vec3 p, Vec3 z, PointLin& L) {
  L.R = qmat(Xi.q);
  L.pc = mulT(L.R, p - Xi.t);
  L.e[0] = L.pc.x - z.x; L.e[1] = L.pc.y - z.y; L.e[2] = L.pc.z - z.z;
}
// Ji = [-I | 2[pc]x] (3x6 row-major), Jl = Ri^T (3x3 row-major)
SSLAM_HD void point_jacobians(const PointLin& L, double Ji[18], double Jl[9]) {
  for (int k = 0; k < 18; ++k) Ji[k] = 0;
  Ji[0] = -1; Ji[7] = -1; Ji[14] = -1;
  Ji[4] = -2 * L.pc.z; Ji[5] = 2 * L.pc.y;
  Ji[6 + 3] = 2 * L.pc.z; Ji[6 + 5] = -2 * L.pc.x;
  Ji[12 + 3] = -2 * L.pc.y; Ji[12 + 4] = 2 * L.pc.x;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Jl[r * 3 + c] = L.R.m[c * 3 + r];
}

// ---------------------------------------------------------------------------------------------
// Plane3D helpers (g2o slam3d_addons): plane = (n, d), n.x + d = 0, distance() = -d
struct Plane {
  Vec3 n;
  double d;
};
SSLAM_HD double pl_azimuth(Vec3 n) { return atan2(n.y, n.x); }
SSLAM_HD double pl_elevation(Vec3 n) { return atan2(n.z, sqrt(n.x * n.x + n.y * n.y)); }
// Rz(azimuth) * Ry(-elevation).  g2o's Plane3D::rotation() goes through the two angles (atan2, then cos / sin of them); the cosines and sines
// of atan2(y, x) and atan2(z, r) ARE x / r, y / r and r / |n|, z / |n|: taken from the components here (round 6) -- the same matrix to an ulp per
// entry, two atan2 and two sincos (700 of the 1,190 FP64 instructions of an error evaluation) less.  A plane edge evaluates its error 19
// times per linearisation (central differences); the rounding noise of such a Jacobian (1e-16 / 2e-9) is the same either way, and is what
// the 2e-5 of the plane parity tests allow for since round 1 (host libm and device ocml differ by an ulp as well).
SSLAM_HD Mat3 pl_rotation(Vec3 n) {
  const double r2 = n.x * n.x + n.y * n.y;
  const double r = sqrt(r2), nn = sqrt(r2 + n.z * n.z);
  const double ca = r > 0 ? n.x / r : 1.0, sa = r > 0 ? n.y / r : 0.0;          // atan2(0, 0) = 0
  const double cb = nn > 0 ? r / nn : 1.0, sb = nn > 0 ? -n.z / nn : 0.0;       // cos(-el) = cos(el), sin(-el) = -sin(el)
  Mat3 R;
  R.m[0] = ca * cb; R.m[1] = -sa; R.m[2] = ca * sb;
  R.m[3] = sa * cb; R.m[4] = ca;  R.m[5] = sa * sb;
  R.m[6] = -sb;     R.m[7] = 0;   R.m[8] = cb;
  return R;
}
SSLAM_HD Plane pl_oplus(Plane p, const double v[3]) {
  const Mat3 R = pl_rotation(p.n);
  const Vec3 s = {cos(v[1]) * cos(v[0]), cos(v[1]) * sin(v[0]), sin(v[1])};
  Vec3 n = mul(R, s);
  double d = -(-p.d + v[2]);
  const double nn = sqrt(dot(n, n));
  return {{n.x / nn, n.y / nn, n.z / nn}, d / nn};
}
// EdgeSE3Plane::computeError: (Xi^-1 ∘ pi_w) ⊖ z
SSLAM_HD void plane_error(const Pose& Xi, Plane pw, Plane z, double e[3]) {
  const Quat qi = qconj(Xi.q);
  const Vec3 ti = -1.0 * qrot(qi, Xi.t);
  const Vec3 n = qrot(qi, pw.n);
  const double d = pw.d - dot(ti, n);
  const Vec3 m = mulT(pl_rotation(n), z.n);
  e[0] = pl_azimuth(m); e[1] = pl_elevation(m); e[2] = -d + z.d;
}
// g2o BaseBinaryEdge numeric Jacobian: central differences, delta = 1e-9
SSLAM_HD void plane_jacobians(const Pose& Xi, Plane pw, Plane z, double Ji[18], double Jl[9]) {
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  for (int d = 0; d < 6; ++d) {
    double dv[6] = {0, 0, 0, 0, 0, 0}, ep[3], em[3];
    dv[d] = delta;  plane_error(se3_oplus(Xi, dv), pw, z, ep);
    dv[d] = -delta; plane_error(se3_oplus(Xi, dv), pw, z, em);
    for (int r = 0; r < 3; ++r) Ji[r * 6 + d] = scalar * (ep[r] - em[r]);
  }
  for (int d = 0; d < 3; ++d) {
    double dv[3] = {0, 0, 0}, ep[3], em[3];
    dv[d] = delta;  plane_error(Xi, pl_oplus(pw, dv), z, ep);
    dv[d] = -delta; plane_error(Xi, pl_oplus(pw, dv), z, em);
    for (int r = 0; r < 3; ++r) Jl[r * 3 + d] = scalar * (ep[r] - em[r]);
  }
}

// ---- absolute orientation (the update of sslam_seg_register_pairs) -------------------------------------------------------------------
// One Jacobi rotation of the symmetric 4 x 4 matrix A in the (P, Q) plane, A <- J^T A J, accumulated into V <- V J.  P and Q are
// template parameters and every loop is unrolled, so that no array is indexed at run time (A and V stay in registers on the device).
template <int P, int Q>
SSLAM_HD void jacobi4_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi / 4
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
  }
  A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
  }
}
// The rigid transform (R, t) minimising sum |R p + t - q|^2 over n >= 3 correspondences, from their plain sums n, sum p, sum q and
// M = sum p q^T (Mab = sum p_a q_b).  T: R row-major, then t.  Horn's closed form (J. Opt. Soc. Am. A 4 (1987) 629): with the
// cross-covariance S = M - (sum p)(sum q)^T / n, the unit quaternion of R is the eigenvector of the largest eigenvalue of the symmetric
//   N = | Sxx+Syy+Szz   Syz-Szy        Szx-Sxz        Sxy-Syx      |
//       | Syz-Szy       Sxx-Syy-Szz    Sxy+Syx        Szx+Sxz      |
//       | Szx-Sxz       Sxy+Syx       -Sxx+Syy-Szz    Syz+Szy      |
//       | Sxy-Syx       Szx+Sxz        Syz+Szy       -Sxx-Syy+Szz  |     (order w, x, y, z),
// found by cyclic Jacobi sweeps; t = mean q - R mean p.  R comes from a unit quaternion, so it is a proper rotation whatever the
// correspondences are (coplanar ones too, where the SVD form needs its determinant correction): it is the minimiser over rotations,
// which is what pcl::TransformationEstimationSVD computes.  The eigenvalues of N are s1+s2+s3', s1-s2-s3', -s1+s2-s3', -s1-s2+s3' for
// the singular values s1 >= s2 >= s3 of S (s3' = s3 times the sign of det S): the largest is simple unless s2 = -s3', i.e. for
// collinear correspondences (s2 = s3 = 0), where the rotation about the line is undetermined and the column Jacobi happens to end
// at is returned, one of the minimisers.
SSLAM_HD void horn_rigid(double n, double px, double py, double pz, double qx, double qy, double qz, double Mxx, double Mxy, double Mxz, double Myx,
                         double Myy, double Myz, double Mzx, double Mzy, double Mzz, double T[12]) {
  const double Sxx = Mxx - px * qx / n, Sxy = Mxy - px * qy / n, Sxz = Mxz - px * qz / n;
  const double Syx = Myx - py * qx / n, Syy = Myy - py * qy / n, Syz = Myz - py * qz / n;
  const double Szx = Mzx - pz * qx / n, Szy = Mzy - pz * qy / n, Szz = Mzz - pz * qz / n;
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {   // quadratic convergence: 6 to 8 sweeps in practice
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
    if (off <= 1e-40 * dia) break;
    jacobi4_rotate<0, 1>(A, V); jacobi4_rotate<0, 2>(A, V); jacobi4_rotate<0, 3>(A, V);
    jacobi4_rotate<1, 2>(A, V); jacobi4_rotate<1, 3>(A, V); jacobi4_rotate<2, 3>(A, V);
  }
  // the column of the largest eigenvalue (the first among equals), picked with 0 / 1 weights: exact, and unlike a chain of conditional
  // copies the compiler cannot turn it into a run-time index into V, which would put V into scratch memory
  double best = A[0][0];
  int kb = 0;
  if (A[1][1] > best) { best = A[1][1]; kb = 1; }
  if (A[2][2] > best) { best = A[2][2]; kb = 2; }
  if (A[3][3] > best) { best = A[3][3]; kb = 3; }
  const double m0 = kb == 0 ? 1.0 : 0.0, m1 = kb == 1 ? 1.0 : 0.0, m2 = kb == 2 ? 1.0 : 0.0, m3 = kb == 3 ? 1.0 : 0.0;
  const double w = (m0 * V[0][0] + m1 * V[0][1]) + (m2 * V[0][2] + m3 * V[0][3]);
  const double x = (m0 * V[1][0] + m1 * V[1][1]) + (m2 * V[1][2] + m3 * V[1][3]);
  const double y = (m0 * V[2][0] + m1 * V[2][1]) + (m2 * V[2][2] + m3 * V[2][3]);
  const double z = (m0 * V[3][0] + m1 * V[3][1]) + (m2 * V[3][2] + m3 * V[3][3]);
  const double nq = sqrt(w * w + x * x + y * y + z * z);
  const Mat3 R = qmat(Quat{x / nq, y / nq, z / nq, w / nq});
  const Vec3 pm = {px / n, py / n, pz / n}, qm = {qx / n, qy / n, qz / n};
  const Vec3 t = qm - mul(R, pm);
#pragma unroll
  for (int k = 0; k < 9; ++k) T[k] = R.m[k];
  T[9] = t.x; T[10] = t.y; T[11] = t.z;
}

// ---- point-to-plane ICP (sslam_seg_icp_point_to_plane on the host, k_icp_frame_step on the device) -----------------------------------
// One Gauss-Newton step from the 29 sums of a pass: J^T J (upper triangle by rows, 21), J^T r (6), r^2, the point count.
// (J^T J) delta = -J^T r by Cholesky, two triangular solves, then T <- (exp[w]x, u) o T with Rodrigues' formula; T: R row-major, then
// t.  Returns false and leaves T alone when the system is rank deficient (planes with fewer than three independent normals leave the
// transform free along some direction).
SSLAM_HD bool icp_gn_step(const double sums[29], double T[12]) {
  double A[36], bvec[6], L[36];
  for (int k = 0; k < 36; ++k) L[k] = 0;
  int m = 0;
  for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { A[r * 6 + c] = A[c * 6 + r] = sums[m++]; }
  for (int r = 0; r < 6; ++r) bvec[r] = -sums[21 + r];
  for (int j = 0; j < 6; ++j) {
    double dsum = A[j * 6 + j];
    for (int k = 0; k < j; ++k) dsum -= L[j * 6 + k] * L[j * 6 + k];
    if (!(dsum > 1e-12 * A[j * 6 + j]) || !(dsum > 0)) return false;
    L[j * 6 + j] = sqrt(dsum);
    for (int i = j + 1; i < 6; ++i) { double v = A[i * 6 + j]; for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k]; L[i * 6 + j] = v / L[j * 6 + j]; }
  }
  double y[6], dx[6];
  for (int i = 0; i < 6; ++i) { double v = bvec[i]; for (int k = 0; k < i; ++k) v -= L[i * 6 + k] * y[k]; y[i] = v / L[i * 6 + i]; }
  for (int i = 5; i >= 0; --i) { double v = y[i]; for (int k = i + 1; k < 6; ++k) v -= L[k * 6 + i] * dx[k]; dx[i] = v / L[i * 6 + i]; }
  const double wx = dx[0], wy = dx[1], wz = dx[2], th = sqrt(wx * wx + wy * wy + wz * wz);
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (th > 0) {
    const double sa = sin(th) / th, bq = (1.0 - cos(th)) / (th * th);
    const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { double kk = 0; for (int q = 0; q < 3; ++q) kk += K[r * 3 + q] * K[q * 3 + c]; E[r * 3 + c] += sa * K[r * 3 + c] + bq * kk; }
  }
  double Tn[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Tn[r * 3 + c] = E[r * 3] * T[c] + E[r * 3 + 1] * T[3 + c] + E[r * 3 + 2] * T[6 + c];
    Tn[9 + r] = E[r * 3] * T[9] + E[r * 3 + 1] * T[10] + E[r * 3 + 2] * T[11] + dx[3 + r];
  }
  for (int k = 0; k < 12; ++k) T[k] = Tn[k];
  return true;
}

// ---- generalized ICP (sslam_seg_cloud_covariances, sslam_seg_register_pairs_gicp) ----------------------------------------------------
// jacobi4_rotate for a symmetric 3 x 3 matrix
template <int P, int Q>
SSLAM_HD void jacobi3_rotate(double (&A)[3][3], double (&V)[3][3]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
  }
  A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
  }
}
// fast_gicp's PLANE regularisation of a neighbourhood covariance C (xx xy xz yy yz zz): U diag(l) U^T -> U diag(eps, 1, 1) U^T with eps
// at the smallest eigenvalue, which is I - (1 - eps) n n^T for the unit eigenvector n of that eigenvalue (the first among equal
// diagonal entries after the sweeps: with l0 = l1 any minimiser may come out).  Cyclic Jacobi sweeps, as horn_rigid runs them.
SSLAM_HD void gicp_plane_covariance(const double C[6], double eps, double out[6]) {
  double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-40 * dia) break;
    jacobi3_rotate<0, 1>(A, V); jacobi3_rotate<0, 2>(A, V); jacobi3_rotate<1, 2>(A, V);
  }
  double best = A[0][0];
  int kb = 0;
  if (A[1][1] < best) { best = A[1][1]; kb = 1; }
  if (A[2][2] < best) { best = A[2][2]; kb = 2; }
  const double m0 = kb == 0 ? 1.0 : 0.0, m1 = kb == 1 ? 1.0 : 0.0, m2 = kb == 2 ? 1.0 : 0.0;   // 0 / 1 weights: see horn_rigid
  double x = (m0 * V[0][0] + m1 * V[0][1]) + m2 * V[0][2];
  double y = (m0 * V[1][0] + m1 * V[1][1]) + m2 * V[1][2];
  double z = (m0 * V[2][0] + m1 * V[2][1]) + m2 * V[2][2];
  const double nn = sqrt(x * x + y * y + z * z);
  x /= nn; y /= nn; z /= nn;
  const double w = 1.0 - eps;
  out[0] = 1.0 - w * x * x; out[1] = -w * x * y; out[2] = -w * x * z;
  out[3] = 1.0 - w * y * y; out[4] = -w * y * z; out[5] = 1.0 - w * z * z;
}
// The contribution of one correspondence to a Gauss-Newton pass of generalized ICP.  x = R p + t, r = q - x, M = (Ct + R Cs R^T)^-1 by
// cofactors (both covariances as xx xy xz yy yz zz), J = [ [x]x | -I ] for the left perturbation T <- exp(delta) T, delta = (w, v):
// a[0..20] = J^T M J (upper triangle by rows), a[21..26] = J^T M r, a[27] = r^T M r, a[28] = 1 -- the layout icp_gn_step reads.
SSLAM_HD void gicp_point_sums(const double T[12], const double p[3], const double q[3], const double Cs[6], const double Ct[6], double (&a)[29]) {
  const double x[3] = {(T[0] * p[0] + T[1] * p[1]) + T[2] * p[2] + T[9], (T[3] * p[0] + T[4] * p[1]) + T[5] * p[2] + T[10],
                       (T[6] * p[0] + T[7] * p[1]) + T[8] * p[2] + T[11]};
  const double r[3] = {q[0] - x[0], q[1] - x[1], q[2] - x[2]};
  // B = R Cs, S = Ct + B R^T (symmetric)
  const double cs[3][3] = {{Cs[0], Cs[1], Cs[2]}, {Cs[1], Cs[3], Cs[4]}, {Cs[2], Cs[4], Cs[5]}};
  double B[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) B[i][j] = (T[3 * i] * cs[0][j] + T[3 * i + 1] * cs[1][j]) + T[3 * i + 2] * cs[2][j];
  auto brt = [&](int i, int j) { return (B[i][0] * T[3 * j] + B[i][1] * T[3 * j + 1]) + B[i][2] * T[3 * j + 2]; };
  const double sxx = Ct[0] + brt(0, 0), sxy = Ct[1] + brt(0, 1), sxz = Ct[2] + brt(0, 2), syy = Ct[3] + brt(1, 1), syz = Ct[4] + brt(1, 2),
               szz = Ct[5] + brt(2, 2);
  const double cxx = syy * szz - syz * syz, cxy = sxz * syz - sxy * szz, cxz = sxy * syz - sxz * syy;
  const double cyy = sxx * szz - sxz * sxz, cyz = sxy * sxz - sxx * syz, czz = sxx * syy - sxy * sxy;
  const double det = (sxx * cxx + sxy * cxy) + sxz * cxz;
  const double M[3][3] = {{cxx / det, cxy / det, cxz / det}, {cxy / det, cyy / det, cyz / det}, {cxz / det, cyz / det, czz / det}};
  const double J[3][6] = {{0.0, -x[2], x[1], -1.0, 0.0, 0.0}, {x[2], 0.0, -x[0], 0.0, -1.0, 0.0}, {-x[1], x[0], 0.0, 0.0, 0.0, -1.0}};
  double MJ[3][6], Mr[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int c = 0; c < 6; ++c) MJ[i][c] = (M[i][0] * J[0][c] + M[i][1] * J[1][c]) + M[i][2] * J[2][c];
    Mr[i] = (M[i][0] * r[0] + M[i][1] * r[1]) + M[i][2] * r[2];
  }
  int m = 0;
#pragma unroll
  for (int rr = 0; rr < 6; ++rr)
#pragma unroll
    for (int cc = rr; cc < 6; ++cc) a[m++] = (J[0][rr] * MJ[0][cc] + J[1][rr] * MJ[1][cc]) + J[2][rr] * MJ[2][cc];
#pragma unroll
  for (int rr = 0; rr < 6; ++rr) a[21 + rr] = (J[0][rr] * Mr[0] + J[1][rr] * Mr[1]) + J[2][rr] * Mr[2];
  a[27] = (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
  a[28] = 1.0;
}
// Unit quaternion of a rotation matrix (row-major), the branch with the largest pivot, as INTEGRATION.md section 2 spells it out
SSLAM_HD Quat quat_of_rotation(const double R[9]) {
  Quat q;
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0)                          { const double s = 2 * sqrt(1 + tr);                 q.w = s / 4; q.x = (R[7] - R[5]) / s; q.y = (R[2] - R[6]) / s; q.z = (R[3] - R[1]) / s; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double s = 2 * sqrt(1 + R[0] - R[4] - R[8]); q.x = s / 4; q.w = (R[7] - R[5]) / s; q.y = (R[1] + R[3]) / s; q.z = (R[2] + R[6]) / s; }
  else if (R[4] > R[8])                { const double s = 2 * sqrt(1 + R[4] - R[0] - R[8]); q.y = s / 4; q.w = (R[2] - R[6]) / s; q.x = (R[1] + R[3]) / s; q.z = (R[5] + R[7]) / s; }
  else                                 { const double s = 2 * sqrt(1 + R[8] - R[0] - R[4]); q.z = s / 4; q.w = (R[3] - R[1]) / s; q.x = (R[2] + R[6]) / s; q.y = (R[5] + R[7]) / s; }
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return {q.x / n, q.y / n, q.z / n, q.w / n};
}
// One Gauss-Newton step of generalized ICP from the 29 sums of a pass: H delta = -b by Cholesky (no damping: M is held fixed within the
// pass), R_new = exp([w]x) R passed through its unit quaternion and qmat (R stays a proper rotation after any number of steps),
// t_new = exp([w]x) t + v.  false, with Tn unwritten: a sum that is not finite, fewer than 3 correspondences, a pivot that is not positive.
SSLAM_HD bool gicp_gn_step(const double sums[29], const double T[12], double Tn[12]) {
  bool fin = true;
  for (int k = 0; k < 29; ++k) fin = fin && isfinite(sums[k]);
  if (!fin || sums[28] < 3.0) return false;
  double A[36], L[36];
  for (int k = 0; k < 36; ++k) L[k] = 0;
  int m = 0;
  for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { A[r * 6 + c] = A[c * 6 + r] = sums[m++]; }
  for (int j = 0; j < 6; ++j) {
    double dsum = A[j * 6 + j];
    for (int k = 0; k < j; ++k) dsum -= L[j * 6 + k] * L[j * 6 + k];
    if (!(dsum > 0)) return false;
    L[j * 6 + j] = sqrt(dsum);
    for (int i = j + 1; i < 6; ++i) { double v = A[i * 6 + j]; for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k]; L[i * 6 + j] = v / L[j * 6 + j]; }
  }
  double y[6], dx[6];
  for (int i = 0; i < 6; ++i) { double v = -sums[21 + i]; for (int k = 0; k < i; ++k) v -= L[i * 6 + k] * y[k]; y[i] = v / L[i * 6 + i]; }
  for (int i = 5; i >= 0; --i) { double v = y[i]; for (int k = i + 1; k < 6; ++k) v -= L[k * 6 + i] * dx[k]; dx[i] = v / L[i * 6 + i]; }
  const double wx = dx[0], wy = dx[1], wz = dx[2], th = sqrt(wx * wx + wy * wy + wz * wz);
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (th > 0) {
    const double sa = sin(th) / th, bq = (1.0 - cos(th)) / (th * th);
    const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { double kk = 0; for (int q = 0; q < 3; ++q) kk += K[r * 3 + q] * K[q * 3 + c]; E[r * 3 + c] += sa * K[r * 3 + c] + bq * kk; }
  }
  double Rn[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = E[r * 3] * T[c] + E[r * 3 + 1] * T[3 + c] + E[r * 3 + 2] * T[6 + c];
    Tn[9 + r] = E[r * 3] * T[9] + E[r * 3 + 1] * T[10] + E[r * 3 + 2] * T[11] + dx[3 + r];
  }
  const Mat3 Rq = qmat(quat_of_rotation(Rn));
  for (int k = 0; k < 9; ++k) Tn[k] = Rq.m[k];
  for (int k = 0; k < 12; ++k) if (!isfinite(Tn[k])) return false;
  return true;
}

}  // namespace sslam
