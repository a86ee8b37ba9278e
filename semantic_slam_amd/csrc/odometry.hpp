// Scan-matching odometry (hdl_graph_slam's prefiltering_nodelet and scan_matching_odometry_nodelet [UPSTREAM, quoted from memory]): the
// device code the resident prefilter chain adds to the cloud filters of sslam_seg.hip, and the host-only rules of the odometry handle
// (parameter checks, the 3 x 4 products, the decision rule).  The contract is at sslam_seg_prefilter / sslam_odom_push in include/sslam.h.
// Internal: included by sslam_seg.hip alone, whose entry points launch these kernels through the shared ordered compaction.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/sslam.h"
#include "sslam_common.hpp"
#include "sslam_math.hpp"

namespace sslam {
namespace seg {
// pcl::RadiusOutlierRemoval: the number of OTHER finite points within the radius of every point, exact (brute force).  The shape of
// k_knn_cov without its LDS columns: one thread per query, the cloud streams through an LDS tile of padded 16-byte points (every lane
// reads the same address: a broadcast), the count is an integer in a register.  No early exit: the count is the same whatever the tile
// size.  A non-finite candidate is staged as NaN and fails the compare; the query itself passes it (d2 = 0) and is taken off at the end.
constexpr int kRadThreads = 128;
__global__ __launch_bounds__(kRadThreads) void k_radius_count(const float* __restrict__ pts, int n, float r2, int* __restrict__ count) {
  __shared__ float4 tile[kRadThreads];
  const int tid = threadIdx.x, i = blockIdx.x * kRadThreads + tid;
  const bool valid_i = i < n;
  float qx = 0, qy = 0, qz = 0;
  bool fin = false;
  if (valid_i) { qx = pts[3 * (size_t)i]; qy = pts[3 * (size_t)i + 1]; qz = pts[3 * (size_t)i + 2]; fin = isfinite(qx) && isfinite(qy) && isfinite(qz); }
  const float nanf_ = __int_as_float(0x7fc00000);
  int cnt = 0;
  for (int t0 = 0; t0 < n; t0 += kRadThreads) {
    __syncthreads();          // the previous tile has been consumed
    const int c = t0 + tid;
    float4 p = make_float4(nanf_, nanf_, nanf_, 0.0f);
    if (c < n) {
      const float x = pts[3 * (size_t)c], y = pts[3 * (size_t)c + 1], z = pts[3 * (size_t)c + 2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) { p.x = x; p.y = y; p.z = z; }
    }
    tile[tid] = p;
    __syncthreads();
    if (!fin) continue;
    const int m = min(kRadThreads, n - t0);
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
      const float4 q = tile[j];
      const float dx = qx - q.x, dy = qy - q.y, dz = qz - q.z;
      const float d = (dx * dx + dy * dy) + dz * dz;      // flann::L2_Simple<float>
      cnt += d <= r2 ? 1 : 0;
    }
  }
  if (valid_i) count[i] = fin ? cnt - 1 : -1;
}
// the flags the ordered compaction reads, one per stage of the chain
__global__ __launch_bounds__(256) void k_radius_flag(const int* __restrict__ count, int n, int min_neighbors, unsigned char* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = count[i] >= min_neighbors ? 1 : 0;      // -1 (not a finite point) is below every min_neighbors >= 0
}
__global__ __launch_bounds__(256) void k_finite_flag(const float* __restrict__ pts, int n, unsigned char* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  flag[i] = (isfinite(x) && isfinite(y) && isfinite(z)) ? 1 : 0;
}
// pcl::StatisticalOutlierRemoval::applyFilterIndices on the device.  The moments of the mean distances are SEQUENTIAL double sums in index
// order, as the host wrapper forms them: one thread, n adds (the chain's clouds are downsampled; 10^4 points take about 0.1 ms).  out:
// sum, sum of squares, number of valid entries.  The host turns them into the threshold with the wrapper's own expression.
__global__ void k_sor_moments(const float* __restrict__ md, int n, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0, sq = 0;
  int valid = 0;
  for (int i = 0; i < n; ++i) {
    const float v = md[i];
    if (v >= 0) { sum += v; sq += (double)v * v; ++valid; }
  }
  out[0] = sum; out[1] = sq; out[2] = (double)valid;
}
__global__ __launch_bounds__(256) void k_sor_flag(const float* __restrict__ md, int n, double thr, unsigned char* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = (md[i] >= 0 && !((double)md[i] > thr)) ? 1 : 0;
}
struct GatherPred {    // set flags -> their POINTS, in ascending index: the gather of a stage's kept points, fused into the compaction
  const unsigned char* flag; const float* src; float* dst;
  __device__ bool keep(int i) const { return flag[i]; }
  __device__ void put(int pos, int i) const {
    dst[3 * (size_t)pos] = src[3 * (size_t)i]; dst[3 * (size_t)pos + 1] = src[3 * (size_t)i + 1]; dst[3 * (size_t)pos + 2] = src[3 * (size_t)i + 2];
  }
};
}  // namespace seg

// ---- host only ---------------------------------------------------------------------------------------------------------------------
constexpr int kSorMaxMeanK = 64;   // kSorMaxK of sslam_seg.hip: mean_k must stay below it
inline int prefilter_check_params(const sslam_prefilter_params* p) {
  if (!p) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (p->use_distance_filter && (std::isnan(p->distance_near) || std::isnan(p->distance_far)))
    return set_error(SSLAM_ERR_INVALID, "prefilter: distance_near / distance_far is NaN");
  if (p->downsample != SSLAM_DOWNSAMPLE_NONE && p->downsample != SSLAM_DOWNSAMPLE_VOXELGRID)
    return set_error(SSLAM_ERR_INVALID, "prefilter: downsample %d is neither NONE nor VOXELGRID", p->downsample);
  if (p->downsample == SSLAM_DOWNSAMPLE_VOXELGRID && !(p->leaf > 0 && std::isfinite(p->leaf)))
    return set_error(SSLAM_ERR_INVALID, "prefilter: leaf %g must be finite and positive", (double)p->leaf);
  if (p->outlier != SSLAM_OUTLIER_NONE && p->outlier != SSLAM_OUTLIER_STATISTICAL && p->outlier != SSLAM_OUTLIER_RADIUS)
    return set_error(SSLAM_ERR_INVALID, "prefilter: outlier %d is none of NONE, STATISTICAL, RADIUS", p->outlier);
  if (p->outlier == SSLAM_OUTLIER_STATISTICAL && (p->mean_k < 1 || p->mean_k >= kSorMaxMeanK || std::isnan(p->stddev_mul)))
    return set_error(SSLAM_ERR_INVALID, "prefilter: mean_k must be in [1, %d) and stddev_mul a number", kSorMaxMeanK);
  if (p->outlier == SSLAM_OUTLIER_RADIUS && (!(p->radius > 0 && std::isfinite(p->radius)) || p->min_neighbors < 0))
    return set_error(SSLAM_ERR_INVALID, "prefilter: radius must be finite and positive, min_neighbors >= 0");
  return 0;
}
inline int odom_check_params(const sslam_odom_params* p) {
  int rc = prefilter_check_params(&p->prefilter);
  if (rc) return rc;
  if (p->method != SSLAM_REG_ICP && p->method != SSLAM_REG_GICP) return set_error(SSLAM_ERR_INVALID, "odometry: method %d is neither ICP nor GICP", p->method);
  if (p->method == SSLAM_REG_GICP && (rc = gicp_check_params(p->gicp.k, p->gicp.plane_epsilon))) return rc;
  if (p->max_iterations < 0) return set_error(SSLAM_ERR_INVALID, "odometry: max_iterations is negative");
  const double v[7] = {p->epsilon, p->max_correspondence_distance, p->keyframe_delta_trans, p->keyframe_delta_angle, p->keyframe_delta_time,
                       p->max_acceptable_trans, p->max_acceptable_angle};
  for (double x : v)
    if (!(std::isfinite(x) && x >= 0.0)) return set_error(SSLAM_ERR_INVALID, "odometry: a threshold (%g) is not finite and >= 0", x);
  return 0;
}
// 3 x 4 transforms as 12 doubles (R row-major, then t), in the order include/sslam.h states; sslam_seg.hip is built without FMA contraction
inline void odom_identity(double T[12]) {
  for (int k = 0; k < 12; ++k) T[k] = 0.0;
  T[0] = T[4] = T[8] = 1.0;
}
inline void odom_mul(const double A[12], const double B[12], double C[12]) {
  double O[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) O[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
    O[9 + i] = ((A[3 * i] * B[9] + A[3 * i + 1] * B[10]) + A[3 * i + 2] * B[11]) + A[9 + i];
  }
  for (int k = 0; k < 12; ++k) C[k] = O[k];
}
inline void odom_inverse(const double A[12], double C[12]) {
  double O[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) O[3 * i + j] = A[3 * j + i];
    O[9 + i] = -((A[i] * A[9] + A[3 + i] * A[10]) + A[6 + i] * A[11]);
  }
  for (int k = 0; k < 12; ++k) C[k] = O[k];
}
inline double odom_trans(const double T[12]) { return std::sqrt((T[9] * T[9] + T[10] * T[10]) + T[11] * T[11]); }
// upstream's acos(Quaternionf(R).w()): HALF the rotation angle
inline double odom_angle(const double T[12]) {
  const Quat q = quat_of_rotation(T);
  return std::acos(std::fmin(1.0, std::fabs(q.w)));
}
}  // namespace sslam
