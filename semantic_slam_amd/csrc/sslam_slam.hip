// Orchestrator tick without ROS: keyframe gate, keyframe / landmark queues, graph growth, optimisation,
// landmark marginals, map->odom, and data association on the device.
//
// Follows   src/ps_graph_slam/semantic_graph_slam.cpp:11-102 (init, run), :104-150 (empty_keyframe_queue),
//           :152-179 (empty_landmark_queue), :181-205 (getAndSetLandmarkCov), :207-232 (semantic_data_ass), :234-287 (VIOCallback),
//           :289-329 (addFirstPoseAndLandmark);
//           include/ps_graph_slam/keyframe_updater.hpp:41-65; include/ps_graph_slam/data_association.h:70-389;
//           src/ps_graph_slam/information_matrix_calculator.cpp:28-35; include/ps_graph_slam/ros_utils.hpp:90-106;
//           include/tools.h:104-135 (transformPoseFromCameraToRobot).
//
// What runs where.  The tick's heavy parts are the three C-ABI calls it makes into this same library -- the batched frontend pass
// over all keyframes of the tick (sslam_seg_segment_batch), sslam_graph_optimize and the landmark marginals -- all on the GPU.
// Data association is a single-workgroup kernel over the device-resident landmark table: the detections of a frame are resolved one
// after the other (a landmark created by detection j is a candidate for detection j+1, as in the reference where map_a_new_lan
// appends to landmarks_ inside the loop), the landmarks are scanned in parallel with a wave argmin.
//
// Deviations from the reference, all on undefined behaviour of the original:
//   * a landmark created earlier in the same frame has no graph node yet; the reference dereferences its uninitialised node
//     pointer (data_association.h:378 through :137); here its expected measurement is the position it was created at.
//   * distance_min is reset per detection unless reference_quirks bit 0 is set; neareast_landmarks_id
//     (uninitialised in the reference when no candidate beat distance_min) maps to "new landmark".
//   * InformationMatrixCalculator without ~use_const_inf_matrix reads members that are never initialised
//     (information_matrix_calculator.hpp:31-36) and has its score stubbed (information_matrix_calculator.cpp:37): the flag is refused;
//     sslam_slam_set_fitness_information installs the model with defined parameters and the real score (sslam_seg_fitness_scores).
#include <hip/hip_runtime.h>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

#include "../../include/sslam.h"
#include "map_cloud.hpp"
#include "occupancy_map.hpp"
#include "sslam_common.hpp"
#include "sslam_math.hpp"

using namespace sslam;

namespace {

// ---- rigid transforms (Eigen::Isometry3d in the reference) as translation + unit quaternion -----------------------------------
Pose pose_identity() { return Pose{{0, 0, 0}, {0, 0, 0, 1}}; }
Quat qnormalized(Quat q) {
  const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return {q.x / n, q.y / n, q.z / n, q.w / n};
}
Pose compose(const Pose& a, const Pose& b) { return Pose{a.t + qrot(a.q, b.t), qnormalized(qmul(a.q, b.q))}; }
Pose inverse(const Pose& a) {
  const Quat qi = qconj(a.q);
  const Vec3 t = qrot(qi, a.t);
  return Pose{{-t.x, -t.y, -t.z}, qi};
}
Pose from_tq(const double* v) { return Pose{{v[0], v[1], v[2]}, qnormalized(Quat{v[3], v[4], v[5], v[6]})}; }
void to_tq(const Pose& p, double* v) {
  v[0] = p.t.x; v[1] = p.t.y; v[2] = p.t.z; v[3] = p.q.x; v[4] = p.q.y; v[5] = p.q.z; v[6] = p.q.w;
}

// ps_graph_slam::matrix2vector (ros_utils.hpp:90-106): float quaternion, normalised, then tf::Matrix3x3::getEulerYPR in double
void pose_to_vector6(const Pose& p, float out[6]) {
  float qx = (float)p.q.x, qy = (float)p.q.y, qz = (float)p.q.z, qw = (float)p.q.w;
  const float n = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx /= n; qy /= n; qz /= n; qw /= n;
  const double x = qx, y = qy, z = qz, w = qw;
  // tf::Matrix3x3::setRotation
  const double d = x * x + y * y + z * z + w * w, s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
  const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
  double yaw, pitch, roll;
  if (std::fabs(m20) >= 1) {   // gimbal lock branch of getEulerYPR
    yaw = 0;
    const double delta = std::atan2(m21, m22);
    if (m20 < 0) { pitch = M_PI / 2.0; roll = delta; }
    else { pitch = -M_PI / 2.0; roll = delta; }
  } else {
    pitch = -std::asin(m20);
    roll = std::atan2(m21 / std::cos(pitch), m22 / std::cos(pitch));
    yaw = std::atan2(m10 / std::cos(pitch), m00 / std::cos(pitch));
  }
  out[0] = (float)p.t.x; out[1] = (float)p.t.y; out[2] = (float)p.t.z;
  out[3] = (float)roll; out[4] = (float)pitch; out[5] = (float)yaw;
}

void mat4_mul(const float* A, const float* B, float* C) {
  float T[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      float s = 0;
      for (int k = 0; k < 4; ++k) s += A[r * 4 + k] * B[k * 4 + c];
      T[r * 4 + c] = s;
    }
  std::memcpy(C, T, sizeof T);
}

// semantic_tools::transformPoseFromCameraToRobot (tools.h:104-135)
void cam_to_robot(float cam_angle, float out[16]) {
  float rxc[16] = {0}, rxr[16] = {0}, rzr[16] = {0};
  const double a = -(double)cam_angle;
  rxc[0] = 1; rxc[5] = (float)std::cos(a); rxc[6] = (float)-std::sin(a); rxc[9] = (float)std::sin(a); rxc[10] = (float)std::cos(a); rxc[15] = 1;
  rxr[0] = 1; rxr[5] = (float)std::cos(-1.5708); rxr[6] = (float)-std::sin(-1.5708); rxr[9] = (float)std::sin(-1.5708); rxr[10] = (float)std::cos(-1.5708); rxr[15] = 1;
  rzr[0] = (float)std::cos(-1.5708); rzr[1] = (float)-std::sin(-1.5708); rzr[4] = (float)std::sin(-1.5708); rzr[5] = (float)std::cos(-1.5708); rzr[10] = 1; rzr[15] = 1;
  float M[16];
  mat4_mul(rzr, rxr, M);
  mat4_mul(M, rxc, out);
}

// ---- data association on the device ------------------------------------------------------------------------------------------
struct DetIn {           // what find_matches reads of a detected_object (detected_object.h:14-24)
  float pose[3];         // centroid in the camera frame
  float normal[4];
  int class_id, plane_type;
};
struct AssocArgs {
  float Tw[16];          // transformNormalsToWorld(robot_pose, cam_angle)
  float Tr[16];          // transformPoseFromCameraToRobot(cam_angle)
  float robot[3];        // robot position; y already carries the -0.04 of ~use_rtab_map_odom (data_association.h:335-338)
  float q;               // Q_ diagonal = land_noise_low
  double maha_thres, eq_thres;
  int use_maha, use_eq, first_object, keep_distance_min;
  int n_det;
};
struct LmTable {         // device-resident landmark list (structure of arrays)
  float* est;            // 3 per landmark: node->estimate() cast to float (landmarkMeasurementModel, data_association.h:375-380)
  float* cov;            // 9 per landmark
  int* kind;             // class_id | plane_type << 16
  int* count;            // number of landmarks
};

__device__ __forceinline__ void mat4_vec(const float* T, const float* v, float* o) {
  for (int r = 0; r < 4; ++r) {
    float s = 0;
    for (int k = 0; k < 4; ++k) s += T[r * 4 + k] * v[k];
    o[r] = s;
  }
}

// z^T (S + Q)^-1 z with the inverse formed the way Eigen forms it for a run-time sized matrix: partial-pivot LU, then the three
// columns of the identity solved one by one (data_association.h:158-168 works on Eigen::MatrixXf)
__device__ float mahalanobis3(const float* S, float q, const float* z) {
  float A[9];
  for (int k = 0; k < 9; ++k) A[k] = S[k];
  A[0] += q; A[4] += q; A[8] += q;
  int piv[3] = {0, 1, 2};
  for (int c = 0; c < 3; ++c) {
    int p = c;
    float best = fabsf(A[piv[c] * 3 + c]);
    for (int r = c + 1; r < 3; ++r) {
      const float v = fabsf(A[piv[r] * 3 + c]);
      if (v > best) { best = v; p = r; }
    }
    const int t = piv[c]; piv[c] = piv[p]; piv[p] = t;
    const float d = A[piv[c] * 3 + c];
    for (int r = c + 1; r < 3; ++r) {
      const float f = A[piv[r] * 3 + c] / d;
      A[piv[r] * 3 + c] = f;
      for (int k = c + 1; k < 3; ++k) A[piv[r] * 3 + k] -= f * A[piv[c] * 3 + k];
    }
  }
  float inv[9];
  for (int col = 0; col < 3; ++col) {
    float y[3];
    for (int r = 0; r < 3; ++r) {
      float s = piv[r] == col ? 1.0f : 0.0f;
      for (int k = 0; k < r; ++k) s -= A[piv[r] * 3 + k] * y[k];
      y[r] = s;
    }
    for (int r = 2; r >= 0; --r) {
      float s = y[r];
      for (int k = r + 1; k < 3; ++k) s -= A[piv[r] * 3 + k] * inv[k * 3 + col];
      inv[r * 3 + col] = s / A[piv[r] * 3 + r];
    }
  }
  float rv[3];
  for (int c = 0; c < 3; ++c) rv[c] = z[0] * inv[c] + z[1] * inv[3 + c] + z[2] * inv[6 + c];
  return rv[0] * z[0] + rv[1] * z[1] + rv[2] * z[2];
}

constexpr int kAssocThreads = 256;

// data_association::find_matches / associate_lanmarks / map_a_new_lan / inserst_a_mapped_lan (data_association.h:75-317).
// One workgroup; detections in order, landmarks in parallel.  The arg-min keeps the lowest landmark index among equal distances
// (the reference's strict `distance < distance_min` over ascending i).
__global__ __launch_bounds__(kAssocThreads) void k_associate(AssocArgs A, const DetIn* __restrict__ det, LmTable L, sslam_landmark* __restrict__ out) {
  __shared__ float s_d[kAssocThreads / 64];
  __shared__ int s_i[kAssocThreads / 64];
  __shared__ int s_any[kAssocThreads / 64];
  __shared__ int s_n;
  __shared__ float s_carry;   // distance_min carried across detections (quirk B5)
  const int tid = threadIdx.x;
  if (tid == 0) { s_n = *L.count; s_carry = 3.402823466e+38f; }
  __syncthreads();
  for (int j = 0; j < A.n_det; ++j) {
    const DetIn D = det[j];
    const float pc[4] = {D.pose[0], D.pose[1], D.pose[2], 1.0f};
    float pw[4], nw[4], pr[4];
    mat4_vec(A.Tw, pc, pw);                 // convertPoseToWorld (data_association.h:319-342)
    pw[0] += A.robot[0]; pw[1] += A.robot[1]; pw[2] += A.robot[2];
    mat4_vec(A.Tw, D.normal, nw);           // convertNormalsToWorld (:344-358)
    mat4_vec(A.Tr, pc, pr);                 // convertCamToRobot (:360-373)
    const int n = s_n;
    const int kind = D.class_id | (D.plane_type << 16);
    float dmin = A.keep_distance_min ? s_carry : 3.402823466e+38f;
    int imin = -1;
    bool any = false;
    if (!A.first_object) {
      for (int i = tid; i < n; i += kAssocThreads) {
        if (L.kind[i] != kind) continue;
        any = true;
        const float z[3] = {pw[0] - L.est[i * 3], pw[1] - L.est[i * 3 + 1], pw[2] - L.est[i * 3 + 2]};
        float dist = 0.0f;
        if (A.use_maha) dist = mahalanobis3(L.cov + i * 9, A.q, z);
        else if (A.use_eq) dist = sqrtf(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);   // semantic_tools::dist
        if (dist < dmin) { dmin = dist; imin = i; }
      }
    }
    // wave, then workgroup arg-min; ties -> lowest index
    for (int off = 32; off > 0; off >>= 1) {
      const float od = __shfl_xor(dmin, off);
      const int oi = __shfl_xor(imin, off);
      if (oi >= 0 && (od < dmin || (od == dmin && (imin < 0 || oi < imin)))) { dmin = od; imin = oi; }
    }
    const unsigned long long anyb = __ballot(any);
    if ((tid & 63) == 0) { s_d[tid >> 6] = dmin; s_i[tid >> 6] = imin; s_any[tid >> 6] = anyb != 0ull; }
    __syncthreads();
    if (tid == 0) {
      float bd = A.keep_distance_min ? s_carry : 3.402823466e+38f;
      int bi = -1;
      bool found = false;                   // found_nearest_neighbour: some landmark of the same type and plane type exists
      for (int w = 0; w < kAssocThreads / 64; ++w) {
        found = found || s_any[w];
        const float wd = s_d[w];
        const int wi = s_i[w];
        if (wi >= 0 && (wd < bd || (wd == bd && (bi < 0 || wi < bi)))) { bd = wd; bi = wi; }
      }
      if (A.keep_distance_min && bi >= 0) s_carry = bd;
      bool matched = false;
      if (found && bi >= 0) {
        if (A.use_maha) matched = !((double)bd > A.maha_thres);
        else if (A.use_eq) matched = !((double)bd > A.eq_thres);
      }
      sslam_landmark R;
      R.class_id = D.class_id; R.plane_type = D.plane_type;
      R.vertex = -1;
      for (int k = 0; k < 3; ++k) { R.pose[k] = pw[k]; R.local_pose[k] = pr[k]; }
      for (int k = 0; k < 4; ++k) R.normal[k] = nw[k];
      for (int k = 0; k < 9; ++k) R.covariance[k] = (k % 4 == 0) ? A.q : 0.0f;   // covariance = Q_ (:265, :304)
      R.distance = (found && bi >= 0) ? bd : -1.0f;
      if (matched) {
        R.is_new = 0; R.id = bi;
      } else {                              // map_a_new_lan: id = landmarks_.size(), appended at once (:259-269)
        R.is_new = 1; R.id = n;
        L.est[n * 3] = pw[0]; L.est[n * 3 + 1] = pw[1]; L.est[n * 3 + 2] = pw[2];
        for (int k = 0; k < 9; ++k) L.cov[n * 9 + k] = R.covariance[k];
        L.kind[n] = kind;
        s_n = n + 1;
        __threadfence_block();
      }
      out[j] = R;
    }
    __syncthreads();
  }
  if (tid == 0) *L.count = s_n;
}

// ---- loop candidates on the device (hdl_graph_slam's LoopDetector::find_candidates [UPSTREAM]) ----------------------------------------
struct LoopCandArgs {
  const double* keys;    // x, y, accum_distance per old keyframe
  const double* news;    // the same per new keyframe
  int n_keys, n_new;
  double accum_thresh;   // accum_distance_thresh
  double d2_thresh;      // distance_thresh * distance_thresh, formed once on the host
  int m;                 // max_candidates: 0 = all that pass, else the m nearest
  int cap;               // row length of cand
  int32_t* cand;         // n_new x cap, filled with -1 by the host
  int32_t* count;        // n_new
};

// whether old keyframe (kx, ky, ka) is a candidate of the new keyframe (qx, qy, qa), and its squared xy distance.  No fused multiply-add.
__device__ __forceinline__ bool loop_pass(double qx, double qy, double qa, double kx, double ky, double ka, double accum_thresh, double d2_thresh, double& d2) {
  const double dx = qx - kx, dy = qy - ky, da = qa - ka;
  d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
  const bool fin = isfinite(qx) && isfinite(qy) && isfinite(qa) && isfinite(kx) && isfinite(ky) && isfinite(ka) && isfinite(da) && isfinite(d2);
  return fin && da >= accum_thresh && d2 <= d2_thresh;
}

constexpr int kLoopWave = 64;

// One wave per new keyframe, its lanes striding over the old keyframes.  m == 0: the passing indices in ascending order by ballot and
// prefix count.  m > 0: m rounds; in each, every lane finds the smallest key (d2, index) of its stride above the key chosen last, and a
// wave reduction picks the smallest of the lanes.  No atomics: the result does not depend on the launch geometry.
__global__ __launch_bounds__(kLoopWave) void k_loop_candidates(LoopCandArgs A) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= A.n_new) return;
  const double qx = A.news[3 * (size_t)n], qy = A.news[3 * (size_t)n + 1], qa = A.news[3 * (size_t)n + 2];
  int32_t* row = A.cand + (size_t)n * A.cap;
  int total = 0;
  if (A.m == 0) {
    for (int base = 0; base < A.n_keys; base += kLoopWave) {
      const int k = base + lane;
      double d2;
      const bool p = k < A.n_keys && loop_pass(qx, qy, qa, A.keys[3 * (size_t)k], A.keys[3 * (size_t)k + 1], A.keys[3 * (size_t)k + 2], A.accum_thresh, A.d2_thresh, d2);
      const unsigned long long b = __ballot(p);
      const int pos = total + __popcll(b & ((1ull << lane) - 1ull));
      if (p && pos < A.cap) row[pos] = k;
      total += __popcll(b);
    }
  } else {
    double last_d = -1.0;   // d2 >= 0: below every key
    int last_k = -1;
    for (int r = 0; r < A.m; ++r) {
      double best_d = 0.0;
      int best_k = -1;
      for (int k = lane; k < A.n_keys; k += kLoopWave) {
        double d2;
        if (!loop_pass(qx, qy, qa, A.keys[3 * (size_t)k], A.keys[3 * (size_t)k + 1], A.keys[3 * (size_t)k + 2], A.accum_thresh, A.d2_thresh, d2)) continue;
        if (!(d2 > last_d || (d2 == last_d && k > last_k))) continue;             // chosen in an earlier round
        if (best_k < 0 || d2 < best_d) { best_d = d2; best_k = k; }               // ascending k: equal d2 keeps the lowest index
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(best_d, off);
        const int ok = __shfl_xor(best_k, off);
        if (ok >= 0 && (best_k < 0 || od < best_d || (od == best_d && ok < best_k))) { best_d = od; best_k = ok; }
      }
      if (best_k < 0) break;                                                      // uniform: every lane holds the wave's result
      if (lane == 0 && r < A.cap) row[r] = best_k;
      last_d = best_d; last_k = best_k;
      ++total;
    }
  }
  if (lane == 0) A.count[n] = total;
}

// ---- host state ---------------------------------------------------------------------------------------------------------------
struct KeyFrame {
  int32_t sec = 0, nsec = 0;
  Pose odom = pose_identity(), robot_pose = pose_identity();
  double accum_distance = 0;
  int node = -1;
  std::vector<uint8_t> cloud;
  int width = 0, height = 0, point_step = 0, row_step = 0, off[3] = {0, 0, 0};
  std::vector<sslam_box> boxes;           // obj_info
  std::vector<sslam_plane> objects;       // pre-segmented (extension)
  bool presegmented = false;
  std::vector<float> ds;                  // loop closure: the downsampled cloud (xyz), kept for the rest of the run
  bool has_ds = false;
  std::vector<double> cov;                // loop registration GICP: 6 doubles per point of ds, computed once, kept with it
  bool map_done = false;                  // map clouds: this keyframe's cloud has been looked at (appended, or found empty)
};

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  int reserve(size_t n, hipStream_t st, size_t keep) {   // grows geometrically, keeps the first `keep` elements
    if (n <= cap) return 0;
    size_t nc = cap ? cap : 256;
    while (nc < n) nc *= 2;
    T* q = nullptr;
    SSLAM_HIP_TRY(hipMalloc(&q, nc * sizeof(T)));
    if (p && keep) SSLAM_HIP_TRY(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st));
    SSLAM_HIP_TRY(hipStreamSynchronize(st));
    if (p) (void)hipFree(p);
    p = q; cap = nc;
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  ~DevBuf() { release(); }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct sslam_slam {
  sslam_slam_params P;
  sslam_seg* seg = nullptr;
  sslam_graph* graph = nullptr;
  double cam_angle = 0;
  // semantic_graph_slam state (semantic_graph_slam.h)
  bool object_detection_available = false, point_cloud_available = false, first_key_added = false;
  Pose robot_pose = pose_identity(), vio_pose = pose_identity(), prev_odom = pose_identity(), map2odom = pose_identity();
  std::deque<std::shared_ptr<KeyFrame>> keyframe_queue;
  std::vector<std::shared_ptr<KeyFrame>> new_keyframes, keyframes;
  KeyFrame latest;                        // point_cloud_msg_ / object_info_ / pre-segmented objects of the callbacks
  bool segmented_available = false;
  // KeyframeUpdater
  bool is_first = true;
  Pose prev_keypose = pose_identity();
  int32_t prev_sec = 0, prev_nsec = 0;
  double accum_distance = 0;
  // data_association
  bool first_object = true;
  std::vector<sslam_landmark> landmarks;
  // device side of the landmark list
  hipStream_t stream = nullptr;
  DevBuf<float> d_est, d_cov;
  DevBuf<int> d_kind, d_count;
  DevBuf<DetIn> d_det;
  DevBuf<sslam_landmark> d_out;
  sslam::PinnedScratch pin;               // page-locked staging of the table / detection / result copies
  bool table_dirty = true;                // host landmarks changed outside the kernel -> re-upload before the next association
  // sslam_slam_set_fitness_information: odometry information from the fitness score of the keyframes' clouds
  bool fit_on = false;
  sslam_inf_params fit_P{};
  float fit_leaf = 0.1f;
  double fit_range = DBL_MAX;
  bool fit_prev_has = false;              // fit_prev: the downsampled cloud of the last processed keyframe (target of the next tick's first pair)
  std::vector<float> fit_prev;
  std::vector<double> fit_score;          // odometry edges of the last run(), in order; -1 / -1: constant matrix
  std::vector<int32_t> fit_used;
  // sslam_slam_set_loop_closure: candidate search, scan match, gate and loop edge inside the tick
  bool loop_on = false;
  sslam_loop_params loop_P{};
  int loop_method = SSLAM_REG_ICP;        // sslam_slam_set_loop_registration
  sslam_gicp_params loop_gicp{20, 1e-3};
  int64_t loop_cov_passes = 0;            // clouds that went through sslam_seg_cloud_covariances so far
  double last_edge_accum = 0;             // accum_distance of the keyframe that got the last loop edge (hdl's last_edge_accum_distance)
  std::vector<sslam_loop> loops;          // records of the last run()
  double loop_seconds[4] = {0, 0, 0, 0};  // candidates, registration, gate, the whole stage (downsampling included) of the last run()
  DevBuf<double> d_ltab;                  // [keys 3 n_keys | news 3 n_new]
  DevBuf<int32_t> d_lout;                 // [cand n_new x cap | count n_new]
  // sslam_slam_set_map_clouds: the downsampled cloud of every keyframe, resident on the device for sslam_slam_map_cloud
  bool map_on = false;
  float map_leaf = 0.1f;
  DevBuf<float> d_map_xyz, d_map_pose;    // the clouds one after the other; 12 floats per cloud, rewritten by every map call
  DevBuf<int32_t> d_map_start;            // cloud_start of the resident clouds
  std::vector<int32_t> map_start{0};      // its host copy
  std::vector<std::shared_ptr<KeyFrame>> map_kf;   // the keyframe of every resident cloud, in keyframe order
  int64_t map_pending_bytes = 0;          // cloud bytes sent since the last sslam_slam_map_cloud
  ~sslam_slam() {
    if (graph) sslam_graph_destroy(graph);
    if (stream) { (void)hipSetDevice(P.device); (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
  }
};

namespace {

int ensure_stream(sslam_slam* s) {
  if (s->stream) return 0;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return set_error(SSLAM_ERR_NO_DEVICE, "no HIP device visible (%s); data association has no CPU fallback", hipGetErrorString(e));
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  SSLAM_HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  return 0;
}

// host landmark list -> device table (after the marginals / estimates changed, or before the first association)
int upload_table(sslam_slam* s) {
  const size_t n = s->landmarks.size();
  int rc;
  if ((rc = s->d_est.reserve(3 * (n + 64), s->stream, 0))) return rc;
  if ((rc = s->d_cov.reserve(9 * (n + 64), s->stream, 0))) return rc;
  if ((rc = s->d_kind.reserve(n + 64, s->stream, 0))) return rc;
  if ((rc = s->d_count.reserve(1, s->stream, 0))) return rc;
  // staged page-locked: [est 3n | cov 9n | kind n | count]
  const size_t bytes = (13 * n + 1) * 4;
  std::vector<char> fallback;
  char* stage = s->pin.get(bytes);
  if (!stage) { fallback.resize(bytes); stage = fallback.data(); }
  float* est = reinterpret_cast<float*>(stage);
  float* cov = est + 3 * n;
  int* kind = reinterpret_cast<int*>(cov + 9 * n);
  int* cnt = kind + n;
  for (size_t i = 0; i < n; ++i) {
    const sslam_landmark& l = s->landmarks[i];
    if (l.vertex >= 0) {   // landmarkMeasurementModel: h = l.node->estimate().cast<float>()
      double p[3];
      if (sslam_graph_get_vertex(s->graph, l.vertex, p) < 0) return SSLAM_ERR_INVALID;
      for (int k = 0; k < 3; ++k) est[3 * i + k] = (float)p[k];
    } else {
      for (int k = 0; k < 3; ++k) est[3 * i + k] = l.pose[k];
    }
    for (int k = 0; k < 9; ++k) cov[9 * i + k] = l.covariance[k];
    kind[i] = l.class_id | (l.plane_type << 16);
  }
  *cnt = (int)n;
  if (n) {
    SSLAM_HIP_TRY(hipMemcpyAsync(s->d_est.p, est, 3 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(s->d_cov.p, cov, 9 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    SSLAM_HIP_TRY(hipMemcpyAsync(s->d_kind.p, kind, n * sizeof(int), hipMemcpyHostToDevice, s->stream));
  }
  SSLAM_HIP_TRY(hipMemcpyAsync(s->d_count.p, cnt, sizeof(int), hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  s->table_dirty = false;
  return 0;
}

// data_association::find_matches (data_association.h:75-95) -> landmark records of this frame's detections
int find_matches(sslam_slam* s, const sslam_plane* objs, int n, const float robot_pose[6], std::vector<sslam_landmark>& out) {
  out.clear();
  if (n <= 0) return 0;
  int rc = ensure_stream(s);
  if (rc) return rc;
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  if (s->table_dirty && (rc = upload_table(s))) return rc;
  const size_t nl = s->landmarks.size();
  if ((rc = s->d_est.reserve(3 * (nl + n), s->stream, 3 * nl))) return rc;
  if ((rc = s->d_cov.reserve(9 * (nl + n), s->stream, 9 * nl))) return rc;
  if ((rc = s->d_kind.reserve(nl + n, s->stream, nl))) return rc;
  if ((rc = s->d_det.reserve(n, s->stream, 0))) return rc;
  if ((rc = s->d_out.reserve(n, s->stream, 0))) return rc;
  // detections in, landmark records out: both through the page-locked staging buffer
  const size_t det_bytes = ((size_t)n * sizeof(DetIn) + 7) & ~(size_t)7, out_bytes = (size_t)n * sizeof(sslam_landmark);
  std::vector<char> fallback;
  char* stage = s->pin.get(det_bytes + out_bytes);
  if (!stage) { fallback.resize(det_bytes + out_bytes); stage = fallback.data(); }
  DetIn* det = reinterpret_cast<DetIn*>(stage);
  for (int j = 0; j < n; ++j) {
    for (int k = 0; k < 3; ++k) det[j].pose[k] = objs[j].centroid_cam[k];
    for (int k = 0; k < 4; ++k) det[j].normal[k] = objs[j].normal_d[k];
    det[j].class_id = objs[j].class_id; det[j].plane_type = objs[j].plane_type;
  }
  AssocArgs A;
  const float cam = (float)s->cam_angle;
  if ((rc = sslam_seg_transform(s->seg, robot_pose, cam, A.Tw)) < 0) return rc;
  cam_to_robot(cam, A.Tr);
  A.robot[0] = robot_pose[0];
  A.robot[1] = s->P.use_rtab_map_odom ? (float)((double)robot_pose[1] - 0.04) : robot_pose[1];
  A.robot[2] = robot_pose[2];
  A.q = (float)s->P.land_noise_low;
  A.maha_thres = s->P.maha_dist_thres; A.eq_thres = s->P.eq_dist_thres;
  A.use_maha = s->P.use_maha_dist; A.use_eq = s->P.use_eq_dist;
  A.first_object = s->first_object ? 1 : 0;
  A.keep_distance_min = s->P.reference_quirks & 1;
  A.n_det = n;
  LmTable L{s->d_est.p, s->d_cov.p, s->d_kind.p, s->d_count.p};
  SSLAM_HIP_TRY(hipMemcpyAsync(s->d_det.p, det, n * sizeof(DetIn), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(k_associate, dim3(1), dim3(kAssocThreads), 0, s->stream, A, s->d_det.p, L, s->d_out.p);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipMemcpyAsync(stage + det_bytes, s->d_out.p, out_bytes, hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  out.resize(n);
  memcpy(out.data(), stage + det_bytes, out_bytes);
  for (sslam_landmark& r : out) {
    if (r.is_new) {
      s->landmarks.push_back(r);                       // landmarks_.push_back(new_landmark) (:269)
    } else {
      r.vertex = s->landmarks[r.id].vertex;            // landmark.node = l.node (:309)
    }
  }
  if (s->first_object && !out.empty()) s->first_object = false;   // (:84-85)
  return 0;
}

// InformationMatrixCalculator::calc_information_matrix (information_matrix_calculator.cpp:28-35)
void odometry_information(const sslam_slam* s, double info[36]) {
  const double sx = s->P.const_stddev_x == 0 ? 0.0667 : s->P.const_stddev_x;
  const double sq = s->P.const_stddev_q == 0 ? 0.0667 : s->P.const_stddev_q;
  std::memset(info, 0, 36 * sizeof(double));
  for (int k = 0; k < 3; ++k) { info[k * 7] = 1.0 / sx; info[(k + 3) * 7] = 1.0 / sq; }
}

// the finite points of a keyframe's cloud, voxel-grid downsampled on the device -> out (xyz)
int downsampled_cloud(sslam_slam* s, const KeyFrame& kf, float leaf, std::vector<float>& out) {
  std::vector<float> pts;
  pts.reserve((size_t)kf.width * kf.height * 3);
  for (int r = 0; r < kf.height; ++r)
    for (int c = 0; c < kf.width; ++c) {
      const uint8_t* p = kf.cloud.data() + (size_t)r * kf.row_step + (size_t)c * kf.point_step;
      float v[3];
      for (int k = 0; k < 3; ++k) std::memcpy(&v[k], p + kf.off[k], sizeof(float));
      if (std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2])) pts.insert(pts.end(), v, v + 3);
    }
  const int n = (int)(pts.size() / 3);
  out.assign(pts.size(), 0.0f);
  if (n == 0) return 0;
  const int m = sslam_seg_voxel_grid(s->seg, pts.data(), n, leaf, out.data(), nullptr, n);
  if (m < 0) return m;
  out.resize((size_t)m * 3);
  return 0;
}

// With the fitness model: the score of every consecutive pair (prev, kf) of the tick whose keyframes both carry a cloud -- all of them in
// ONE pass on the frontend handle -- before anything is added to the graph.  score / used [n]: -1 where the edge takes the constant matrix.
int fitness_of_tick(sslam_slam* s, int n, std::vector<double>& score, std::vector<int32_t>& used, std::vector<float>& last_cloud, bool& last_has) {
  score.assign(n, -1.0); used.assign(n, -1);
  last_has = false;
  auto has_cloud = [&](int i) { return i < 0 ? s->fit_prev_has : !s->keyframe_queue[i]->cloud.empty(); };   // -1: the last keyframe of the tick before
  std::vector<int> edge;                  // keyframes i whose edge (i - 1, i) is scored
  for (int i = 0; i < n; ++i) {
    if (i == 0 && s->keyframes.empty()) continue;   // the first keyframe of all has no odometry edge
    if (has_cloud(i - 1) && has_cloud(i)) edge.push_back(i);
  }
  const bool keep_last = n > 0 && has_cloud(n - 1);
  if (edge.empty() && !keep_last) return 0;
  if (!s->seg) return set_error(SSLAM_ERR_INVALID, "the fitness model needs the frontend handle: none was given to sslam_slam_create");
  // the clouds the pairs name, each downsampled once: slot 0 = the cloud kept from the last tick, slot i + 1 = keyframe i of this one
  std::vector<int> cloud_of(n + 1, -1);
  std::vector<float> xyz;
  std::vector<int32_t> start{0};
  auto need = [&](int i) -> int {
    if (cloud_of[i + 1] >= 0) return 0;
    std::vector<float> ds;
    if (i < 0) ds = s->fit_prev;
    else { const int rc = downsampled_cloud(s, *s->keyframe_queue[i], s->fit_leaf, ds); if (rc < 0) return rc; }
    cloud_of[i + 1] = (int)start.size() - 1;
    xyz.insert(xyz.end(), ds.begin(), ds.end());
    start.push_back((int32_t)(xyz.size() / 3));
    return 0;
  };
  int rc;
  std::vector<sslam_fitness_pair> pairs;
  for (int i : edge) {
    if ((rc = need(i - 1)) < 0 || (rc = need(i)) < 0) return rc;
    const Pose& po = i == 0 ? s->keyframes.back()->odom : s->keyframe_queue[i - 1]->odom;
    const Pose rel = compose(inverse(po), s->keyframe_queue[i]->odom);
    sslam_fitness_pair P;
    P.target = cloud_of[i]; P.source = cloud_of[i + 1];
    const Mat3 R = qmat(rel.q);            // of the quaternion the edge's measurement carries
    for (int k = 0; k < 9; ++k) P.T[k] = R.m[k];
    P.T[9] = rel.t.x; P.T[10] = rel.t.y; P.T[11] = rel.t.z;
    P.max_range = s->fit_range;
    pairs.push_back(P);
  }
  if (keep_last && (rc = need(n - 1)) < 0) return rc;
  if (!pairs.empty()) {
    std::vector<double> sc(pairs.size());
    std::vector<int32_t> us(pairs.size());
    rc = sslam_seg_fitness_scores(s->seg, xyz.data(), start.data(), (int)start.size() - 1, pairs.data(), (int)pairs.size(), sc.data(), us.data(),
                                  nullptr, nullptr, nullptr);
    if (rc < 0) return rc;
    for (size_t k = 0; k < edge.size(); ++k) { score[edge[k]] = sc[k]; used[edge[k]] = us[k]; }
  }
  if (keep_last) {
    const int c = cloud_of[n];
    last_cloud.assign(xyz.begin() + 3 * (size_t)start[c], xyz.begin() + 3 * (size_t)start[c + 1]);
    last_has = true;
  }
  return 0;
}

// empty_keyframe_queue (semantic_graph_slam.cpp:104-150)
int empty_keyframe_queue(sslam_slam* s) {
  s->fit_score.clear(); s->fit_used.clear();
  if (s->keyframe_queue.empty()) return 0;
  const int n = std::min<int>((int)s->keyframe_queue.size(), s->P.max_keyframes_per_update);
  double info[36], const_info[36];
  odometry_information(s, const_info);
  std::memcpy(info, const_info, sizeof info);
  std::vector<double> score;
  std::vector<int32_t> nused;
  std::vector<float> last_cloud;
  bool last_has = false;
  if (s->fit_on) {
    const int rc = fitness_of_tick(s, n, score, nused, last_cloud, last_has);
    if (rc < 0) return rc;               // nothing has been touched: the queue keeps its keyframes
  }
  int err = 0, used = 0;
  for (int i = 0; i < n && !err; ++i) {
    const std::shared_ptr<KeyFrame>& kf = s->keyframe_queue[i];
    double tq[7];
    to_tq(kf->odom, tq);
    kf->node = sslam_graph_add_vertex_se3(s->graph, tq, -1);
    used = i + 1;
    if (kf->node < 0) { err = kf->node; break; }      // the keyframe is dropped: it never reached the graph
    s->new_keyframes.push_back(kf);
    if (i == 0 && s->keyframes.empty()) continue;
    const std::shared_ptr<KeyFrame>& prev = i == 0 ? s->keyframes.back() : s->keyframe_queue[i - 1];
    const Pose rel = compose(inverse(prev->odom), kf->odom);
    double z[7];
    to_tq(rel, z);
    if (s->fit_on) {
      if (nused[i] >= 0) { const int rc = sslam_information_from_fitness(&s->fit_P, score[i], info); if (rc < 0) { err = rc; break; } }
      else std::memcpy(info, const_info, sizeof info);
    }
    const int rc = sslam_graph_add_edge_se3(s->graph, prev->node, kf->node, z, info);
    if (rc < 0) { err = rc; break; }
    if (s->fit_on) { s->fit_score.push_back(score[i]); s->fit_used.push_back(nused[i]); }
  }
  if (s->fit_on) {   // the target of the next tick's first pair; after an error the chain of clouds is broken
    s->fit_prev_has = !err && last_has;
    if (s->fit_prev_has) s->fit_prev.swap(last_cloud); else { s->fit_prev.clear(); s->fit_prev.shrink_to_fit(); }
  }
  // whatever was touched leaves the queue, also on an error: a second call must not add the same keyframes again
  s->keyframe_queue.erase(s->keyframe_queue.begin(), s->keyframe_queue.begin() + (err ? used : n));
  return err ? err : 1;
}

// Eigen's fixed-size 3x3 inverse (cofactors times 1/det), as `covariance.inverse()` of a Matrix3f evaluates (semantic_graph_slam.cpp:170)
void inverse3f(const float* m, float* o) {
  const float c00 = m[4] * m[8] - m[5] * m[7], c10 = m[5] * m[6] - m[3] * m[8], c20 = m[3] * m[7] - m[4] * m[6];
  const float det = m[0] * c00 + m[1] * c10 + m[2] * c20;
  const float id = 1.0f / det;
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c10 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c20 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// empty_landmark_queue (semantic_graph_slam.cpp:152-179)
int empty_landmark_queue(sslam_slam* s, std::vector<sslam_landmark>& q, const KeyFrame& kf, sslam_tick_stats* st) {
  for (sslam_landmark& l : q) {
    if (l.is_new) {
      const double p[3] = {l.pose[0], l.pose[1], l.pose[2]};
      l.vertex = sslam_graph_add_vertex_point(s->graph, p);
      if (l.vertex < 0) return l.vertex;
      l.is_new = 0;
      s->landmarks[l.id].vertex = l.vertex;            // assignLandmarkNode (:163-164)
      if (st) st->landmarks_added++;
    } else {
      // a landmark created by an earlier detection of the same frame had no vertex yet when find_matches copied it; the earlier
      // record of this queue has assigned it by now
      if (l.vertex < 0) l.vertex = s->landmarks[l.id].vertex;
      if (st) st->landmarks_matched++;
    }
    float inf[9];
    inverse3f(l.covariance, inf);
    double z[3], info[9];
    for (int k = 0; k < 3; ++k) z[k] = l.local_pose[k];
    for (int k = 0; k < 9; ++k) info[k] = inf[k];
    const int rc = sslam_graph_add_edge_se3_point(s->graph, kf.node, l.vertex, z, info);
    if (rc < 0) return rc;
    if (st) st->landmark_edges_added++;
  }
  return 0;
}

// getAndSetLandmarkCov (semantic_graph_slam.cpp:181-205)
int get_and_set_landmark_cov(sslam_slam* s, sslam_tick_stats* st) {
  const int n = (int)s->landmarks.size();
  if (n == 0) { if (st) st->marginals_ok = 1; return 0; }   // computeMarginals over an empty pair list
  // the reference hands (hessianIndex, hessianIndex) pairs to computeMarginals (:186-191); the vertex ids name the same blocks and
  // spare one scan of the vertex list per landmark
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = s->landmarks[i].vertex;
  std::vector<double> blocks(9 * (size_t)n);
  const int rc = sslam_graph_marginals(s->graph, ids.data(), n, blocks.data());
  if (rc == SSLAM_ERR_NUMERIC || rc == SSLAM_ERR_INVALID) return 0;   // computeLandmarkMarginals returned false: covariances keep their values
  if (rc < 0) return rc;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 9; ++k) s->landmarks[i].covariance[k] = (float)blocks[9 * (size_t)i + k];   // setLandmarkCovs (:198-202)
  if (st) st->marginals_ok = 1;
  return 0;
}

// the segmented objects of every new keyframe that carries boxes: ONE batched frontend pass per tick (the reference runs
// segmentallPointCloudData keyframe by keyframe inside semantic_data_ass; the result does not depend on the association)
int segment_new_keyframes(sslam_slam* s) {
  std::vector<int> idx;
  for (size_t i = 0; i < s->new_keyframes.size(); ++i) {
    KeyFrame& kf = *s->new_keyframes[i];
    if (!kf.presegmented && !kf.boxes.empty()) idx.push_back((int)i);
  }
  if (idx.empty()) return 0;
  if (!s->seg) return set_error(SSLAM_ERR_INVALID, "a keyframe carries detection boxes but no frontend handle was given to sslam_slam_create");
  size_t a = 0;
  while (a < idx.size()) {   // runs of keyframes whose clouds share their geometry go through one call
    const KeyFrame& k0 = *s->new_keyframes[idx[a]];
    size_t b = a + 1;
    while (b < idx.size()) {
      const KeyFrame& k = *s->new_keyframes[idx[b]];
      if (k.width != k0.width || k.height != k0.height || k.point_step != k0.point_step || k.row_step != k0.row_step ||
          k.off[0] != k0.off[0] || k.off[1] != k0.off[1] || k.off[2] != k0.off[2]) break;
      ++b;
    }
    std::vector<sslam_frame> frames(b - a);
    int nbox = 0;
    for (size_t f = a; f < b; ++f) {
      KeyFrame& k = *s->new_keyframes[idx[f]];
      if (k.cloud.empty()) return set_error(SSLAM_ERR_INVALID, "keyframe with detection boxes has no point cloud");
      sslam_frame& F = frames[f - a];
      F.cloud = k.cloud.data(); F.boxes = k.boxes.data(); F.n_boxes = (int)k.boxes.size();
      pose_to_vector6(k.robot_pose, F.robot_pose);
      F.cam_angle = (float)s->cam_angle;
      nbox += F.n_boxes;
    }
    const int max_out = 64 * std::max(nbox, 1);
    std::vector<sslam_plane> planes(max_out);
    std::vector<int32_t> fr(max_out);
    const int np = sslam_seg_segment_batch(s->seg, frames.data(), (int)frames.size(), k0.width, k0.height, k0.point_step, k0.row_step,
                                           k0.off[0], k0.off[1], k0.off[2], planes.data(), max_out, fr.data());
    if (np < 0) return np;
    for (int k = 0; k < np; ++k) s->new_keyframes[idx[a + fr[k]]]->objects.push_back(planes[k]);
    a = b;
  }
  return 0;
}

// ---- loop closing (hdl_graph_slam's LoopDetector::detect [UPSTREAM]) -------------------------------------------------------------------
int check_loop_params(const sslam_loop_params* p, bool tick) {
  auto bad = [](double v) { return !std::isfinite(v) || v < 0; };
  if (bad(p->distance_thresh) || bad(p->accum_distance_thresh)) return set_error(SSLAM_ERR_INVALID, "loop closure: a distance threshold is negative or not finite");
  if (p->max_candidates < 0 || p->max_candidates > 64) return set_error(SSLAM_ERR_INVALID, "loop closure: max_candidates %d outside 0 .. 64", p->max_candidates);
  if (!tick) return 0;
  if (bad(p->distance_from_last_edge_thresh) || bad(p->fitness_score_max_range) || bad(p->fitness_score_thresh) || bad(p->gate_chi2) || bad(p->voxel_leaf))
    return set_error(SSLAM_ERR_INVALID, "loop closure: a threshold is negative or not finite");
  if (p->max_iterations < 0) return set_error(SSLAM_ERR_INVALID, "loop closure: negative max_iterations");
  if (!(p->epsilon >= 0)) return set_error(SSLAM_ERR_INVALID, "loop closure: epsilon is negative or NaN");
  if (p->robust_kernel < SSLAM_ROBUST_NONE || p->robust_kernel > SSLAM_ROBUST_DCS)
    return set_error(SSLAM_ERR_INVALID, "loop closure: robust kernel kind %d: 0 .. 7 (SSLAM_ROBUST_*)", p->robust_kernel);
  if (p->robust_kernel != SSLAM_ROBUST_NONE && !(std::isfinite(p->robust_delta) && p->robust_delta > 0))
    return set_error(SSLAM_ERR_INVALID, "loop closure: robust kernel width must be finite and > 0");
  return 0;
}

// k_loop_candidates over host tables: both go up, the rows and counts come down, through the pinned scratch on the handle's stream
int loop_candidates(sslam_slam* s, const double* keys, int n_keys, const double* news, int n_new, const sslam_loop_params& P,
                    int32_t* cand_out, int32_t* count_out, int cap) {
  if (n_new == 0) return 0;
  int rc = ensure_stream(s);
  if (rc) return rc;
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  const size_t n_tab = 3 * ((size_t)n_keys + n_new), n_cand = (size_t)n_new * cap, n_out = n_cand + n_new;
  if ((rc = s->d_ltab.reserve(n_tab, s->stream, 0))) return rc;
  if ((rc = s->d_lout.reserve(n_out, s->stream, 0))) return rc;
  const size_t tab_bytes = n_tab * sizeof(double), out_bytes = n_out * sizeof(int32_t);
  std::vector<char> fallback;
  char* stage = s->pin.get(tab_bytes + out_bytes);
  if (!stage) { fallback.resize(tab_bytes + out_bytes); stage = fallback.data(); }
  double* tab = reinterpret_cast<double*>(stage);
  if (n_keys) std::memcpy(tab, keys, 3 * (size_t)n_keys * sizeof(double));
  std::memcpy(tab + 3 * (size_t)n_keys, news, 3 * (size_t)n_new * sizeof(double));
  LoopCandArgs A;
  A.keys = s->d_ltab.p; A.news = s->d_ltab.p + 3 * (size_t)n_keys;
  A.n_keys = n_keys; A.n_new = n_new;
  A.accum_thresh = P.accum_distance_thresh;
  A.d2_thresh = P.distance_thresh * P.distance_thresh;
  A.m = P.max_candidates; A.cap = cap;
  A.cand = s->d_lout.p; A.count = s->d_lout.p + n_cand;
  SSLAM_HIP_TRY(hipMemcpyAsync(s->d_ltab.p, tab, tab_bytes, hipMemcpyHostToDevice, s->stream));
  if (n_cand) SSLAM_HIP_TRY(hipMemsetAsync(s->d_lout.p, 0xff, n_cand * sizeof(int32_t), s->stream));   // -1: not filled
  hipLaunchKernelGGL(k_loop_candidates, dim3(n_new), dim3(kLoopWave), 0, s->stream, A);
  SSLAM_HIP_TRY(hipGetLastError());
  SSLAM_HIP_TRY(hipMemcpyAsync(stage + tab_bytes, s->d_lout.p, out_bytes, hipMemcpyDeviceToHost, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  if (n_cand) std::memcpy(cand_out, stage + tab_bytes, n_cand * sizeof(int32_t));
  std::memcpy(count_out, stage + tab_bytes + n_cand * sizeof(int32_t), (size_t)n_new * sizeof(int32_t));
  return 0;
}

// T (R row-major, then t) -> the edge's measurement (t, q xyzw): the quaternion of a rotation matrix by the branch with the largest
// pivot, operation for operation as INTEGRATION.md section 2 spells it out for a caller
void measurement_of_T(const double* R, double z[7]) {
  z[0] = R[9]; z[1] = R[10]; z[2] = R[11]; z[3] = 0; z[4] = 0; z[5] = 0; z[6] = 1;
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0)                          { const double q = 2 * std::sqrt(1 + tr);                 z[6] = q / 4; z[3] = (R[7] - R[5]) / q; z[4] = (R[2] - R[6]) / q; z[5] = (R[3] - R[1]) / q; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double q = 2 * std::sqrt(1 + R[0] - R[4] - R[8]); z[3] = q / 4; z[6] = (R[7] - R[5]) / q; z[4] = (R[1] + R[3]) / q; z[5] = (R[2] + R[6]) / q; }
  else if (R[4] > R[8])                { const double q = 2 * std::sqrt(1 + R[4] - R[0] - R[8]); z[4] = q / 4; z[6] = (R[2] - R[6]) / q; z[3] = (R[1] + R[3]) / q; z[5] = (R[5] + R[7]) / q; }
  else                                 { const double q = 2 * std::sqrt(1 + R[8] - R[0] - R[4]); z[5] = q / 4; z[6] = (R[3] - R[1]) / q; z[3] = (R[2] + R[6]) / q; z[4] = (R[5] + R[7]) / q; }
}

// loop registration GICP: the covariances of a keyframe's downsampled cloud, once per keyframe
int keyframe_covariances(sslam_slam* s, KeyFrame& kf) {
  if (s->loop_method != SSLAM_REG_GICP || !kf.has_ds || kf.cov.size() == 2 * kf.ds.size()) return 0;
  const int32_t start[2] = {0, (int32_t)(kf.ds.size() / 3)};
  kf.cov.resize(2 * kf.ds.size());
  const int rc = sslam_seg_cloud_covariances(s->seg, kf.ds.data(), start, 1, s->loop_gicp.k, s->loop_gicp.plane_epsilon, kf.cov.data(), nullptr, nullptr);
  if (rc < 0) { kf.cov.clear(); return rc; }
  s->loop_cov_passes += 1;
  return 0;
}

// the downsampled cloud of every new keyframe that carries one; before the association loop, which drops the raw clouds
int downsample_new_keyframes(sslam_slam* s) {
  for (auto& kf : s->new_keyframes) {
    if (kf->cloud.empty() || kf->has_ds) continue;
    int rc = downsampled_cloud(s, *kf, s->loop_P.voxel_leaf, kf->ds);
    if (rc < 0) return rc;
    kf->has_ds = !kf->ds.empty();
    if ((rc = keyframe_covariances(s, *kf)) < 0) return rc;      // nothing to do without a cloud or with SSLAM_REG_ICP
  }
  return 0;
}

// map clouds: the downsampled cloud of every new keyframe that carries one goes to the device ONCE, behind the clouds already there;
// before the association loop, which drops the raw clouds.  The boundary of a new cloud is written by a device fill: only points travel.
int keep_map_clouds(sslam_slam* s) {
  for (auto& kf : s->new_keyframes) {
    if (kf->cloud.empty() || kf->map_done) continue;
    std::vector<float> own;
    const bool share = s->loop_on && kf->has_ds && s->loop_P.voxel_leaf == s->map_leaf;   // equal leaves: the same cloud
    int rc;
    if (!share && (rc = downsampled_cloud(s, *kf, s->map_leaf, own)) < 0) return rc;
    const std::vector<float>& ds = share ? kf->ds : own;
    kf->map_done = true;
    if (ds.empty()) continue;
    if ((rc = ensure_stream(s))) return rc;
    SSLAM_HIP_TRY(hipSetDevice(s->P.device));
    const size_t have = 3 * (size_t)s->map_start.back(), n_cl = s->map_kf.size();
    if (have / 3 + ds.size() / 3 > (size_t)INT32_MAX) return set_error(SSLAM_ERR_UNSUPPORTED, "map clouds: more than 2^31 - 1 points kept");
    if ((rc = s->d_map_xyz.reserve(have + ds.size(), s->stream, have))) return rc;
    if ((rc = s->d_map_start.reserve(n_cl + 2, s->stream, n_cl + 1))) return rc;
    const int32_t end = (int32_t)((have + ds.size()) / 3);
    SSLAM_HIP_TRY(hipMemcpyAsync(s->d_map_xyz.p + have, ds.data(), ds.size() * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (n_cl == 0) SSLAM_HIP_TRY(hipMemsetAsync(s->d_map_start.p, 0, sizeof(int32_t), s->stream));
    SSLAM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(s->d_map_start.p + n_cl + 1), end, 1, s->stream));
    SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
    s->map_start.push_back(end);
    s->map_kf.push_back(kf);
    s->map_pending_bytes += (int64_t)(ds.size() * sizeof(float));
  }
  return 0;
}

// The resident clouds are allocated on the orchestrator's device and read by the frontend's kernels on the frontend's: one device, or no map.
int map_same_device(const sslam_slam* s) {
  const int d = seg_device_index(s->seg);
  if (d == s->P.device) return 0;
  return set_error(SSLAM_ERR_UNSUPPORTED, "map clouds: the orchestrator runs on device %d and its frontend handle on device %d; the kept clouds are read by "
                   "the frontend's kernels, so both must be the same device", s->P.device, d);
}

void drop_map_clouds(sslam_slam* s) {
  s->d_map_xyz.release(); s->d_map_pose.release(); s->d_map_start.release();
  s->map_start.assign(1, 0);
  s->map_kf.clear();
  s->map_pending_bytes = 0;
  for (auto* list : {&s->keyframes, &s->new_keyframes})
    for (auto& kf : *list) kf->map_done = false;
}

// steps 1 - 7 of sslam_slam_set_loop_closure (include/sslam.h)
int close_loops(sslam_slam* s) {
  const sslam_loop_params& P = s->loop_P;
  struct Entry { int kf; Pose est; };
  auto entry = [&](const std::vector<std::shared_ptr<KeyFrame>>& list, int i, std::vector<Entry>& out, std::vector<double>& tab) -> int {
    double tq[7];
    if (sslam_graph_get_vertex(s->graph, list[i]->node, tq) < 0) return SSLAM_ERR_INVALID;
    out.push_back(Entry{i, from_tq(tq)});
    tab.push_back(tq[0]); tab.push_back(tq[1]); tab.push_back(list[i]->accum_distance);
    return 0;
  };
  std::vector<Entry> olds, news;
  std::vector<double> keys, qs;
  int rc;
  for (int i = 0; i < (int)s->new_keyframes.size(); ++i) {
    const KeyFrame& kf = *s->new_keyframes[i];
    if (!kf.has_ds || kf.accum_distance - s->last_edge_accum < P.distance_from_last_edge_thresh) continue;
    if ((rc = entry(s->new_keyframes, i, news, qs)) < 0) return rc;
  }
  if (news.empty()) return 0;
  for (int i = 0; i < (int)s->keyframes.size(); ++i)
    if (s->keyframes[i]->has_ds && (rc = entry(s->keyframes, i, olds, keys)) < 0) return rc;
  if (olds.empty()) return 0;
  const int n_new = (int)news.size(), n_keys = (int)olds.size();
  const int cap = P.max_candidates ? P.max_candidates : n_keys;
  std::vector<int32_t> cand((size_t)n_new * cap), count(n_new);
  double t0 = now_s();
  if ((rc = loop_candidates(s, keys.data(), n_keys, qs.data(), n_new, P, cand.data(), count.data(), cap)) < 0) return rc;
  s->loop_seconds[0] = now_s() - t0;
  // every (new, candidate) pair of the tick through one registration call; each cloud is packed once
  std::vector<float> xyz;
  std::vector<int32_t> start{0};
  std::vector<int> cloud_of_old(n_keys, -1), first_pair(n_new, 0);
  const bool gicp = s->loop_method == SSLAM_REG_GICP;
  std::vector<double> cov;                // GICP: the kept covariances of the packed clouds, in step with xyz
  auto pack = [&](KeyFrame& kf) -> int {
    if (gicp) {                           // a keyframe downsampled before GICP was chosen gets its covariances here, once
      const int rcc = keyframe_covariances(s, kf);
      if (rcc < 0) return rcc;
      cov.insert(cov.end(), kf.cov.begin(), kf.cov.end());
    }
    xyz.insert(xyz.end(), kf.ds.begin(), kf.ds.end()); start.push_back((int32_t)(xyz.size() / 3)); return (int)start.size() - 2;
  };
  std::vector<sslam_reg_pair> pairs;
  for (int j = 0; j < n_new; ++j) {
    first_pair[j] = (int)pairs.size();
    const int nc = std::min<int>(count[j], cap);
    if (nc == 0) continue;
    const int target = pack(*s->new_keyframes[news[j].kf]);
    if (target < 0) return target;
    const Pose inv = inverse(news[j].est);
    for (int c = 0; c < nc; ++c) {
      const int k = cand[(size_t)j * cap + c];
      if (cloud_of_old[k] < 0 && (cloud_of_old[k] = pack(*s->keyframes[olds[k].kf])) < 0) return cloud_of_old[k];
      const Pose rel = compose(inv, olds[k].est);
      sslam_reg_pair R;
      R.target = target; R.source = cloud_of_old[k];
      const Mat3 M = qmat(rel.q);
      for (int q = 0; q < 9; ++q) R.T0[q] = M.m[q];
      R.T0[9] = rel.t.x; R.T0[10] = rel.t.y; R.T0[11] = rel.t.z;
      R.max_corr2 = P.fitness_score_max_range;
      pairs.push_back(R);
    }
  }
  if (pairs.empty()) return 0;
  std::vector<sslam_reg_result> reg(pairs.size());
  t0 = now_s();
  if (gicp)
    rc = sslam_seg_register_pairs_gicp(s->seg, xyz.data(), start.data(), (int)start.size() - 1, pairs.data(), (int)pairs.size(), cov.data(), &s->loop_gicp,
                                       P.max_iterations, P.epsilon, reg.data(), nullptr, nullptr, nullptr);
  else
    rc = sslam_seg_register_pairs(s->seg, xyz.data(), start.data(), (int)start.size() - 1, pairs.data(), (int)pairs.size(), P.max_iterations, P.epsilon,
                                  reg.data(), nullptr, nullptr, nullptr);
  s->loop_seconds[1] = now_s() - t0;
  if (rc < 0) return rc;
  // the best pair of every new keyframe; its measurement and information where it passes the score test
  struct Best { int pair = -1, key = -1; double z[7], info[36], d2 = NAN; bool scored = false; };
  std::vector<Best> best(n_new);
  std::vector<int32_t> gate_cand;
  std::vector<double> gate_z, gate_info;
  std::vector<int> gate_of;
  for (int j = 0; j < n_new; ++j) {
    Best& B = best[j];
    const int nc = std::min<int>(count[j], cap);
    for (int c = 0; c < nc; ++c) {
      const sslam_reg_result& r = reg[first_pair[j] + c];
      const int k = cand[(size_t)j * cap + c];
      if (r.status != 0 || r.used <= 0) continue;
      if (B.pair < 0 || r.score < reg[B.pair].score || (r.score == reg[B.pair].score && k < B.key)) { B.pair = first_pair[j] + c; B.key = k; }
    }
    if (B.pair < 0 || reg[B.pair].score > P.fitness_score_thresh) continue;
    B.scored = true;
    measurement_of_T(reg[B.pair].T, B.z);
    if ((rc = sslam_information_from_fitness(&P.inf, reg[B.pair].score, B.info)) < 0) return rc;
    if (P.gate_chi2 > 0) {
      gate_cand.push_back(SSLAM_GATE_SE3);
      gate_cand.push_back(s->new_keyframes[news[j].kf]->node);
      gate_cand.push_back(s->keyframes[olds[B.key].kf]->node);
      gate_z.insert(gate_z.end(), B.z, B.z + 7);
      gate_info.insert(gate_info.end(), B.info, B.info + 36);
      gate_of.push_back(j);
    }
  }
  if (!gate_of.empty()) {   // one call for the whole tick, before any loop edge is added
    std::vector<double> d2(gate_of.size());
    t0 = now_s();
    rc = sslam_graph_gate(s->graph, gate_cand.data(), gate_z.data(), gate_info.data(), (int)gate_of.size(), d2.data(), nullptr, nullptr);
    s->loop_seconds[2] = now_s() - t0;
    if (rc < 0) return rc;
    for (size_t g = 0; g < gate_of.size(); ++g) best[gate_of[g]].d2 = d2[g];
  }
  // the new keyframes in order, as hdl's sequential loop meets them
  for (int j = 0; j < n_new; ++j) {
    const KeyFrame& kf = *s->new_keyframes[news[j].kf];
    if (kf.accum_distance - s->last_edge_accum < P.distance_from_last_edge_thresh) continue;
    if (count[j] <= 0) continue;
    const Best& B = best[j];
    sslam_loop L;
    std::memset(&L, 0, sizeof L);
    L.new_vertex = kf.node; L.cand_vertex = -1; L.n_candidates = count[j]; L.edge_id = -1;
    L.score = DBL_MAX; L.d2 = NAN;
    if (B.pair < 0) {
      L.outcome = SSLAM_LOOP_NO_MATCH;
    } else {
      const sslam_reg_result& r = reg[B.pair];
      const KeyFrame& ck = *s->keyframes[olds[B.key].kf];
      L.cand_vertex = ck.node;
      std::memcpy(L.T, r.T, sizeof L.T);
      L.score = r.score; L.used = r.used; L.iterations = r.iterations; L.converged = r.converged;
      if (!B.scored) {
        L.outcome = SSLAM_LOOP_SCORE;
      } else {
        L.d2 = B.d2;
        if (P.gate_chi2 > 0 && !(B.d2 < P.gate_chi2)) {
          L.outcome = SSLAM_LOOP_GATE;
        } else {
          const int eid = sslam_graph_add_edge_se3(s->graph, kf.node, ck.node, B.z, B.info);
          if (eid < 0) return eid;
          if (P.robust_kernel != SSLAM_ROBUST_NONE && (rc = sslam_graph_set_edge_robust_kernel(s->graph, eid, P.robust_kernel, P.robust_delta)) < 0) return rc;
          s->last_edge_accum = kf.accum_distance;
          L.outcome = SSLAM_LOOP_ADDED; L.edge_id = eid;
        }
      }
    }
    s->loops.push_back(L);
  }
  return 0;
}

}  // namespace

extern "C" {

void sslam_slam_default_params(sslam_slam_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->keyframe_delta_trans = 0.5; p->keyframe_delta_angle = 0.5; p->keyframe_delta_time = 1.0;
  p->max_keyframes_per_update = 10;
  p->first_lan[0] = 1.8; p->first_lan[1] = 0; p->first_lan[2] = 0.3;
  p->use_const_inf_matrix = 1;
  p->maha_dist_thres = 0.5; p->eq_dist_thres = 1.21; p->land_noise_low = 0.5; p->land_noise_high = 0.9;
  p->use_maha_dist = 1;
  p->max_iterations = 1024;
}

sslam_slam* sslam_slam_create(const sslam_slam_params* p, sslam_seg* seg) {
  sslam_slam_params P;
  if (p) P = *p; else sslam_slam_default_params(&P);
  if (!P.use_const_inf_matrix) {
    set_error(SSLAM_ERR_UNSUPPORTED, "use_const_inf_matrix = false reads uninitialised members in the reference (information_matrix_calculator.hpp:31-36)");
    return nullptr;
  }
  if (P.max_keyframes_per_update <= 0) { set_error(SSLAM_ERR_INVALID, "max_keyframes_per_update must be positive"); return nullptr; }
  sslam_slam* s = new sslam_slam();
  s->P = P;
  s->seg = seg;
  s->graph = sslam_graph_create(P.device);
  s->cam_angle = P.camera_angle_deg * (M_PI / 180);
  if (P.add_first_lan) {   // addFirstPoseAndLandmark (semantic_graph_slam.cpp:289-329)
    sslam_landmark l;
    std::memset(&l, 0, sizeof l);
    l.is_new = 1; l.id = 0; l.vertex = -1; l.class_id = SSLAM_CLASS_BUCKET; l.plane_type = 1;
    for (int k = 0; k < 3; ++k) l.pose[k] = l.local_pose[k] = (float)P.first_lan[k];
    l.normal[0] = -0.4f; l.normal[1] = 0.86f;
    l.covariance[0] = l.covariance[4] = l.covariance[8] = 0.1f;
    s->first_object = false;                    // addFirstLandmark (data_association.h:70-73)
    s->landmarks.push_back(l);
    auto kf = std::make_shared<KeyFrame>();
    kf->robot_pose = s->robot_pose;
    s->keyframe_queue.push_back(kf);
    if (empty_keyframe_queue(s) > 0) {
      std::vector<sslam_landmark> q{l};
      for (auto& k : s->new_keyframes) (void)empty_landmark_queue(s, q, *k, nullptr);
      for (auto& k : s->new_keyframes) s->keyframes.push_back(k);
      s->new_keyframes.clear();
    }
  }
  return s;
}

void sslam_slam_destroy(sslam_slam* s) { delete s; }

int sslam_slam_set_point_cloud(sslam_slam* s, const uint8_t* cloud, int width, int height, int point_step, int row_step, int off_x, int off_y, int off_z) {
  if (!s || !cloud || width <= 0 || height <= 0 || point_step <= 0 || row_step < width * point_step)
    return set_error(SSLAM_ERR_INVALID, "bad point cloud");
  s->point_cloud_available = true;
  KeyFrame& L = s->latest;
  L.cloud.assign(cloud, cloud + (size_t)row_step * height);
  L.width = width; L.height = height; L.point_step = point_step; L.row_step = row_step;
  L.off[0] = off_x; L.off[1] = off_y; L.off[2] = off_z;
  return 0;
}

int sslam_slam_set_detected_objects(sslam_slam* s, const sslam_box* boxes, int n) {
  if (!s || n < 0 || (n > 0 && !boxes)) return set_error(SSLAM_ERR_INVALID, "bad box list");
  s->object_detection_available = true;
  s->latest.boxes.assign(boxes, boxes + n);
  s->segmented_available = false;
  return 0;
}

int sslam_slam_set_segmented_objects(sslam_slam* s, const sslam_plane* objects, int n) {
  if (!s || n < 0 || (n > 0 && !objects)) return set_error(SSLAM_ERR_INVALID, "bad object list");
  s->object_detection_available = true;
  s->segmented_available = true;
  s->latest.objects.assign(objects, objects + n);
  return 0;
}

int sslam_slam_vio(sslam_slam* s, int32_t sec, int32_t nsec, const double odom_tq[7]) {
  if (!s || !odom_tq) return set_error(SSLAM_ERR_INVALID, "null argument");
  const Pose odom = from_tq(odom_tq);
  // KeyframeUpdater::update (keyframe_updater.hpp:41-65)
  bool accept;
  if (s->is_first) {
    s->is_first = false; s->prev_sec = sec; s->prev_nsec = nsec; s->prev_keypose = odom;
    accept = true;
  } else {
    const Pose delta = compose(inverse(s->prev_keypose), odom);
    const double dx = std::sqrt(dot(delta.t, delta.t));
    // Eigen::Quaterniond(delta.linear()).w(): the matrix -> quaternion conversion yields w >= 0, whatever the sign of the odometry
    // quaternions that went in (q and -q are the same rotation)
    const double da = std::acos(std::min(1.0, std::fabs(delta.q.w)));
    // ros::Duration::sec: whole seconds of the normalised difference (nsec part in [0, 1e9))
    int64_t dsec = (int64_t)sec - s->prev_sec, dnsec = (int64_t)nsec - s->prev_nsec;
    if (dnsec < 0) { dnsec += 1000000000; dsec -= 1; }
    if ((double)dsec < s->P.keyframe_delta_time && dx < s->P.keyframe_delta_trans && da < s->P.keyframe_delta_angle) {
      accept = false;
    } else {
      s->accum_distance += dx; s->prev_keypose = odom; s->prev_sec = sec; s->prev_nsec = nsec;
      accept = true;
    }
  }
  const bool reject = s->P.update_keyframes_using_detections ? (!accept && !s->object_detection_available) : !accept;
  if (reject) {   // semantic_graph_slam.cpp:239-262
    if (s->first_key_added) s->robot_pose = compose(s->robot_pose, compose(inverse(s->prev_odom), odom));
    s->vio_pose = odom; s->prev_odom = odom;
    return 0;
  }
  auto kf = std::make_shared<KeyFrame>();
  kf->sec = sec; kf->nsec = nsec; kf->odom = odom; kf->robot_pose = s->robot_pose; kf->accum_distance = s->accum_distance;
  // getPointCloudData / getDetectedObjectInfo (semantic_graph_slam.cpp:264-272): the latest cloud always, the boxes when a detection is pending
  const bool fresh_cloud = s->point_cloud_available;
  s->point_cloud_available = false;
  if (s->object_detection_available) {
    s->object_detection_available = false;
    if (s->segmented_available) { kf->objects = s->latest.objects; kf->presegmented = true; s->segmented_available = false; }
    else {
      kf->boxes = s->latest.boxes;
      kf->cloud = s->latest.cloud;
      kf->width = s->latest.width; kf->height = s->latest.height; kf->point_step = s->latest.point_step; kf->row_step = s->latest.row_step;
      for (int k = 0; k < 3; ++k) kf->off[k] = s->latest.off[k];
    }
  }
  if ((s->fit_on || s->loop_on || s->map_on) && fresh_cloud && kf->cloud.empty() && !s->latest.cloud.empty()) {   // the fitness model, loop closure and the map clouds read the cloud of a keyframe without boxes too
    kf->cloud = s->latest.cloud;
    kf->width = s->latest.width; kf->height = s->latest.height; kf->point_step = s->latest.point_step; kf->row_step = s->latest.row_step;
    for (int k = 0; k < 3; ++k) kf->off[k] = s->latest.off[k];
  }
  s->keyframe_queue.push_back(kf);
  s->vio_pose = odom; s->prev_odom = odom;
  return 1;
}

int sslam_slam_run(sslam_slam* s, sslam_tick_stats* st) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  sslam_tick_stats local;
  if (!st) st = &local;
  std::memset(st, 0, sizeof *st);
  s->loops.clear();
  for (double& v : s->loop_seconds) v = 0;
  // on an error after the queue was touched the bookkeeping is completed before the error is returned (the keyframes that reached the
  // graph move to `keyframes`): the next call must neither add them again nor associate them a second time
  auto fail = [&](int code) {
    for (auto& kf : s->new_keyframes) { kf->cloud.clear(); kf->cloud.shrink_to_fit(); s->keyframes.push_back(kf); }
    s->new_keyframes.clear();
    s->table_dirty = true;
    return code;
  };
  int rc = empty_keyframe_queue(s);
  if (rc < 0) return fail(rc);
  if (rc == 0) return 0;
  st->keyframes_added = (int)s->new_keyframes.size();
  double t0 = now_s();
  const double t_loop = t0;
  if (s->loop_on) {
    if ((rc = downsample_new_keyframes(s)) < 0) return fail(rc);
    s->loop_seconds[3] = now_s() - t_loop;
    t0 = now_s();
  }
  if (s->map_on) {
    if ((rc = keep_map_clouds(s)) < 0) return fail(rc);
    t0 = now_s();
  }
  if ((rc = segment_new_keyframes(s)) < 0) return fail(rc);
  st->seconds_frontend = now_s() - t0;
  t0 = now_s();
  for (auto& kfp : s->new_keyframes) {   // semantic_graph_slam.cpp:62-70
    KeyFrame& kf = *kfp;
    if (kf.presegmented ? kf.objects.empty() : kf.boxes.empty()) continue;
    float rp[6];
    pose_to_vector6(kf.robot_pose, rp);
    std::vector<sslam_landmark> cur;
    if ((rc = find_matches(s, kf.objects.data(), (int)kf.objects.size(), rp, cur)) < 0) return fail(rc);
    if ((rc = empty_landmark_queue(s, cur, kf, st)) < 0) return fail(rc);
    kf.cloud.clear(); kf.cloud.shrink_to_fit();
  }
  st->seconds_association = now_s() - t0;
  if (s->loop_on) {   // where hdl calls LoopDetector::detect: the new keyframes are in the graph, nothing is optimised yet
    t0 = now_s();
    rc = close_loops(s);
    s->loop_seconds[3] += now_s() - t0;
    if (rc < 0) return fail(rc);
  }
  for (auto& kf : s->new_keyframes) {
    if (s->fit_on || s->loop_on || s->map_on) { kf->cloud.clear(); kf->cloud.shrink_to_fit(); }   // only downsampled clouds are kept
    s->keyframes.push_back(kf);
  }
  s->new_keyframes.clear();
  t0 = now_s();
  rc = sslam_graph_optimize(s->graph, s->P.max_iterations, &st->opt);
  st->seconds_optimize = now_s() - t0;
  if (rc < 0 && rc != SSLAM_ERR_TOO_FEW_EDGES && rc != SSLAM_ERR_NUMERIC) return rc;
  if (rc != SSLAM_ERR_TOO_FEW_EDGES) {   // GraphSLAM::optimize returns true whatever LM did (graph_slam.cpp:218)
    st->optimized = 1;
    t0 = now_s();
    if ((rc = get_and_set_landmark_cov(s, st)) < 0) return rc;
    st->seconds_marginals = now_s() - t0;
    s->table_dirty = true;               // estimates and covariances moved
    const KeyFrame& last = *s->keyframes.back();
    double tq[7];
    if ((rc = sslam_graph_get_vertex(s->graph, last.node, tq)) < 0) return rc;
    s->robot_pose = from_tq(tq);
    s->map2odom = compose(s->robot_pose, inverse(last.odom));
  }
  s->first_key_added = true;
  return 1;
}

int sslam_slam_robot_pose(const sslam_slam* s, double tq[7]) {
  if (!s || !tq) return set_error(SSLAM_ERR_INVALID, "null argument");
  to_tq(s->robot_pose, tq);
  return 0;
}
int sslam_slam_map2odom(const sslam_slam* s, double tq[7]) {
  if (!s || !tq) return set_error(SSLAM_ERR_INVALID, "null argument");
  to_tq(s->map2odom, tq);
  return 0;
}
int sslam_slam_landmarks(const sslam_slam* s, sslam_landmark* out, int max) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  const int n = (int)s->landmarks.size();
  for (int i = 0; i < n && i < max && out; ++i) {
    out[i] = s->landmarks[i];
  }
  return n;
}
int sslam_slam_keyframes(const sslam_slam* s, int32_t* ids, double* est, int max) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  const int n = (int)s->keyframes.size();
  for (int i = 0; i < n && i < max; ++i) {
    if (ids) ids[i] = s->keyframes[i]->node;
    if (est && sslam_graph_get_vertex(s->graph, s->keyframes[i]->node, est + 7 * (size_t)i) < 0) return SSLAM_ERR_INVALID;
  }
  return n;
}
sslam_graph* sslam_slam_graph(sslam_slam* s) { return s ? s->graph : nullptr; }

int sslam_slam_set_fitness_information(sslam_slam* s, const sslam_inf_params* p, float voxel_leaf, double max_range) {
  if (!s || !std::isfinite(voxel_leaf) || voxel_leaf < 0 || !std::isfinite(max_range)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  s->fit_on = p != nullptr;
  if (p) s->fit_P = *p;
  s->fit_leaf = voxel_leaf == 0 ? 0.1f : voxel_leaf;
  s->fit_range = max_range <= 0 ? DBL_MAX : max_range;
  if (!s->fit_on) { s->fit_prev_has = false; s->fit_prev.clear(); s->fit_prev.shrink_to_fit(); }
  return 0;
}

int sslam_slam_last_fitness(const sslam_slam* s, double* score, int32_t* used, int max) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  const int n = (int)s->fit_score.size();
  for (int i = 0; i < n && i < max; ++i) {
    if (score) score[i] = s->fit_score[i];
    if (used) used[i] = s->fit_used[i];
  }
  return n;
}

void sslam_loop_default_params(sslam_loop_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  // hdl_graph_slam's defaults [UPSTREAM, unverified here]
  p->distance_thresh = 5.0; p->accum_distance_thresh = 8.0; p->distance_from_last_edge_thresh = 5.0;
  p->fitness_score_max_range = DBL_MAX; p->fitness_score_thresh = 0.5;
  p->max_iterations = 64; p->epsilon = 0.01;
  p->max_candidates = 0; p->voxel_leaf = 0.1f; p->gate_chi2 = 0;
  p->robust_kernel = SSLAM_ROBUST_HUBER; p->robust_delta = 1.0;
  sslam_inf_default_params(&p->inf);
}

int sslam_slam_set_loop_closure(sslam_slam* s, const sslam_loop_params* p) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  if (!p) {
    s->loop_on = false;
    s->last_edge_accum = 0;
    for (auto* list : {&s->keyframes, &s->new_keyframes})
      for (auto& kf : *list) { kf->ds.clear(); kf->ds.shrink_to_fit(); kf->has_ds = false; kf->cov.clear(); kf->cov.shrink_to_fit(); }
    return 0;
  }
  const int rc = check_loop_params(p, true);
  if (rc < 0) return rc;
  if (!s->seg) return set_error(SSLAM_ERR_INVALID, "loop closure needs the frontend handle: none was given to sslam_slam_create");
  s->loop_on = true;
  s->loop_P = *p;
  if (s->loop_P.voxel_leaf == 0) s->loop_P.voxel_leaf = 0.1f;
  return 0;
}

int sslam_slam_set_loop_registration(sslam_slam* s, int method, const sslam_gicp_params* p) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  if (method != SSLAM_REG_ICP && method != SSLAM_REG_GICP) return set_error(SSLAM_ERR_INVALID, "loop registration: method %d: SSLAM_REG_ICP or SSLAM_REG_GICP", method);
  sslam_gicp_params g;
  sslam_gicp_default_params(&g);
  if (p) g = *p;
  const int rc = gicp_check_params(g.k, g.plane_epsilon);
  if (rc) return rc;
  if (method != s->loop_method || g.k != s->loop_gicp.k || g.plane_epsilon != s->loop_gicp.plane_epsilon)   // kept covariances belong to other parameters
    for (auto* list : {&s->keyframes, &s->new_keyframes})
      for (auto& kf : *list) { kf->cov.clear(); kf->cov.shrink_to_fit(); }
  s->loop_method = method;
  s->loop_gicp = g;
  return 0;
}

int sslam_slam_loop_covariance_passes(const sslam_slam* s, int64_t* clouds) {
  if (!s || !clouds) return set_error(SSLAM_ERR_INVALID, "null argument");
  *clouds = s->loop_cov_passes;
  return 0;
}

int sslam_slam_last_loops(const sslam_slam* s, sslam_loop* out, int max) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  const int n = (int)s->loops.size();
  for (int i = 0; i < n && i < max && out; ++i) out[i] = s->loops[i];
  return n;
}

int sslam_slam_last_loop_timing(const sslam_slam* s, double seconds[4]) {
  if (!s || !seconds) return set_error(SSLAM_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) seconds[k] = s->loop_seconds[k];
  return 0;
}

int sslam_slam_set_map_clouds(sslam_slam* s, int on, float keyframe_leaf) {
  if (!s || !std::isfinite(keyframe_leaf) || keyframe_leaf < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (on && !s->seg) return set_error(SSLAM_ERR_INVALID, "map clouds need the frontend handle: none was given to sslam_slam_create");
  int rc;
  if (on && (rc = map_same_device(s))) return rc;
  s->map_on = on != 0;
  s->map_leaf = keyframe_leaf == 0 ? 0.1f : keyframe_leaf;
  if (!s->map_on) drop_map_clouds(s);
  return 0;
}

int sslam_slam_map_clouds_kept(const sslam_slam* s, int32_t* n_points) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "null handle");
  if (n_points) *n_points = s->map_start.back();
  return (int)s->map_kf.size();
}

// the kept clouds at the current estimates, ready for the frontend's kernels: the pose of every cloud's keyframe (quaternion normalised, R by
// qmat as in the loop stage) goes to the device, 48 bytes each.  *sent: those bytes plus the cloud bytes sent since the last map call.
static int map_poses_to_device(sslam_slam* s, const char* what, int32_t* vertex_out, double* poses_out, int max_clouds, MapCloudIn* in, int64_t* sent) {
  const int n = (int)s->map_kf.size();
  int rc;
  std::vector<float> pose(12 * (size_t)n);
  for (int c = 0; c < n; ++c) {
    const KeyFrame& kf = *s->map_kf[c];
    double tq[7], T[12];
    if (sslam_graph_get_vertex(s->graph, kf.node, tq) < 0) return SSLAM_ERR_INVALID;
    const Pose est = from_tq(tq);
    const Mat3 R = qmat(est.q);
    for (int k = 0; k < 9; ++k) T[k] = R.m[k];
    T[9] = est.t.x; T[10] = est.t.y; T[11] = est.t.z;
    for (int k = 0; k < 12; ++k) {
      if (!std::isfinite(T[k])) return set_error(SSLAM_ERR_INVALID, "%s: the estimate of vertex %d is not finite", what, kf.node);
      pose[12 * (size_t)c + k] = (float)T[k];
    }
    if (c < max_clouds) {
      if (vertex_out) vertex_out[c] = kf.node;
      if (poses_out) std::memcpy(poses_out + 12 * (size_t)c, T, sizeof T);
    }
  }
  *in = MapCloudIn{nullptr, nullptr, nullptr, s->map_start.data(), n};
  if ((rc = ensure_stream(s))) return rc;
  SSLAM_HIP_TRY(hipSetDevice(s->P.device));
  if ((rc = s->d_map_pose.reserve(pose.size(), s->stream, 0))) return rc;
  const size_t bytes = pose.size() * sizeof(float);
  std::vector<char> fallback;
  char* stage = s->pin.get(bytes);
  if (!stage) { fallback.resize(bytes); stage = fallback.data(); }
  std::memcpy(stage, pose.data(), bytes);
  SSLAM_HIP_TRY(hipMemcpyAsync(s->d_map_pose.p, stage, bytes, hipMemcpyHostToDevice, s->stream));
  SSLAM_HIP_TRY(hipStreamSynchronize(s->stream));
  in->d_xyz = s->d_map_xyz.p; in->d_start = s->d_map_start.p; in->d_pose = s->d_map_pose.p;
  *sent = s->map_pending_bytes + (int64_t)bytes;
  return 0;
}

int sslam_slam_map_cloud(sslam_slam* s, float resolution, int min_points, float* xyz_out, int32_t* cells_out, int32_t* counts_out, int max_out,
                         int32_t* vertex_out, double* poses_out, int max_clouds, sslam_map_stats* stats) {
  if (!s || max_clouds < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = map_cloud_check_args(resolution, min_points, xyz_out, max_out);
  if (rc) return rc;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (!s->map_on || s->map_kf.empty()) return 0;   // nothing is kept
  if ((rc = map_same_device(s))) return rc;
  MapCloudIn in;
  int64_t sent = 0;
  if ((rc = map_poses_to_device(s, "map cloud", vertex_out, poses_out, max_clouds, &in, &sent))) return rc;
  rc = seg_map_cloud_device(s->seg, in, resolution, min_points, xyz_out, cells_out, counts_out, max_out, stats);
  if (rc >= 0) s->map_pending_bytes = 0;
  if (stats) stats->upload_bytes = sent;
  return rc;
}

// sslam_slam_occupancy_map and sslam_slam_occupancy_map_scans: the kept clouds at the current estimates through one of the two device entries
static int occupancy_map_kept(decltype(&seg_occupancy_map_device) entry, sslam_slam* s, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out,
                              int32_t* misses_out, float* logodds_out, int max_out, sslam_occ_stats* stats) {
  if (!s) return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = occupancy_check_args(p, max_out);
  if (rc) return rc;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (!s->map_on || s->map_kf.empty()) return 0;   // nothing is kept: what sslam_slam_map_cloud returns in that state
  if ((rc = map_same_device(s))) return rc;
  MapCloudIn in;
  int64_t sent = 0;
  if ((rc = map_poses_to_device(s, "occupancy map", nullptr, nullptr, 0, &in, &sent))) return rc;
  rc = entry(s->seg, in, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
  if (rc >= 0) s->map_pending_bytes = 0;
  if (stats) stats->upload_bytes = sent;
  return rc;
}

int sslam_slam_occupancy_map(sslam_slam* s, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out, float* logodds_out,
                             int max_out, sslam_occ_stats* stats) {
  return occupancy_map_kept(seg_occupancy_map_device, s, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
}

int sslam_slam_occupancy_map_scans(sslam_slam* s, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out,
                                   float* logodds_out, int max_out, sslam_occ_stats* stats) {
  return occupancy_map_kept(seg_occupancy_map_scans_device, s, p, cells_out, hits_out, misses_out, logodds_out, max_out, stats);
}

int sslam_slam_loop_candidates(sslam_slam* s, const double* keys, int n_keys, const double* news, int n_new, const sslam_loop_params* p,
                               int32_t* cand_out, int32_t* count_out, int cap) {
  if (!s || !p || n_keys < 0 || n_new < 0 || cap < 0 || (n_keys > 0 && !keys) || (n_new > 0 && (!news || !count_out)) ||
      ((size_t)n_new * cap > 0 && !cand_out))
    return set_error(SSLAM_ERR_INVALID, "bad argument");
  int rc = check_loop_params(p, false);
  if (rc < 0) return rc;
  if ((rc = loop_candidates(s, keys, n_keys, news, n_new, *p, cand_out, count_out, cap)) < 0) return rc;
  return n_new;
}

int sslam_slam_find_matches(sslam_slam* s, const sslam_plane* objects, int n, const float robot_pose[6], sslam_landmark* out) {
  if (!s || n < 0 || (n > 0 && (!objects || !out)) || !robot_pose) return set_error(SSLAM_ERR_INVALID, "null argument");
  std::vector<sslam_landmark> cur;
  const int rc = find_matches(s, objects, n, robot_pose, cur);
  if (rc < 0) return rc;
  for (int j = 0; j < n; ++j) out[j] = cur[j];
  return n;
}

}  // extern "C"
