// C++ shim: ps_graph_slam::Prefilter and ps_graph_slam::ScanMatchingOdometry -- hdl_graph_slam's prefiltering_nodelet (distance filter,
// downsample, outlier removal) and scan_matching_odometry_nodelet (matching(): every frame against the current keyframe cloud) [UPSTREAM,
// quoted from memory] over the MI355X C-ABI (sslam_seg_prefilter, sslam_odom_push in include/sslam.h).  The reference has neither: its
// pose comes from a VIO stack.  matching() returns the pose SemanticGraphSLAM::VIOCallback takes.
//
// Header-only; neither Eigen nor PCL is needed.  Clouds are the types scan_matcher.hpp accepts (.points[i].x / .y / .z, or a float* / count
// pair of packed xyz); a pose comes back as 12 doubles (R row-major, then t): the frame in the frame of the first one.  The public members
// carry hdl's parameter names: filter() reads them at every call, matching() builds its handle from them at its first call and at the
// first one after reset(), so change them before.  The work runs on the
// GPU, on the process-wide frontend handle of InformationMatrixCalculator::handle() (there is no CPU fallback): a failed call throws.
#ifndef PS_GRAPH_SLAM_AMD_SCAN_MATCHING_ODOMETRY_HPP
#define PS_GRAPH_SLAM_AMD_SCAN_MATCHING_ODOMETRY_HPP

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sslam.h"
#include "information_matrix_calculator.hpp"

namespace ps_graph_slam {

namespace odometry_detail {
template <class Cloud>
inline std::vector<float> packed(const Cloud& c) {   // .points[i].x / .y / .z -> packed xyz
  std::vector<float> v;
  v.reserve(3 * c.points.size());
  for (const auto& p : c.points) { v.push_back(p.x); v.push_back(p.y); v.push_back(p.z); }
  return v;
}
}  // namespace odometry_detail

class Prefilter {
 public:
  // prefiltering_nodelet's parameters
  bool use_distance_filter = true;
  double distance_near_thresh = 1.0, distance_far_thresh = 100.0;
  std::string downsample_method = "VOXELGRID";        // VOXELGRID | NONE (APPROX_VOXELGRID has no kernel here)
  double downsample_resolution = 0.1;
  std::string outlier_removal_method = "STATISTICAL"; // STATISTICAL | RADIUS | NONE
  int statistical_mean_k = 20;
  double statistical_stddev = 1.0;
  double radius_radius = 0.8;
  int radius_min_neighbors = 2;

  sslam_prefilter_params params() const {
    sslam_prefilter_params p;
    sslam_prefilter_default_params(&p);
    p.use_distance_filter = use_distance_filter ? 1 : 0;
    p.distance_near = distance_near_thresh; p.distance_far = distance_far_thresh;
    if (downsample_method == "VOXELGRID") p.downsample = SSLAM_DOWNSAMPLE_VOXELGRID;
    else if (downsample_method == "NONE") p.downsample = SSLAM_DOWNSAMPLE_NONE;
    else throw std::invalid_argument("Prefilter: unknown downsample_method \"" + downsample_method + "\" (VOXELGRID, NONE)");
    p.leaf = (float)downsample_resolution;
    if (outlier_removal_method == "STATISTICAL") p.outlier = SSLAM_OUTLIER_STATISTICAL;
    else if (outlier_removal_method == "RADIUS") p.outlier = SSLAM_OUTLIER_RADIUS;
    else if (outlier_removal_method == "NONE") p.outlier = SSLAM_OUTLIER_NONE;
    else throw std::invalid_argument("Prefilter: unknown outlier_removal_method \"" + outlier_removal_method + "\" (STATISTICAL, RADIUS, NONE)");
    p.mean_k = statistical_mean_k; p.stddev_mul = statistical_stddev;
    p.radius = radius_radius; p.min_neighbors = radius_min_neighbors;
    return p;
  }

  // the filtered cloud as packed xyz
  std::vector<float> filter(const float* xyz, int n) const {
    const sslam_prefilter_params p = params();
    std::vector<float> out(3 * (size_t)(n > 0 ? n : 1));
    const int m = sslam_seg_prefilter(InformationMatrixCalculator::handle(), xyz, n, &p, out.data(), n, nullptr, nullptr);
    if (m < 0) throw std::runtime_error(std::string("sslam_seg_prefilter: ") + sslam_last_error());
    out.resize(3 * (size_t)m);
    return out;
  }
  template <class Cloud>
  std::vector<float> filter(const Cloud& cloud) const {
    const std::vector<float> a = odometry_detail::packed(cloud);
    return filter(a.data(), (int)(a.size() / 3));
  }
};

class ScanMatchingOdometry {
 public:
  // scan_matching_odometry_nodelet's parameters
  double keyframe_delta_trans = 0.25, keyframe_delta_angle = 0.15, keyframe_delta_time = 1.0;
  bool transform_thresholding = false;
  double max_acceptable_trans = 1.0, max_acceptable_angle = 1.0;
  // select_registration_method's: "GICP" / "FAST_GICP" (the default there) or "ICP"; pcl::Registration's setters by their parameter names
  std::string registration_method = "FAST_GICP";
  int reg_maximum_iterations = 64;
  double reg_transformation_epsilon = 0.01;
  double reg_max_correspondence_distance = 2.5;
  int reg_correspondence_randomness = 20;        // neighbours per covariance
  double gicp_plane_epsilon = 1e-3;
  Prefilter prefilter;                           // the prefiltering_nodelet in front of it

  ScanMatchingOdometry() = default;
  ScanMatchingOdometry(const ScanMatchingOdometry&) = delete;
  ScanMatchingOdometry& operator=(const ScanMatchingOdometry&) = delete;
  ~ScanMatchingOdometry() { if (h_) sslam_odom_destroy(h_); }

  sslam_odom_params params() const {
    sslam_odom_params p;
    sslam_odom_default_params(&p);
    p.prefilter = prefilter.params();
    if (registration_method == "ICP") p.method = SSLAM_REG_ICP;
    else if (registration_method == "GICP" || registration_method == "FAST_GICP") p.method = SSLAM_REG_GICP;
    else throw std::invalid_argument("ScanMatchingOdometry: unknown registration_method \"" + registration_method + "\" (ICP, GICP, FAST_GICP)");
    p.gicp.k = reg_correspondence_randomness; p.gicp.plane_epsilon = gicp_plane_epsilon;
    p.max_iterations = reg_maximum_iterations; p.epsilon = reg_transformation_epsilon;
    p.max_correspondence_distance = reg_max_correspondence_distance;
    p.keyframe_delta_trans = keyframe_delta_trans; p.keyframe_delta_angle = keyframe_delta_angle; p.keyframe_delta_time = keyframe_delta_time;
    p.transform_thresholding = transform_thresholding ? 1 : 0;
    p.max_acceptable_trans = max_acceptable_trans; p.max_acceptable_angle = max_acceptable_angle;
    return p;
  }

  // matching(stamp, cloud): the pose of the frame in the frame of the first one.  stamp: seconds and nanoseconds, as ros::Time has them.
  std::array<double, 12> matching(int32_t stamp_sec, int32_t stamp_nsec, const float* xyz, int n) {
    if (!h_) {
      const sslam_odom_params p = params();
      h_ = sslam_odom_create(InformationMatrixCalculator::handle(), &p);
      if (!h_) throw std::runtime_error(std::string("sslam_odom_create: ") + sslam_last_error());
    }
    std::array<double, 12> pose;
    const float none[3] = {0, 0, 0};
    if (sslam_odom_push(h_, n > 0 ? xyz : none, n, stamp_sec, stamp_nsec, pose.data(), &last_) < 0)
      throw std::runtime_error(std::string("sslam_odom_push: ") + sslam_last_error());
    return pose;
  }
  template <class Cloud>
  std::array<double, 12> matching(int32_t stamp_sec, int32_t stamp_nsec, const Cloud& cloud) {
    const std::vector<float> a = odometry_detail::packed(cloud);
    return matching(stamp_sec, stamp_nsec, a.data(), (int)(a.size() / 3));
  }
  // forgets the keyframe AND the handle: the next matching() reads the members again
  void reset() { if (h_) { sslam_odom_destroy(h_); h_ = nullptr; } }
  // what the last matching() did: accepted, new_keyframe, the keyframe -> frame transform, fitness, times
  const sslam_odom_stats& stats() const { return last_; }
  // the current keyframe's filtered cloud as packed xyz (empty before the first frame)
  std::vector<float> keyframe() const {
    if (!h_) return {};
    const int m = sslam_odom_keyframe(h_, nullptr, 0, nullptr);
    if (m < 0) throw std::runtime_error(std::string("sslam_odom_keyframe: ") + sslam_last_error());
    std::vector<float> out(3 * (size_t)m);
    if (m > 0 && sslam_odom_keyframe(h_, out.data(), m, nullptr) < 0) throw std::runtime_error(std::string("sslam_odom_keyframe: ") + sslam_last_error());
    return out;
  }

 private:
  sslam_odom* h_ = nullptr;
  sslam_odom_stats last_{};
};

}  // namespace ps_graph_slam

#endif
