// Drop-in C++ shim: ps_graph_slam::InformationMatrixCalculator (reference include/ps_graph_slam/information_matrix_calculator.hpp,
// src/ps_graph_slam/information_matrix_calculator.cpp) with the two methods the reference cut out of hdl_graph_slam's class of the same
// name [UPSTREAM]: calc_fitness_score(cloud1, cloud2, relpose, max_range) -- the call commented out at
// information_matrix_calculator.cpp:37 -- and calc_information_matrix(cloud1, cloud2, relpose), over the MI355X C-ABI
// (sslam_seg_fitness_scores, sslam_information_from_fitness in include/sslam.h).
//
// Header-only; neither Eigen nor PCL is needed.  A cloud is any type with .points[i].x / .y / .z and .points.size() (pcl::PointCloud<T>
// is one) or a plain float* / count pair of packed xyz; relpose is 12 doubles (R row-major, then t) or anything with .linear()(r, c)
// and .translation()(r) (Eigen::Isometry3d is one), taking cloud2 into the frame of cloud1.  The ROS parameters of the constructor
// become public members.  The nearest-neighbour search runs on the GPU (there is no CPU fallback): a failed call throws.
#ifndef PS_GRAPH_SLAM_AMD_INFORMATION_MATRIX_CALCULATOR_HPP
#define PS_GRAPH_SLAM_AMD_INFORMATION_MATRIX_CALCULATOR_HPP

#include <array>
#include <cfloat>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sslam.h"

namespace ps_graph_slam {

class InformationMatrixCalculator {
 public:
  // information_matrix_calculator.cpp:9-17 (~use_const_inf_matrix, ~const_stddev_x, ~const_stddev_q; 0 -> 0.0667) and the members of
  // information_matrix_calculator.hpp:31-36, which the reference never initialises: hdl_graph_slam's defaults
  // [UPSTREAM, unverified here] through sslam_inf_default_params
  bool use_const_inf_matrix = false;
  double const_stddev_x = 0.0667, const_stddev_q = 0.0667;
  sslam_inf_params params;

  InformationMatrixCalculator() { sslam_inf_default_params(&params); }

  // the frontend handle the search runs on: one per process, created on first use with the default parameters (device 0)
  static sslam_seg* handle() {
    static Handle h;
    return h.s;
  }

  // mean squared distance of the points of cloud2, moved by relpose, to their nearest point of cloud1, over the points whose squared
  // distance does not exceed max_range (hdl_graph_slam compares nn_dists[0]); DBL_MAX when no point qualifies
  template <class Pose>
  static double calc_fitness_score(const float* xyz1, int n1, const float* xyz2, int n2, const Pose& relpose, double max_range = DBL_MAX) {
    std::vector<float> xyz;
    xyz.reserve(3 * ((size_t)n1 + (size_t)n2));
    xyz.insert(xyz.end(), xyz1, xyz1 + 3 * (size_t)n1);
    xyz.insert(xyz.end(), xyz2, xyz2 + 3 * (size_t)n2);
    const int32_t start[3] = {0, n1, n1 + n2};
    sslam_fitness_pair P;
    P.target = 0; P.source = 1; P.max_range = max_range;
    pose12(relpose, P.T);
    double score = 0;
    int32_t used = 0;
    if (sslam_seg_fitness_scores(handle(), xyz.data(), start, 2, &P, 1, &score, &used, nullptr, nullptr, nullptr) < 0)
      throw std::runtime_error(std::string("sslam_seg_fitness_scores: ") + sslam_last_error());
    return score;
  }
  template <class Cloud, class Pose>
  static double calc_fitness_score(const Cloud& cloud1, const Cloud& cloud2, const Pose& relpose, double max_range = DBL_MAX) {
    const std::vector<float> a = packed(cloud1), b = packed(cloud2);
    return calc_fitness_score(a.data(), (int)(a.size() / 3), b.data(), (int)(b.size() / 3), relpose, max_range);
  }

  // calc_information_matrix (information_matrix_calculator.cpp:28-51 with the score restored): row-major 6 x 6
  template <class Cloud, class Pose>
  std::array<double, 36> calc_information_matrix(const Cloud& cloud1, const Cloud& cloud2, const Pose& relpose) const {
    if (use_const_inf_matrix) return constant();
    return from_score(calc_fitness_score(cloud1, cloud2, relpose));
  }
  template <class Pose>
  std::array<double, 36> calc_information_matrix(const float* xyz1, int n1, const float* xyz2, int n2, const Pose& relpose) const {
    if (use_const_inf_matrix) return constant();
    return from_score(calc_fitness_score(xyz1, n1, xyz2, n2, relpose));
  }
  // the reference's own signature: the constant matrix (information_matrix_calculator.cpp:28-35)
  std::array<double, 36> calc_information_matrix() const { return constant(); }

  std::array<double, 36> from_score(double fitness_score) const {
    std::array<double, 36> inf;
    if (sslam_information_from_fitness(&params, fitness_score, inf.data()) < 0)
      throw std::runtime_error(std::string("sslam_information_from_fitness: ") + sslam_last_error());
    return inf;
  }

 private:
  friend class ScanMatcher;         // scan_matcher.hpp: the same cloud and pose types, the same handle
  friend class MapCloudGenerator;   // map_cloud_generator.hpp: likewise
  friend class OccupancyMapGenerator;   // occupancy_map_generator.hpp: likewise
  struct Handle {
    sslam_seg* s;
    Handle() : s(sslam_seg_create(nullptr)) {}
    ~Handle() { if (s) sslam_seg_destroy(s); }
  };
  std::array<double, 36> constant() const {
    std::array<double, 36> inf{};
    const double sx = const_stddev_x == 0 ? 0.0667 : const_stddev_x, sq = const_stddev_q == 0 ? 0.0667 : const_stddev_q;
    for (int k = 0; k < 3; ++k) { inf[k * 7] = 1.0 / sx; inf[(k + 3) * 7] = 1.0 / sq; }
    return inf;
  }
  template <class Cloud>
  static std::vector<float> packed(const Cloud& c) {
    std::vector<float> v;
    v.reserve(3 * c.points.size());
    for (const auto& p : c.points) { v.push_back(p.x); v.push_back(p.y); v.push_back(p.z); }
    return v;
  }
  static void pose12(const double* T, double out[12]) { for (int k = 0; k < 12; ++k) out[k] = T[k]; }
  template <class Pose>
  static auto pose12(const Pose& T, double out[12]) -> decltype(T.linear(), void()) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) out[r * 3 + c] = T.linear()(r, c);
      out[9 + r] = T.translation()(r);
    }
  }
};

}  // namespace ps_graph_slam

#endif
