// C++ shim: ps_graph_slam::ScanMatcher, the scan matcher of hdl_graph_slam's loop detector [UPSTREAM] (LoopDetector::matching aligns two
// downsampled keyframe clouds with pcl::IterativeClosestPoint: setInputTarget, setInputSource, align(guess), getFinalTransformation,
// getFitnessScore, hasConverged) over the MI355X C-ABI (sslam_seg_register_pairs in include/sslam.h).  The reference has none.
//
// Header-only; neither Eigen nor PCL is needed.  Clouds and poses are the types information_matrix_calculator.hpp accepts: a cloud is any
// type with .points[i].x / .y / .z and .points.size() or a plain float* / count pair of packed xyz; a pose is 12 doubles (R row-major,
// then t) or anything with .linear()(r, c) and .translation()(r), taking the source cloud into the frame of the target cloud.  The
// loop runs on the GPU, on the process-wide frontend handle of InformationMatrixCalculator::handle() (there is no CPU fallback): a
// failed call throws.  result.fitness goes to InformationMatrixCalculator::from_score for the information matrix of the loop edge.
#ifndef PS_GRAPH_SLAM_AMD_SCAN_MATCHER_HPP
#define PS_GRAPH_SLAM_AMD_SCAN_MATCHER_HPP

#include <array>
#include <cfloat>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sslam.h"
#include "information_matrix_calculator.hpp"

namespace ps_graph_slam {

class ScanMatcher {
 public:
  // pcl::Registration's setters of the same names: setMaximumIterations, setTransformationEpsilon (here the largest change of an entry
  // of the 3 x 4 transform; 0 = until it repeats bit for bit) and setMaxCorrespondenceDistance -- a DISTANCE, squared before the call
  // as PCL squares it before it compares (DBL_MAX-like values stay "no bound")
  int max_iterations = 64;
  double transformation_epsilon = 0.0;
  double max_correspondence_distance = DBL_MAX;
  // GICP only: neighbours per covariance and the eigenvalue along the normal (fast_gicp's setCorrespondenceRandomness and its PLANE
  // regularisation); the covariances are computed inside the call
  int gicp_k = 20;
  double gicp_plane_epsilon = 1e-3;

  // hdl_graph_slam's registration_method (select_registration_method): "ICP" (the default: pcl::IterativeClosestPoint), "GICP" or
  // "FAST_GICP" (generalized ICP, sslam_seg_register_pairs_gicp).  Any other name -- "NDT", "NDT_OMP", ... have no kernel here -- throws.
  void setMethod(const std::string& name) {
    if (name == "ICP") gicp_ = false;
    else if (name == "GICP" || name == "FAST_GICP") gicp_ = true;
    else throw std::invalid_argument("ScanMatcher::setMethod: unknown registration method \"" + name + "\" (ICP, GICP, FAST_GICP)");
  }
  bool isGicp() const { return gicp_; }

  struct Result {
    std::array<double, 12> relpose;   // R row-major, then t: source -> target frame (getFinalTransformation)
    double fitness;                   // getFitnessScore at relpose, bounded by the same distance
    bool converged;                   // hasConverged
    int iterations;
    int status;                       // 0, or SSLAM_ERR_NUMERIC: fewer than 3 correspondences in some pass
  };

  // one pair of a batch: plain arrays of packed xyz and the initial guess
  struct Pair {
    const float* target; int n_target;
    const float* source; int n_source;
    double guess[12];
  };

  template <class Pose>
  Result align(const float* target, int n_target, const float* source, int n_source, const Pose& guess) const {
    Pair P{target, n_target, source, n_source, {}};
    InformationMatrixCalculator::pose12(guess, P.guess);
    return align(std::vector<Pair>{P})[0];
  }
  template <class Cloud, class Pose>
  Result align(const Cloud& target, const Cloud& source, const Pose& guess) const {
    const std::vector<float> a = InformationMatrixCalculator::packed(target), b = InformationMatrixCalculator::packed(source);
    return align(a.data(), (int)(a.size() / 3), b.data(), (int)(b.size() / 3), guess);
  }
  // all pairs in one call: they share the launches of every iteration
  std::vector<Result> align(const std::vector<Pair>& pairs) const {
    std::vector<float> xyz;
    std::vector<int32_t> start{0};
    std::vector<sslam_reg_pair> rp(pairs.size());
    const double d = max_correspondence_distance;
    for (size_t k = 0; k < pairs.size(); ++k) {
      const Pair& P = pairs[k];
      xyz.insert(xyz.end(), P.target, P.target + 3 * (size_t)P.n_target);
      start.push_back(start.back() + P.n_target);
      xyz.insert(xyz.end(), P.source, P.source + 3 * (size_t)P.n_source);
      start.push_back(start.back() + P.n_source);
      rp[k].target = (int32_t)(2 * k); rp[k].source = (int32_t)(2 * k + 1);
      for (int q = 0; q < 12; ++q) rp[k].T0[q] = P.guess[q];
      rp[k].max_corr2 = d < 1e154 ? d * d : DBL_MAX;
    }
    std::vector<sslam_reg_result> rr(pairs.size());
    const sslam_gicp_params gp{gicp_k, gicp_plane_epsilon};
    const int rc = gicp_ ? sslam_seg_register_pairs_gicp(InformationMatrixCalculator::handle(), xyz.data(), start.data(), (int)(2 * pairs.size()), rp.data(),
                                                         (int)rp.size(), nullptr, &gp, max_iterations, transformation_epsilon, rr.data(), nullptr, nullptr, nullptr)
                         : sslam_seg_register_pairs(InformationMatrixCalculator::handle(), xyz.data(), start.data(), (int)(2 * pairs.size()), rp.data(),
                                                    (int)rp.size(), max_iterations, transformation_epsilon, rr.data(), nullptr, nullptr, nullptr);
    if (rc < 0) throw std::runtime_error(std::string(gicp_ ? "sslam_seg_register_pairs_gicp: " : "sslam_seg_register_pairs: ") + sslam_last_error());
    std::vector<Result> out(pairs.size());
    for (size_t k = 0; k < pairs.size(); ++k) {
      for (int q = 0; q < 12; ++q) out[k].relpose[q] = rr[k].T[q];
      out[k].fitness = rr[k].score; out[k].converged = rr[k].converged != 0; out[k].iterations = rr[k].iterations; out[k].status = rr[k].status;
    }
    return out;
  }

 private:
  bool gicp_ = false;
};

}  // namespace ps_graph_slam

#endif
