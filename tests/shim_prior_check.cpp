// The C++ shim's prior factories (add_se3_prior_xy_edge / add_se3_prior_xyz_edge: reference graph_slam.hpp:115-126, commented out
// there): a drifting pose chain anchored by position priors, built through ps_graph_slam::GraphSLAM and optimised.  Without a GPU the
// program checks the host side only; with one it prints the chi2 that tests/test_prior_edges_gpu.py compares with the Python mirror.
// The same graph is rebuilt there from prior_chain() in that file: keep the two in step.
#include <cmath>
#include <cstdio>
#include "../include/ps_graph_slam_amd/graph_slam.hpp"

int main() {
  ps_graph_slam::GraphSLAM slam(false);
  std::vector<sslam::VertexSE3*> nodes;
  double W[36] = {0};
  for (int k = 0; k < 6; ++k) W[k * 7] = k < 3 ? 150.0 : 1e5;
  const int n = 20;
  for (int i = 0; i < n; ++i) {
    sslam::Isometry T = sslam::Isometry::Identity();
    T.t[0] = 0.55 * i; T.t[1] = 0.02 * i;                // odometry that drifts: 10 % long, sideways
    nodes.push_back(slam.add_se3_node(T));
    if (i > 0) { sslam::Isometry rel = sslam::Isometry::Identity(); rel.t[0] = 0.5; slam.add_se3_edge(nodes[i - 1], nodes[i], rel, W); }
  }
  const double Wxyz[9] = {4, 0.5, 0, 0.5, 4, 0, 0, 0, 1};
  const double Wxy[4] = {4, -0.25, -0.25, 2};
  std::vector<sslam::EdgeSE3PriorXYZ*> pz;
  std::vector<sslam::EdgeSE3PriorXY*> pxy;
  for (int i = 5; i < n; i += 5) pz.push_back(slam.add_se3_prior_xyz_edge(nodes[i], {0.5 * i, 0.0, 0.0}, Wxyz));
  for (int i = 7; i < n; i += 6) pxy.push_back(slam.add_se3_prior_xy_edge(nodes[i], {0.5 * i, 0.0}, Wxy));
  // edge ids share the binary edges' counter; the handed-out pointers stay valid while more are added
  if (pz.size() != 3 || pxy.size() != 3 || pz[0]->id != n - 1 || pz[2]->id != n + 1 || pxy[0]->id != n + 2 || pxy[2]->id != n + 4) {
    std::printf("prior edge ids wrong\n"); return 2;
  }
  if (sslam_graph_num_edges(slam.graph.get()) != n - 1 + 6) { std::printf("edge count wrong\n"); return 2; }
  try {   // a prior on a vertex that is not a pose is refused
    slam.add_se3_prior_xyz_edge(reinterpret_cast<sslam::VertexSE3*>(slam.add_point_xyz_node({0, 0, 0})), {0, 0, 0}, Wxyz);
    std::printf("prior on a point accepted\n"); return 2;
  } catch (const std::runtime_error&) {}
  if (sslam_device_count() < 1) { std::printf("shim prior ok (no GPU: compile/link/host-logic only)\n"); return 0; }
  if (!slam.optimize()) { std::printf("optimize returned false\n"); return 3; }
  const double x19 = nodes[19]->estimate().t[0];
  std::printf("shim prior ok: chi2 %.17g -> %.17g x19 %.17g\n", slam.last_stats.chi2_before, slam.last_stats.chi2_after, x19);
  if (!(std::fabs(x19 - 9.5) < 0.2)) { std::printf("the priors did not pull the chain back\n"); return 4; }
  return 0;
}
