// The C++ shim's loop-closure gate (gate_se3_edge / gate_se3_point_xyz_edge): a drifting pose chain with four point landmarks, built
// through ps_graph_slam::GraphSLAM and optimised, then the distance of one pose-pose and one pose-landmark candidate that are not in the
// graph.  Without a GPU the program checks the host side only; with one it prints the distances that tests/test_gate_gpu.py compares
// with the Python mirror.  The same graph is rebuilt there by _gate_chain(): keep the two in step.
#include <cmath>
#include <cstdio>
#include "../include/ps_graph_slam_amd/graph_slam.hpp"

int main() {
  ps_graph_slam::GraphSLAM slam(false);
  std::vector<sslam::VertexSE3*> nodes;
  std::vector<sslam::VertexPointXYZ*> pts;
  double W[36] = {0};
  for (int k = 0; k < 6; ++k) W[k * 7] = k < 3 ? 150.0 : 1e5;
  const double Wp[9] = {50, 0, 0, 0, 50, 0, 0, 0, 50};
  for (int i = 0; i < 20; ++i) {
    sslam::Isometry T = sslam::Isometry::Identity();
    T.t[0] = 0.55 * i; T.t[1] = 0.02 * i;
    nodes.push_back(slam.add_se3_node(T));
    if (i > 0) { sslam::Isometry rel = sslam::Isometry::Identity(); rel.t[0] = 0.5; slam.add_se3_edge(nodes[i - 1], nodes[i], rel, W); }
  }
  for (int l = 0; l < 4; ++l) {
    pts.push_back(slam.add_point_xyz_node({2.5 * l + 1.0, 1.5, 0.5}));
    for (int i = 5 * l; i < 5 * l + 4; ++i) slam.add_se3_point_xyz_edge(nodes[i], pts[l], {2.5 * l + 1.0 - 0.5 * i, 1.5, 0.5}, Wp);
  }
  sslam::Isometry Z = sslam::Isometry::Identity();
  Z.t[0] = 8.1; Z.t[1] = 0.1;
  try {   // a candidate between a vertex and itself is refused, before any device work
    slam.gate_se3_edge(nodes[3], nodes[3], Z, W);
    std::printf("a candidate from a vertex to itself accepted\n"); return 2;
  } catch (const std::runtime_error&) {}
  if (sslam_device_count() < 1) { std::printf("shim gate ok (no GPU: compile/link/host-logic only)\n"); return 0; }
  if (!slam.optimize()) { std::printf("optimize returned false\n"); return 3; }
  const double d_se3 = slam.gate_se3_edge(nodes[2], nodes[18], Z, W);
  const double d_pt = slam.gate_se3_point_xyz_edge(nodes[17], pts[0], {-7.4, 1.4, 0.6}, Wp);
  const double d_free = slam.gate_se3_edge(nodes[2], nodes[18], Z, nullptr);
  std::printf("shim gate ok: se3 %.17g point %.17g no-info %.17g\n", d_se3, d_pt, d_free);
  if (!(d_se3 > 0) || !(d_pt > 0) || !(d_free > d_se3)) { std::printf("distances out of order\n"); return 4; }
  if (sslam_graph_num_edges(slam.graph.get()) != 19 + 16) { std::printf("the gate changed the graph\n"); return 4; }
  return 0;
}
