// Compile-and-link check of GraphSLAM::add_robust_kernel (hdl_graph_slam's signature) on every edge handle type, and its host logic:
// g2o's factory names reach the C-ABI as SSLAM_ROBUST_*, an unknown name and a bad width throw, "NONE" removes the kernel.
#include <cstdio>
#include <stdexcept>
#include "../include/ps_graph_slam_amd/graph_slam.hpp"

int main() {
  ps_graph_slam::GraphSLAM slam(false);
  sslam::Isometry T = sslam::Isometry::Identity();
  sslam::VertexSE3* a = slam.add_se3_node(T);
  T.t[0] = 1.0;
  sslam::VertexSE3* b = slam.add_se3_node(T);
  sslam::VertexPointXYZ* p = slam.add_point_xyz_node({1.0, 1.0, 0.5});
  sslam::VertexPointXYZ* q = slam.add_point_xyz_node({2.0, 1.0, 0.5});
  sslam::VertexPlane* pl = slam.add_plane_node({0.0, 0.0, 1.0, -1.0});
  double W6[36] = {0}, W3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, W2[4] = {1, 0, 0, 1};
  for (int k = 0; k < 6; ++k) W6[k * 7] = 1.0;
  sslam::Isometry rel = sslam::Isometry::Identity();
  rel.t[0] = 1.0;
  const sslam::EdgeHandle e0 = slam.add_se3_edge(a, b, rel, W6);
  const sslam::EdgeHandle e1 = slam.add_se3_point_xyz_edge(b, p, {0.0, 1.0, 0.5}, W3);
  const sslam::EdgeHandle e2 = slam.add_se3_plane_edge(b, pl, {0.0, 0.0, 1.0, -1.0}, W3);
  const sslam::EdgeHandle e3 = slam.add_point_xyz_point_xyz_edge(p, q, {1.0, 0.0, 0.0}, W3);
  sslam::EdgeSE3PriorXY* e4 = slam.add_se3_prior_xy_edge(b, {1.0, 0.0}, W2);
  sslam::EdgeSE3PriorXYZ* e5 = slam.add_se3_prior_xyz_edge(b, {1.0, 0.0, 0.0}, W3);
  slam.add_robust_kernel(e0, "Huber", 1.0);
  slam.add_robust_kernel(e1, "Cauchy", 2.0);
  slam.add_robust_kernel(e2, "DCS", 3.0);
  slam.add_robust_kernel(e3, "Welsch", 4.0);
  slam.add_robust_kernel(e4, "Fair", 5.0);
  slam.add_robust_kernel(e5, "Saturated", 6.0);
  const int want[6] = {SSLAM_ROBUST_HUBER, SSLAM_ROBUST_CAUCHY, SSLAM_ROBUST_DCS, SSLAM_ROBUST_WELSCH, SSLAM_ROBUST_FAIR, SSLAM_ROBUST_SATURATED};
  const int ids[6] = {e0.id, e1.id, e2.id, e3.id, e4->id, e5->id};
  for (int k = 0; k < 6; ++k) {
    int kind = -1; double d = -1;
    if (sslam_graph_get_edge_robust_kernel(slam.graph.get(), ids[k], &kind, &d) != 0 || kind != want[k] || d != 1.0 + k) { std::printf("edge %d: kind %d delta %g\n", k, kind, d); return 2; }
  }
  slam.add_robust_kernel(e0, "PseudoHuber", 0.5);
  slam.add_robust_kernel(e0, "NONE", 0.5);
  int kind = -1;
  if (sslam_graph_get_edge_robust_kernel(slam.graph.get(), e0.id, &kind, nullptr) != 0 || kind != SSLAM_ROBUST_NONE) return 3;
  bool threw = false;
  try { slam.add_robust_kernel(e1, "GemanMcClure", 1.0); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { std::printf("unknown kernel name accepted\n"); return 4; }
  threw = false;
  try { slam.add_robust_kernel(e1, "Huber", -1.0); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { std::printf("negative width accepted\n"); return 5; }
  if (sslam_graph_get_edge_robust_kernel(slam.graph.get(), e1.id, &kind, nullptr) != 0 || kind != SSLAM_ROBUST_CAUCHY) return 6;
  std::printf("robust shim ok\n");
  return 0;
}
