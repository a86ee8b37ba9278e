// The C++ shim's ScanMatcher (include/ps_graph_slam_amd/scan_matcher.hpp): align() of two small clouds through a cloud type with
// .points[i].x/.y/.z and an Eigen-like pose, through plain arrays, and through the overload that takes several pairs.  Without a GPU the
// program checks that the shim compiles and links; with one it compares the result, bitwise, with the 15 numbers on its command line
// (T[12], fitness, converged, iterations), which tests/test_registration_gpu.py takes from the Python mirror.  The clouds are rebuilt
// there by _shim_clouds(): keep the two in step.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/ps_graph_slam_amd/scan_matcher.hpp"

struct Point { float x, y, z; };
struct Cloud { std::vector<Point> points; };
struct Pose {   // what the shim reads of an Eigen::Isometry3d
  double R[9], t[3];
  struct Lin { const double* R; double operator()(int r, int c) const { return R[r * 3 + c]; } };
  struct Tr { const double* t; double operator()(int r) const { return t[r]; } };
  Lin linear() const { return Lin{R}; }
  Tr translation() const { return Tr{t}; }
};

static bool same(const ps_graph_slam::ScanMatcher::Result& a, const ps_graph_slam::ScanMatcher::Result& b) {
  for (int q = 0; q < 12; ++q) if (a.relpose[q] != b.relpose[q]) return false;
  return a.fitness == b.fitness && a.converged == b.converged && a.iterations == b.iterations && a.status == b.status;
}

int main(int argc, char** argv) {
  Cloud tg, sr;
  for (int i = 0; i < 300; ++i) tg.points.push_back(Point{0.125f * (float)(i % 20), 0.25f * (float)(i / 20), 0.0625f * (float)((i * 7) % 11)});
  for (int j = 0; j < 130; ++j) {   // every other target point, seen from a frame shifted by (1/32, -1/64, 1/128)
    const Point& p = tg.points[2 * j + 3];
    sr.points.push_back(Point{p.x - 0.03125f, p.y + 0.015625f, p.z - 0.0078125f});
  }
  sr.points[17].y = NAN;
  const Pose guess{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  ps_graph_slam::ScanMatcher sm;
  sm.max_iterations = 30;
  sm.max_correspondence_distance = 0.2;
  if (sslam_device_count() < 1) { std::printf("shim registration ok (no GPU: compile/link only)\n"); return 0; }
  if (argc != 16) { std::printf("usage: %s T[12] fitness converged iterations\n", argv[0]); return 2; }
  const ps_graph_slam::ScanMatcher::Result r = sm.align(tg, sr, guess);
  // the plain-array route and the batch overload give the same bits
  std::vector<float> a, b;
  for (const Point& p : tg.points) { a.push_back(p.x); a.push_back(p.y); a.push_back(p.z); }
  for (const Point& p : sr.points) { b.push_back(p.x); b.push_back(p.y); b.push_back(p.z); }
  const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (!same(sm.align(a.data(), 300, b.data(), 130, I), r)) { std::printf("array route differs\n"); return 3; }
  ps_graph_slam::ScanMatcher::Pair P{a.data(), 300, b.data(), 130, {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}};
  ps_graph_slam::ScanMatcher::Pair Q{b.data(), 130, a.data(), 300, {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}};   // the other way round, in the same call
  const std::vector<ps_graph_slam::ScanMatcher::Result> two = sm.align(std::vector<ps_graph_slam::ScanMatcher::Pair>{Q, P});
  if (two.size() != 2 || !same(two[1], r)) { std::printf("batch route differs\n"); return 3; }
  std::printf("shim registration: T");
  for (double v : r.relpose) std::printf(" %.17g", v);
  std::printf(" fitness %.17g converged %d iterations %d status %d\n", r.fitness, (int)r.converged, r.iterations, r.status);
  for (int q = 0; q < 12; ++q)
    if (r.relpose[q] != std::strtod(argv[1 + q], nullptr)) { std::printf("T[%d] differs from the mirror's %s\n", q, argv[1 + q]); return 4; }
  if (r.fitness != std::strtod(argv[13], nullptr) || (int)r.converged != std::atoi(argv[14]) || r.iterations != std::atoi(argv[15])) {
    std::printf("fitness / converged / iterations differ from the mirror's %s %s %s\n", argv[13], argv[14], argv[15]);
    return 4;
  }
  if (r.status != 0 || !r.converged) { std::printf("the loop did not converge\n"); return 5; }
  std::printf("shim registration ok\n");
  return 0;
}
