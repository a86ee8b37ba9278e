// The C++ shim's ScanMatcher::setMethod (include/ps_graph_slam_amd/scan_matcher.hpp).  `names`: the method names alone, no device needed
// (tests/test_gicp_cpu.py).  With 16 numbers (T[12], fitness, converged, iterations, status) and a GPU: align() with "GICP" on a corner of
// three faces, compared bitwise with those numbers, which tests/test_gicp_gpu.py takes from the Python mirror; "FAST_GICP" gives the same
// bits and "ICP" others.  The clouds are rebuilt there by _shim_clouds(): keep the two in step.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "../include/ps_graph_slam_amd/scan_matcher.hpp"

typedef ps_graph_slam::ScanMatcher::Result Result;

static bool same(const Result& a, const Result& b) {
  for (int q = 0; q < 12; ++q) if (a.relpose[q] != b.relpose[q]) return false;
  return a.fitness == b.fitness && a.converged == b.converged && a.iterations == b.iterations && a.status == b.status;
}

int main(int argc, char** argv) {
  ps_graph_slam::ScanMatcher sm;
  if (sm.isGicp()) { std::printf("the default is not ICP\n"); return 3; }
  const char* names[] = {"GICP", "FAST_GICP", "ICP"};
  for (const char* n : names) {
    sm.setMethod(n);
    if (sm.isGicp() != (std::strcmp(n, "ICP") != 0)) { std::printf("setMethod(%s)\n", n); return 3; }
  }
  const char* refused[] = {"NDT", "NDT_OMP", "gicp", ""};
  for (const char* n : refused) {
    bool threw = false;
    try { sm.setMethod(n); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw || sm.isGicp()) { std::printf("setMethod(\"%s\") was not refused\n", n); return 3; }
  }
  if (argc == 2 && !std::strcmp(argv[1], "names")) { std::printf("shim gicp names ok\n"); return 0; }
  if (sslam_device_count() < 1) { std::printf("shim gicp ok (no GPU: names only)\n"); return 0; }
  if (argc != 17) { std::printf("usage: %s names | T[12] fitness converged iterations status\n", argv[0]); return 2; }
  std::vector<float> tg, sr;
  for (int i = 0; i < 300; ++i) {
    const float u = 0.125f * (float)(i % 10), v = 0.125f * (float)((i / 10) % 10);
    const int face = i / 100;
    const float p[3] = {face == 2 ? 0.0f : u, face == 0 ? v : (face == 1 ? 0.0f : u + 0.125f), face == 0 ? 0.0f : v + 0.125f};
    tg.insert(tg.end(), p, p + 3);
  }
  for (int j = 0; j < 140; ++j) {   // every other target point, seen from a frame shifted by (1/32, -1/64, 1/128)
    const float* p = &tg[3 * (2 * j + 1)];
    sr.push_back(p[0] - 0.03125f); sr.push_back(p[1] + 0.015625f); sr.push_back(p[2] - 0.0078125f);
  }
  const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  sm.max_iterations = 30;
  sm.transformation_epsilon = 1e-9;
  sm.setMethod("GICP");
  const Result r = sm.align(tg.data(), 300, sr.data(), 140, I);
  sm.setMethod("FAST_GICP");
  if (!same(sm.align(tg.data(), 300, sr.data(), 140, I), r)) { std::printf("FAST_GICP differs from GICP\n"); return 3; }
  sm.setMethod("ICP");
  if (same(sm.align(tg.data(), 300, sr.data(), 140, I), r)) { std::printf("ICP gives GICP's bits\n"); return 3; }
  std::printf("shim gicp: T");
  for (double v : r.relpose) std::printf(" %.17g", v);
  std::printf(" fitness %.17g converged %d iterations %d status %d\n", r.fitness, (int)r.converged, r.iterations, r.status);
  for (int q = 0; q < 12; ++q)
    if (r.relpose[q] != std::strtod(argv[1 + q], nullptr)) { std::printf("T[%d] differs from the mirror's %s\n", q, argv[1 + q]); return 4; }
  if (r.fitness != std::strtod(argv[13], nullptr) || (int)r.converged != std::atoi(argv[14]) || r.iterations != std::atoi(argv[15]) ||
      r.status != std::atoi(argv[16])) {
    std::printf("fitness / converged / iterations / status differ from the mirror's %s %s %s %s\n", argv[13], argv[14], argv[15], argv[16]);
    return 4;
  }
  std::printf("shim gicp ok\n");
  return 0;
}
