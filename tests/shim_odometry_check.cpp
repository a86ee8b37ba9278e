// The C++ shim's Prefilter and ScanMatchingOdometry (include/ps_graph_slam_amd/scan_matching_odometry.hpp).  `params`: the mapping of hdl's
// parameter names onto the C structs, the struct sizes and the refused method names, no device needed (tests/test_odometry_cpu.py); without
// a GPU matching() must throw.  With 72 numbers (six poses of 12) and a GPU: six frames of a corner of three faces, each seen from a frame
// shifted by (1/32, -1/64, 1/128) more, pushed through matching() and compared bitwise with those numbers, which tests/test_odometry_gpu.py
// takes from the Python mirror.  The clouds and the parameters are rebuilt there by _shim_frames() / SHIM_KW: keep the two in step.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "../include/ps_graph_slam_amd/scan_matching_odometry.hpp"

static_assert(sizeof(sslam_prefilter_params) == 64, "layout of sslam_prefilter_params");
static_assert(sizeof(sslam_odom_params) == 160, "layout of sslam_odom_params");
static_assert(sizeof(sslam_odom_stats) == 208, "layout of sslam_odom_stats");

struct Point { float x, y, z; };
struct Cloud { std::vector<Point> points; };

static int fail(const char* what) { std::printf("%s\n", what); return 3; }

int main(int argc, char** argv) {
  {   // the members' defaults are the C defaults
    ps_graph_slam::ScanMatchingOdometry od;
    sslam_odom_params d;
    sslam_odom_default_params(&d);
    const sslam_odom_params p = od.params();
    const sslam_prefilter_params &a = p.prefilter, &b = d.prefilter;
    if (a.use_distance_filter != b.use_distance_filter || a.distance_near != b.distance_near || a.distance_far != b.distance_far ||
        a.downsample != b.downsample || a.leaf != b.leaf || a.outlier != b.outlier || a.mean_k != b.mean_k || a.stddev_mul != b.stddev_mul ||
        a.radius != b.radius || a.min_neighbors != b.min_neighbors) return fail("Prefilter's defaults are not sslam_prefilter_default_params'");
    if (p.method != d.method || p.method != SSLAM_REG_GICP || p.gicp.k != d.gicp.k || p.gicp.plane_epsilon != d.gicp.plane_epsilon ||
        p.max_iterations != d.max_iterations || p.epsilon != d.epsilon || p.max_correspondence_distance != d.max_correspondence_distance ||
        p.keyframe_delta_trans != d.keyframe_delta_trans || p.keyframe_delta_angle != d.keyframe_delta_angle ||
        p.keyframe_delta_time != d.keyframe_delta_time || p.transform_thresholding != d.transform_thresholding ||
        p.max_acceptable_trans != d.max_acceptable_trans || p.max_acceptable_angle != d.max_acceptable_angle)
      return fail("ScanMatchingOdometry's defaults are not sslam_odom_default_params'");
    od.registration_method = "ICP";
    if (od.params().method != SSLAM_REG_ICP) return fail("registration_method ICP");
    od.prefilter.outlier_removal_method = "RADIUS"; od.prefilter.downsample_method = "NONE";
    if (od.params().prefilter.outlier != SSLAM_OUTLIER_RADIUS || od.params().prefilter.downsample != SSLAM_DOWNSAMPLE_NONE) return fail("method names");
    const char* refused[] = {"NDT", "NDT_OMP", "gicp", ""};
    for (const char* n : refused) {
      od.registration_method = n;
      bool threw = false;
      try { (void)od.params(); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return fail("an unknown registration_method was not refused");
    }
    od.registration_method = "GICP";
    od.prefilter.downsample_method = "APPROX_VOXELGRID";
    bool threw = false;
    try { (void)od.params(); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) return fail("an unknown downsample_method was not refused");
  }
  if (argc == 2 && !std::strcmp(argv[1], "params")) { std::printf("shim odometry params ok\n"); return 0; }
  ps_graph_slam::ScanMatchingOdometry od;
  od.prefilter.use_distance_filter = false;
  od.prefilter.downsample_method = "NONE";
  od.prefilter.outlier_removal_method = "RADIUS";
  od.prefilter.radius_radius = 0.3; od.prefilter.radius_min_neighbors = 2;
  od.keyframe_delta_trans = 0.05;
  od.reg_transformation_epsilon = 1e-9;
  od.reg_maximum_iterations = 30;
  std::vector<Cloud> frames(6);
  for (int k = 0; k < 6; ++k)
    for (int i = 0; i < 300; ++i) {
      const float u = 0.125f * (float)(i % 10), v = 0.125f * (float)((i / 10) % 10);
      const int face = i / 100;
      const float p[3] = {face == 2 ? 0.0f : u, face == 0 ? v : (face == 1 ? 0.0f : u + 0.125f), face == 0 ? 0.0f : v + 0.125f};
      frames[k].points.push_back(Point{p[0] - 0.03125f * (float)k, p[1] + 0.015625f * (float)k, p[2] - 0.0078125f * (float)k});
    }
  if (sslam_device_count() < 1) {
    bool threw = false;
    try { (void)od.matching(0, 0, frames[0]); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) return fail("matching() without a GPU did not throw");
    std::printf("shim odometry ok (no GPU: params and the refusal only)\n");
    return 0;
  }
  if (argc != 73) { std::printf("usage: %s params | 6 x pose[12]\n", argv[0]); return 2; }
  int keyframes = 0;
  for (int k = 0; k < 6; ++k) {
    const std::array<double, 12> pose = od.matching(k / 10, (k % 10) * 100000000, frames[k]);
    keyframes += od.stats().new_keyframe;
    std::printf("shim odometry: frame %d accepted %d new_keyframe %d pose", k, od.stats().accepted, od.stats().new_keyframe);
    for (double v : pose) std::printf(" %.17g", v);
    std::printf("\n");
    for (int q = 0; q < 12; ++q)
      if (pose[q] != std::strtod(argv[1 + 12 * k + q], nullptr)) { std::printf("frame %d: pose[%d] differs from the mirror's %s\n", k, q, argv[1 + 12 * k + q]); return 4; }
  }
  if (keyframes < 2 || od.stats().keyframes != keyframes) return fail("the six frames took fewer than two keyframes");
  if (od.keyframe().size() % 3 != 0 || od.keyframe().empty()) return fail("keyframe()");
  const std::vector<float> f = od.prefilter.filter(frames[0]);
  if (f.empty() || f.size() > 900) return fail("Prefilter::filter");
  od.reset();
  const std::array<double, 12> first = od.matching(0, 0, frames[3]);
  if (first[0] != 1.0 || first[9] != 0.0 || od.stats().new_keyframe != 1) return fail("matching() after reset() is not a first frame");
  std::printf("shim odometry ok\n");
  return 0;
}
