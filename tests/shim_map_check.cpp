// The C++ shim's map cloud: ps_graph_slam::MapCloudGenerator::generate (include/ps_graph_slam_amd/map_cloud_generator.hpp) over three small
// fixed clouds -- through a cloud type with .points[i].x/.y/.z and an Eigen-like pose, and through plain arrays -- and
// semantic_graph_slam::set_map_clouds / map_cloud over a replay recorded by tests/test_map_cloud_gpu.py (per sample the stamp, whether the
// loop runs after it, the odometry and a 48 x 36 organised cloud of xyz + padding floats).  The voxel counts and first centroids are
// printed for the test to compare with the Python calls; the fixed clouds are rebuilt there by _shim_input(): keep the two in step.
// Without a GPU, or without a recording, the program checks the host side only.
#include <cstdio>
#include <vector>
#include "../include/ps_graph_slam_amd/map_cloud_generator.hpp"
#include "../include/ps_graph_slam_amd/semantic_graph_slam.hpp"

struct Point { float x, y, z; };
struct Cloud { std::vector<Point> points; };
struct Pose {   // what the shim reads of an Eigen::Isometry3d
  double R[9], t[3];
  struct Lin { const double* R; double operator()(int r, int c) const { return R[r * 3 + c]; } };
  struct Tr { const double* t; double operator()(int r) const { return t[r]; } };
  Lin linear() const { return Lin{R}; }
  Tr translation() const { return Tr{t}; }
};

int main(int argc, char** argv) {
  std::vector<Cloud> clouds(3);
  const std::vector<Pose> poses{Pose{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0.125}}, Pose{{0, -1, 0, 1, 0, 0, 0, 0, 1}, {0.25, -0.5, 0.125}},
                                Pose{{1, 0, 0, 0, 0, -1, 0, 1, 0}, {0.5, -1.0, 0.125}}};
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 200 + 50 * c; ++i)
      clouds[c].points.push_back(Point{0.125f * (float)(i % 16) - 1.0f, 0.0625f * (float)(i / 16) + 0.5f * (float)c, 0.03125f * (float)((i * 7) % 13)});
  sslam_seg_params sp;
  sslam_seg_default_params(&sp);
  sslam_seg* seg = sslam_seg_create(&sp);
  if (!seg) { std::printf("sslam_seg_create: %s\n", sslam_last_error()); return 2; }
  int rc = 0;
  {
    semantic_graph_slam bare, slam;
    bare.init(false);
    try {   // map clouds without a frontend handle are refused
      bare.set_map_clouds(true);
      std::printf("map clouds accepted without a frontend handle\n"); return 2;
    } catch (const std::runtime_error&) {}
    bare.set_map_clouds(false);
    slam.init(false, seg);
    try {
      slam.set_map_clouds(true, -1.0f);
      std::printf("a negative leaf accepted\n"); return 2;
    } catch (const std::runtime_error&) {}
    slam.set_map_clouds(true, 0.3f);
    if (slam.map_cloud(0.2f).counts.size() != 0) { std::printf("a map before any keyframe\n"); return 2; }
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (sslam_device_count() < 1 || !f) {
      std::printf("shim map ok (no GPU or no recording: compile/link/host-logic only)\n");
    } else {
      ps_graph_slam::MapCloudGenerator gen;
      const ps_graph_slam::MapCloudGenerator::Map M = gen.generate(clouds, poses, 0.25f);
      // the plain-array route gives the same bits
      std::vector<std::vector<float>> packed(3);
      std::vector<ps_graph_slam::MapCloudGenerator::Item> items(3);
      for (int c = 0; c < 3; ++c) {
        for (const Point& p : clouds[c].points) { packed[c].push_back(p.x); packed[c].push_back(p.y); packed[c].push_back(p.z); }
        items[c].xyz = packed[c].data(); items[c].n = (int)clouds[c].points.size();
        for (int k = 0; k < 9; ++k) items[c].pose[k] = poses[c].R[k];
        for (int k = 0; k < 3; ++k) items[c].pose[9 + k] = poses[c].t[k];
      }
      const ps_graph_slam::MapCloudGenerator::Map A = gen.generate(items, 0.25f);
      if (M.size() == 0 || A.xyz != M.xyz || A.cells != M.cells || A.counts != M.counts) { std::printf("array route differs\n"); rc = 3; }
      if (!rc) {
        const std::array<float, 3> c0 = M.centre(0);
        for (int a = 0; a < 3; ++a)
          if (!(M.xyz[a] >= c0[a] - 0.125f && M.xyz[a] <= c0[a] + 0.125f)) { std::printf("centroid 0 outside its voxel\n"); rc = 3; }
        std::printf("shim map generate: voxels %d first %.9g %.9g %.9g count %d\n", (int)M.size(), M.xyz[0], M.xyz[1], M.xyz[2], M.counts[0]);
      }
      const int W = 48, H = 36;
      std::vector<float> cloud((size_t)W * H * 4);
      int32_t head[3];
      double odom[7];
      while (!rc && std::fread(head, sizeof head, 1, f) == 1 && std::fread(odom, sizeof odom, 1, f) == 1 &&
             std::fread(cloud.data(), sizeof(float), cloud.size(), f) == cloud.size()) {
        slam.setPointCloudData(reinterpret_cast<const uint8_t*>(cloud.data()), W, H, 16, 16 * W, 0, 4, 8);
        slam.VIOCallback(head[0], head[1], sslam::tq_to_isometry(odom));
        if (head[2]) slam.run();
      }
      if (!rc) {
        const semantic_graph_slam::MapCloud T = slam.map_cloud(0.2f);
        if (T.counts.empty() || T.vertices.size() * 12 != T.poses.size() || (int)T.vertices.size() != T.stats.n_clouds) { std::printf("no map from the replay\n"); rc = 4; }
        else {
          std::printf("shim map tick: clouds %d voxels %d first %.9g %.9g %.9g\n", (int)T.vertices.size(), (int)T.counts.size(), T.xyz[0], T.xyz[1], T.xyz[2]);
          const semantic_graph_slam::MapCloud again = slam.map_cloud(0.2f);   // only the poses travel the second time
          if (again.stats.upload_bytes != 48 * (int64_t)again.vertices.size() || again.xyz != T.xyz) { std::printf("second call: %lld bytes\n", (long long)again.stats.upload_bytes); rc = 4; }
        }
      }
      if (!rc) std::printf("shim map ok\n");
    }
    if (f) std::fclose(f);
  }
  sslam_seg_destroy(seg);
  return rc;
}
