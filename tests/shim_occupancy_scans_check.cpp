// The C++ shim's per-scan occupancy map: ps_graph_slam::OccupancyMapGenerator::generate_scans (include/ps_graph_slam_amd/
// occupancy_map_generator.hpp) over the three fixed clouds of tests/shim_occupancy_check.cpp -- through a cloud type with .points[i].x/.y/.z
// and an Eigen-like pose, and through plain arrays -- and semantic_graph_slam::occupancy_map_scans over a replay recorded by
// tests/test_occupancy_scans_gpu.py (the format of tests/shim_map_check.cpp's).  The counts are printed for the test to compare with the
// Python calls; the fixed clouds are rebuilt there by _shim_input(): keep the two in step.
// Without a GPU, or without a recording, the program checks the host side only.
#include <cstdio>
#include <vector>
#include "../include/ps_graph_slam_amd/occupancy_map_generator.hpp"
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
  const sslam_occ_params P = ps_graph_slam::OccupancyMapGenerator::default_params();
  sslam_seg_params sp;
  sslam_seg_default_params(&sp);
  sslam_seg* seg = sslam_seg_create(&sp);
  if (!seg) { std::printf("sslam_seg_create: %s\n", sslam_last_error()); return 2; }
  int rc = 0;
  {
    semantic_graph_slam bare, slam;
    bare.init(false);
    if (bare.occupancy_map_scans(P).size() != 0) { std::printf("an occupancy map without kept clouds\n"); return 2; }
    try {   // a bad parameter is refused on the host
      sslam_occ_params bad = P;
      bad.emit = 3;
      bare.occupancy_map_scans(bad);
      std::printf("emit 3 accepted\n"); return 2;
    } catch (const std::runtime_error&) {}
    try {   // one pose per cloud
      ps_graph_slam::OccupancyMapGenerator().generate_scans(clouds, std::vector<Pose>(poses.begin(), poses.begin() + 2), P);
      std::printf("two poses for three clouds accepted\n"); return 2;
    } catch (const std::invalid_argument&) {}
    slam.init(false, seg);
    slam.set_map_clouds(true, 0.3f);
    if (slam.occupancy_map_scans(P).size() != 0) { std::printf("an occupancy map before any keyframe\n"); return 2; }
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (sslam_device_count() < 1 || !f) {
      std::printf("shim occupancy scans ok (no GPU or no recording: compile/link/host-logic only)\n");
    } else {
      ps_graph_slam::OccupancyMapGenerator gen;
      sslam_occ_params Q = P;
      Q.resolution = 0.125f;
      Q.sensor_origin[2] = 0.5f;
      const ps_graph_slam::OccupancyMap M = gen.generate_scans(clouds, poses, Q);
      // the plain-array route gives the same bits
      std::vector<std::vector<float>> packed(3);
      std::vector<ps_graph_slam::OccupancyMapGenerator::Item> items(3);
      for (int c = 0; c < 3; ++c) {
        for (const Point& p : clouds[c].points) { packed[c].push_back(p.x); packed[c].push_back(p.y); packed[c].push_back(p.z); }
        items[c].xyz = packed[c].data(); items[c].n = (int)clouds[c].points.size();
        for (int k = 0; k < 9; ++k) items[c].pose[k] = poses[c].R[k];
        for (int k = 0; k < 3; ++k) items[c].pose[9 + k] = poses[c].t[k];
      }
      const ps_graph_slam::OccupancyMap A = gen.generate_scans(items, Q);
      if (M.size() == 0 || A.cells != M.cells || A.hits != M.hits || A.misses != M.misses || A.logodds != M.logodds) { std::printf("array route differs\n"); rc = 3; }
      const ps_graph_slam::OccupancyMap rays = gen.generate(items, Q);   // the ray entry: the same cells, never fewer counts
      if (!rc && (rays.cells != M.cells || rays.stats.n_steps <= M.stats.n_steps)) { std::printf("the ray entry's cells differ\n"); rc = 3; }
      if (!rc) {
        long long hits = 0, misses = 0; int occupied = 0; double sum = 0;
        for (size_t k = 0; k < M.size(); ++k) {
          hits += M.hits[k]; misses += M.misses[k]; occupied += M.is_occupied(k) ? 1 : 0; sum += (double)M.logodds[k];
          if (M.hits[k] + M.misses[k] > 3) { std::printf("a cell updated more than once per scan\n"); rc = 3; break; }
        }
        if (hits + misses != M.stats.n_steps || (long long)M.size() != M.stats.n_cells) { std::printf("stats do not add up\n"); rc = 3; }
        std::printf("shim occupancy scans generate: cells %d occupied %d hits %lld misses %lld logodds sum %.17g\n", (int)M.size(), occupied, hits, misses, sum);
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
        sslam_occ_params T = P;
        T.resolution = 0.2f;
        const ps_graph_slam::OccupancyMap O = slam.occupancy_map_scans(T);
        if (O.size() == 0 || O.stats.n_clouds < 1 || (long long)O.size() != O.stats.n_cells) { std::printf("no occupancy map from the replay\n"); rc = 4; }
        else {
          std::printf("shim occupancy scans tick: clouds %d cells %d steps %lld\n", O.stats.n_clouds, (int)O.size(), (long long)O.stats.n_steps);
          const ps_graph_slam::OccupancyMap again = slam.occupancy_map_scans(T);   // only the poses travel the second time
          if (again.stats.upload_bytes != 48 * (int64_t)again.stats.n_clouds || again.hits != O.hits || again.cells != O.cells || again.logodds != O.logodds) {
            std::printf("second call: %lld bytes\n", (long long)again.stats.upload_bytes); rc = 4;
          }
        }
      }
      if (!rc) std::printf("shim occupancy scans ok\n");
    }
    if (f) std::fclose(f);
  }
  sslam_seg_destroy(seg);
  return rc;
}
