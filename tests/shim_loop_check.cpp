// The C++ shim's loop closing (semantic_graph_slam::set_loop_closure / last_loops / loop_candidates): a replay recorded by
// tests/test_loop_closure_gpu.py -- per sample the stamp, whether the loop runs after it, the odometry and a 48 x 36 organised cloud of
// xyz + padding floats -- goes through the shim with loop closure on, and the first loop edge it adds is printed for the test to compare
// with the Python mirror's.  The loop parameters are those of tests/loop_scene.py's LOOP_KW and the odometry's its ODOM_STDDEV_*: keep
// them in step.  Without a GPU, or without a recording, the program checks the host side only.
#include <cstdio>
#include <vector>
#include "../include/ps_graph_slam_amd/semantic_graph_slam.hpp"

int main(int argc, char** argv) {
  sslam_seg_params sp;
  sslam_seg_default_params(&sp);
  sslam_seg* seg = sslam_seg_create(&sp);
  if (!seg) { std::printf("sslam_seg_create: %s\n", sslam_last_error()); return 2; }
  sslam_loop_params lp;
  sslam_loop_default_params(&lp);
  lp.distance_thresh = 1.0; lp.distance_from_last_edge_thresh = 2.5; lp.epsilon = 1e-4; lp.max_candidates = 3; lp.voxel_leaf = 0.3f;
  lp.fitness_score_thresh = 0.04; lp.robust_kernel = SSLAM_ROBUST_NONE;
  lp.inf = sslam_inf_params{20.0, 0.05, 0.5, 0.02, 0.1, 0.5};
  int rc = 0;
  {
    semantic_graph_slam bare, slam;
    bare.init(false);
    try {   // loop closure without a frontend handle is refused
      bare.set_loop_closure(&lp);
      std::printf("loop closure accepted without a frontend handle\n"); return 2;
    } catch (const std::runtime_error&) {}
    bare.set_loop_closure(nullptr);
    slam.params().const_stddev_x = 0.1; slam.params().const_stddev_q = 0.01;
    slam.init(false, seg);
    sslam_loop_params bad = lp;
    bad.max_candidates = 65;
    try {
      slam.set_loop_closure(&bad);
      std::printf("max_candidates = 65 accepted\n"); return 2;
    } catch (const std::runtime_error&) {}
    slam.set_loop_closure(&lp);
    if (!slam.last_loops().empty()) { std::printf("loop records before any tick\n"); return 2; }
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (sslam_device_count() < 1 || !f) {
      std::printf("shim loop ok (no GPU or no recording: compile/link/host-logic only)\n");
    } else {
      const int W = 48, H = 36;
      std::vector<float> cloud((size_t)W * H * 4);
      int32_t head[3];
      double odom[7];
      bool found = false;
      // LoopDetector::find_candidates on its own: of three old keyframes the first two are within a metre, the third has not travelled enough
      std::vector<int32_t> cand;
      const std::vector<int32_t> count = slam.loop_candidates({0, 0, 0, 0.6, 0, 1, 0, 0, 5}, {0.1, 0, 10}, lp, 3, cand);
      if (count[0] != 2 || cand[0] != 0 || cand[1] != 1 || cand[2] != -1) { std::printf("loop_candidates: %d %d %d %d\n", count[0], cand[0], cand[1], cand[2]); rc = 3; }
      while (!rc && !found && std::fread(head, sizeof head, 1, f) == 1 && std::fread(odom, sizeof odom, 1, f) == 1 &&
             std::fread(cloud.data(), sizeof(float), cloud.size(), f) == cloud.size()) {
        slam.setPointCloudData(reinterpret_cast<const uint8_t*>(cloud.data()), W, H, 16, 16 * W, 0, 4, 8);
        sslam::Isometry T = sslam::tq_to_isometry(odom);
        slam.VIOCallback(head[0], head[1], T);
        if (!head[2]) continue;
        slam.run();
        for (const sslam_loop& L : slam.last_loops()) {
          if (L.outcome != SSLAM_LOOP_ADDED) continue;
          std::printf("shim loop ok: new %d cand %d candidates %d edge %d used %d iterations %d score %.17g T", L.new_vertex, L.cand_vertex, L.n_candidates,
                      L.edge_id, L.used, L.iterations, L.score);
          for (int k = 0; k < 12; ++k) std::printf(" %.17g", L.T[k]);
          std::printf("\n");
          found = true;
          break;
        }
      }
      if (!rc && !found) { std::printf("no loop edge in the recording\n"); rc = 4; }
    }
    if (f) std::fclose(f);
  }
  sslam_seg_destroy(seg);
  return rc;
}
