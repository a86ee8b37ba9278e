// Drop-in C++ shim: the reference's orchestrator class, semantic_graph_slam (reference include/ps_graph_slam/semantic_graph_slam.h,
// src/ps_graph_slam/semantic_graph_slam.cpp), over the MI355X C-ABI (sslam_slam_* in include/sslam.h).
//
// Same method names and call pattern as the reference: the ROS node's callbacks call setPointCloudData / setDetectedObjectInfo /
// VIOCallback, its loop calls run(), the publishers read getRobotPose / getMap2OdomTrans / getMappedLandmarks / getKeyframes.
// ROS, Eigen, g2o and PCL types are replaced by plain ones: stamps are (sec, nsec), poses sslam::Isometry (graph_slam.hpp of this
// directory), the cloud is the PointCloud2 byte buffer with its layout, boxes are sslam_box, landmarks sslam_landmark.  The ROS
// private parameters read in semantic_graph_slam::init, KeyframeUpdater, InformationMatrixCalculator and data_association::init
// become the fields of sslam_slam_params (set them from ros::param in the node).
#ifndef PS_GRAPH_SLAM_AMD_SEMANTIC_GRAPH_SLAM_HPP
#define PS_GRAPH_SLAM_AMD_SEMANTIC_GRAPH_SLAM_HPP

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../sslam.h"
#include "graph_slam.hpp"
#include "occupancy_map_generator.hpp"

class semantic_graph_slam {
 public:
  semantic_graph_slam() { sslam_slam_default_params(&params_); }
  ~semantic_graph_slam() { if (h_) sslam_slam_destroy(h_); }
  semantic_graph_slam(const semantic_graph_slam&) = delete;
  semantic_graph_slam& operator=(const semantic_graph_slam&) = delete;

  // the ROS parameters (semantic_graph_slam.cpp:22-29, keyframe_updater.hpp:24-29, information_matrix_calculator.cpp:9-17,
  // data_association.h:49-55); change them before init()
  sslam_slam_params& params() { return params_; }

  // semantic_graph_slam::init (semantic_graph_slam.cpp:11-56).  seg: the frontend handle segmentallPointCloudData runs on
  // (point_cloud_segmentation of planar_segmentation_amd owns one); nullptr when objects arrive pre-segmented.
  void init(bool verbose, sslam_seg* seg = nullptr) {
    verbose_ = verbose;
    if (h_) sslam_slam_destroy(h_);
    h_ = sslam_slam_create(&params_, seg);
    if (!h_) throw std::runtime_error(std::string("sslam_slam_create: ") + sslam_last_error());
  }

  // semantic_graph_slam::run (semantic_graph_slam.cpp:58-102)
  bool run() {
    const int rc = sslam_slam_run(h_, &last_);
    if (rc < 0) throw std::runtime_error(std::string("sslam_slam_run: ") + sslam_last_error());
    return rc > 0;
  }
  const sslam_tick_stats& lastTick() const { return last_; }

  // VIOCallback (semantic_graph_slam.cpp:234-287); returns whether the sample became a keyframe
  bool VIOCallback(int32_t stamp_sec, int32_t stamp_nsec, const sslam::Isometry& odom) {
    double tq[7];
    sslam::isometry_to_tq(odom, tq);
    return check(sslam_slam_vio(h_, stamp_sec, stamp_nsec, tq), "sslam_slam_vio") > 0;
  }
  // setPointCloudData (semantic_graph_slam.cpp:341-345): sensor_msgs::PointCloud2::data + its layout
  void setPointCloudData(const uint8_t* data, int width, int height, int point_step, int row_step, int off_x, int off_y, int off_z) {
    check(sslam_slam_set_point_cloud(h_, data, width, height, point_step, row_step, off_x, off_y, off_z), "sslam_slam_set_point_cloud");
  }
  // setDetectedObjectInfo (semantic_graph_slam.cpp:353-357)
  void setDetectedObjectInfo(const std::vector<sslam_box>& object_info) {
    check(sslam_slam_set_detected_objects(h_, object_info.data(), (int)object_info.size()), "sslam_slam_set_detected_objects");
  }
  // extension: objects segmented elsewhere, for the next keyframe
  void setSegmentedObjects(const std::vector<sslam_plane>& objects) {
    check(sslam_slam_set_segmented_objects(h_, objects.data(), (int)objects.size()), "sslam_slam_set_segmented_objects");
  }

  // loop closing inside the tick (hdl_graph_slam's LoopDetector::detect; sslam_slam_set_loop_closure): nullptr turns it off.  After
  // init(), which needs the frontend handle for it.
  void set_loop_closure(const sslam_loop_params* params) { check(sslam_slam_set_loop_closure(h_, params), "sslam_slam_set_loop_closure"); }
  // the scan matcher of the loop stage (hdl_graph_slam's registration_method; sslam_slam_set_loop_registration): SSLAM_REG_ICP, the
  // default, or SSLAM_REG_GICP with its parameters (nullptr: k 20, plane_epsilon 1e-3)
  void set_loop_registration(int method, const sslam_gicp_params* params = nullptr) {
    check(sslam_slam_set_loop_registration(h_, method, params), "sslam_slam_set_loop_registration");
  }
  // the records of the last run(): one per new keyframe that reached the selection with at least one candidate
  std::vector<sslam_loop> last_loops() const {
    const int n = check(sslam_slam_last_loops(h_, nullptr, 0), "sslam_slam_last_loops");
    std::vector<sslam_loop> out(n);
    if (n) check(sslam_slam_last_loops(h_, out.data(), n), "sslam_slam_last_loops");
    return out;
  }
  // LoopDetector::find_candidates on its own: keys / news hold x, y, accum_distance per old / new keyframe; returns the counts, cand gets
  // news.size() / 3 rows of `cap` indices (-1 where not filled)
  std::vector<int32_t> loop_candidates(const std::vector<double>& keys, const std::vector<double>& news, const sslam_loop_params& params, int cap,
                                       std::vector<int32_t>& cand) {
    const int n_keys = (int)(keys.size() / 3), n_new = (int)(news.size() / 3);
    cand.assign((size_t)n_new * cap, -1);
    std::vector<int32_t> count(n_new);
    check(sslam_slam_loop_candidates(h_, keys.data(), n_keys, news.data(), n_new, &params, cand.data(), count.data(), cap), "sslam_slam_loop_candidates");
    return count;
  }

  // the map of the run (sslam_slam_set_map_clouds / sslam_slam_map_cloud; where the reference has its commented-out mapping thread,
  // semantic_graph_slam.cpp:72-73, 85-86).  set_map_clouds after init(), which needs the frontend handle for it: from then on every
  // keyframe's downsampled cloud stays on the device.  map_cloud puts them at the current estimates: one centroid per occupied voxel.
  void set_map_clouds(bool on = true, float keyframe_leaf = 0.1f) { check(sslam_slam_set_map_clouds(h_, on ? 1 : 0, keyframe_leaf), "sslam_slam_set_map_clouds"); }
  struct MapCloud {
    std::vector<float> xyz;          // 3 per voxel: the centroid
    std::vector<int32_t> cells;      // 3 per voxel: the global cell; its centre is (cell + 0.5) * resolution
    std::vector<int32_t> counts;
    std::vector<int32_t> vertices;   // the keyframes the map was built from
    std::vector<double> poses;       // 12 per keyframe: R row-major, then t
    sslam_map_stats stats{};
  };
  MapCloud map_cloud(float resolution, int min_points = 1) {
    MapCloud M;
    int32_t n_points = 0;
    const int n_clouds = check(sslam_slam_map_clouds_kept(h_, &n_points), "sslam_slam_map_clouds_kept");
    M.xyz.resize(3 * (size_t)n_points); M.cells.resize(3 * (size_t)n_points); M.counts.resize((size_t)n_points);
    M.vertices.resize((size_t)n_clouds); M.poses.resize(12 * (size_t)n_clouds);
    const int m = check(sslam_slam_map_cloud(h_, resolution, min_points, M.xyz.data(), M.cells.data(), M.counts.data(), n_points, M.vertices.data(),
                                             M.poses.data(), n_clouds, &M.stats), "sslam_slam_map_cloud");
    M.xyz.resize(3 * (size_t)m); M.cells.resize(3 * (size_t)m); M.counts.resize((size_t)m);
    return M;
  }

  // the occupancy map of the run (sslam_slam_occupancy_map; where the reference's launch file runs octomap_server): the clouds set_map_clouds
  // keeps, at the current estimates, ray-cast into the sparse grid.  Empty with map clouds off or none kept.
  ps_graph_slam::OccupancyMap occupancy_map(const sslam_occ_params& params) { return occupancy_map(sslam_slam_occupancy_map, "sslam_slam_occupancy_map", params); }
  // the same through OctoMap's per-scan update (sslam_slam_occupancy_map_scans): every keyframe's cloud one scan, in keyframe order
  ps_graph_slam::OccupancyMap occupancy_map_scans(const sslam_occ_params& params) {
    return occupancy_map(sslam_slam_occupancy_map_scans, "sslam_slam_occupancy_map_scans", params);
  }

  // getRobotPose / getMap2OdomTrans (semantic_graph_slam.cpp:375-381)
  void getRobotPose(sslam::Isometry& robot_pose) const {
    double tq[7];
    check(sslam_slam_robot_pose(h_, tq), "sslam_slam_robot_pose");
    robot_pose = sslam::tq_to_isometry(tq);
  }
  void getMap2OdomTrans(sslam::Isometry& map2odom) const {
    double tq[7];
    check(sslam_slam_map2odom(h_, tq), "sslam_slam_map2odom");
    map2odom = sslam::tq_to_isometry(tq);
  }
  // getMappedLandmarks (semantic_graph_slam.cpp:366-368)
  void getMappedLandmarks(std::vector<sslam_landmark>& l_vec) const {
    const int n = check(sslam_slam_landmarks(h_, nullptr, 0), "sslam_slam_landmarks");
    l_vec.resize(n);
    if (n) check(sslam_slam_landmarks(h_, l_vec.data(), n), "sslam_slam_landmarks");
  }
  // getKeyframes (semantic_graph_slam.cpp:370-373): vertex id and optimised pose of every keyframe in the graph
  void getKeyframes(std::vector<std::pair<int, sslam::Isometry>>& keyframes) const {
    const int n = check(sslam_slam_keyframes(h_, nullptr, nullptr, 0), "sslam_slam_keyframes");
    std::vector<int32_t> ids(n);
    std::vector<double> est(7 * (size_t)n);
    if (n) check(sslam_slam_keyframes(h_, ids.data(), est.data(), n), "sslam_slam_keyframes");
    keyframes.clear();
    for (int i = 0; i < n; ++i) keyframes.emplace_back(ids[i], sslam::tq_to_isometry(&est[7 * (size_t)i]));
  }
  // saveGraph (semantic_graph_slam.cpp:391-394)
  void saveGraph(const std::string& save_graph_path) {
    check(sslam_graph_save_g2o(sslam_slam_graph(h_), save_graph_path.c_str()), "sslam_graph_save_g2o");
    std::cout << "saved the graph at " << save_graph_path << std::endl;
  }

 private:
  static int check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + sslam_last_error());
    return rc;
  }
  using OccEntry = int (*)(sslam_slam*, const sslam_occ_params*, int32_t*, int32_t*, int32_t*, float*, int, sslam_occ_stats*);
  ps_graph_slam::OccupancyMap occupancy_map(OccEntry entry, const char* what, const sslam_occ_params& params) {
    ps_graph_slam::OccupancyMap M;
    M.params = params;
    const int cap = check(entry(h_, &params, nullptr, nullptr, nullptr, nullptr, 0, nullptr), what);   // count, then fetch
    M.resize((size_t)cap);
    const int m = check(entry(h_, &params, M.cells.data(), M.hits.data(), M.misses.data(), M.logodds.data(), cap, &M.stats), what);
    M.resize((size_t)(m < cap ? m : cap));
    return M;
  }
  sslam_slam_params params_;
  sslam_slam* h_ = nullptr;
  sslam_tick_stats last_{};
  bool verbose_ = false;
};

#endif
