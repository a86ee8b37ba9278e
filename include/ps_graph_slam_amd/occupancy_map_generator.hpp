// C++ shim: ps_graph_slam::OccupancyMapGenerator, the occupancy map the reference gets from octomap_server in its launch file (resolution
// 0.05, sensor_model/max_range 10, pointcloud_min_z -1, pointcloud_max_z 5) [UPSTREAM], over the MI355X C-ABI (sslam_seg_occupancy_map in
// include/sslam.h): every keyframe's cloud at its pose, every point the end of a ray from the sensor, hits and misses per cell.
//
// Header-only; neither Eigen nor PCL nor OctoMap is needed.  Clouds and poses are the types map_cloud_generator.hpp accepts.  The passes
// run on the GPU, on the process-wide frontend handle of InformationMatrixCalculator::handle() (there is no CPU fallback): a failed call
// throws.  DEVIATIONS from OctoMap (stated at sslam_seg_occupancy_map): per-ray integration, one clamp on the sum, a flat list of cells;
// generate_scans (sslam_seg_occupancy_map_scans) is OctoMap's per-scan update and keeps only the last of the three.
#ifndef PS_GRAPH_SLAM_AMD_OCCUPANCY_MAP_GENERATOR_HPP
#define PS_GRAPH_SLAM_AMD_OCCUPANCY_MAP_GENERATOR_HPP

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sslam.h"
#include "information_matrix_calculator.hpp"

namespace ps_graph_slam {

// the product of a call, also of semantic_graph_slam::occupancy_map
struct OccupancyMap {
  std::vector<int32_t> cells;     // 3 per record: the global cell indices
  std::vector<int32_t> hits, misses;
  std::vector<float> logodds;     // clamped
  sslam_occ_params params{};
  sslam_occ_stats stats{};
  size_t size() const { return hits.size(); }
  std::array<float, 3> cell_center(size_t k) const {
    const float r = params.resolution;
    return {((float)cells[3 * k] + 0.5f) * r, ((float)cells[3 * k + 1] + 0.5f) * r, ((float)cells[3 * k + 2] + 0.5f) * r};
  }
  bool is_occupied(size_t k) const { return logodds[k] >= params.l_occ; }
  // sizes the vectors for `cap` records / cuts them to the m that came back
  void resize(size_t m) { cells.resize(3 * m); hits.resize(m); misses.resize(m); logodds.resize(m); }
};

class OccupancyMapGenerator {
 public:
  static sslam_occ_params default_params() { sslam_occ_params p; sslam_occ_default_params(&p); return p; }

  // one cloud of a call: packed xyz and its pose
  struct Item {
    const float* xyz; int n;
    double pose[12];
  };

  OccupancyMap generate(const std::vector<Item>& items, const sslam_occ_params& params) const {
    return generate(sslam_seg_occupancy_map, "sslam_seg_occupancy_map: ", items, params);
  }
  // OctoMap's per-scan update (sslam_seg_occupancy_map_scans): every item is one scan, applied in the order given; a cell is updated once
  // per scan, a hit overriding a miss, and clamped after every update.  Deviations (1) and (2) of the ray entry do not apply.
  OccupancyMap generate_scans(const std::vector<Item>& items, const sslam_occ_params& params) const {
    return generate(sslam_seg_occupancy_map_scans, "sslam_seg_occupancy_map_scans: ", items, params);
  }
  // over plain vectors: clouds[k] at poses[k]
  template <class Cloud, class Pose>
  OccupancyMap generate(const std::vector<Cloud>& clouds, const std::vector<Pose>& poses, const sslam_occ_params& params) const {
    const Packed P(clouds, poses);
    return generate(P.items, params);
  }
  template <class Cloud, class Pose>
  OccupancyMap generate_scans(const std::vector<Cloud>& clouds, const std::vector<Pose>& poses, const sslam_occ_params& params) const {
    const Packed P(clouds, poses);
    return generate_scans(P.items, params);
  }

 private:
  using Entry = int (*)(sslam_seg*, const float*, const int32_t*, int, const double*, const sslam_occ_params*, int32_t*, int32_t*, int32_t*, float*, int,
                        sslam_occ_stats*);
  struct Packed {   // clouds and poses of the caller's types as items
    std::vector<std::vector<float>> packed;
    std::vector<Item> items;
    template <class Cloud, class Pose>
    Packed(const std::vector<Cloud>& clouds, const std::vector<Pose>& poses) : packed(clouds.size()), items(clouds.size()) {
      if (clouds.size() != poses.size()) throw std::invalid_argument("OccupancyMapGenerator::generate: one pose per cloud");
      for (size_t k = 0; k < clouds.size(); ++k) {
        packed[k] = InformationMatrixCalculator::packed(clouds[k]);
        items[k].xyz = packed[k].data(); items[k].n = (int)(packed[k].size() / 3);
        InformationMatrixCalculator::pose12(poses[k], items[k].pose);
      }
    }
  };
  OccupancyMap generate(Entry entry, const char* what, const std::vector<Item>& items, const sslam_occ_params& params) const {
    std::vector<float> xyz;
    std::vector<int32_t> start{0};
    std::vector<double> T;
    for (const Item& I : items) {
      xyz.insert(xyz.end(), I.xyz, I.xyz + 3 * (size_t)I.n);
      start.push_back(start.back() + I.n);
      T.insert(T.end(), I.pose, I.pose + 12);
    }
    OccupancyMap M;
    M.params = params;
    sslam_seg* h = InformationMatrixCalculator::handle();
    // the number of known cells is not bounded by the number of points: count first, then fetch
    const int cap = entry(h, xyz.data(), start.data(), (int)items.size(), T.data(), &params, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    if (cap < 0) throw std::runtime_error(std::string(what) + sslam_last_error());
    M.resize((size_t)cap);
    const int m = entry(h, xyz.data(), start.data(), (int)items.size(), T.data(), &params, M.cells.data(), M.hits.data(), M.misses.data(), M.logodds.data(), cap,
                        &M.stats);
    if (m < 0) throw std::runtime_error(std::string(what) + sslam_last_error());
    M.resize((size_t)(m < cap ? m : cap));
    return M;
  }
};

}  // namespace ps_graph_slam

#endif
