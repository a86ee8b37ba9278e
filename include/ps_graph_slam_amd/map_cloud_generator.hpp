// C++ shim: ps_graph_slam::MapCloudGenerator, the map builder of hdl_graph_slam [UPSTREAM] (MapCloudGenerator::generate(keyframes,
// resolution): every keyframe's cloud transformed by its pose, concatenated, octree-downsampled) over the MI355X C-ABI
// (sslam_seg_map_cloud in include/sslam.h).  The reference planned the call (mapping::generateMap, commented out at
// semantic_graph_slam.cpp:36-40) and has none.
//
// Header-only; neither Eigen nor PCL is needed.  Clouds and poses are the types information_matrix_calculator.hpp accepts: a cloud is any
// type with .points[i].x / .y / .z and .points.size() or a plain float* / count pair of packed xyz; a pose is 12 doubles (R row-major,
// then t) or anything with .linear()(r, c) and .translation()(r), taking the cloud into the map frame.  The passes run on the GPU, on the
// process-wide frontend handle of InformationMatrixCalculator::handle() (there is no CPU fallback): a failed call throws.
// DEVIATION from hdl: a voxel's point is the CENTROID of what fell into it, not the voxel's centre; Map::centre() gives the centre.
#ifndef PS_GRAPH_SLAM_AMD_MAP_CLOUD_GENERATOR_HPP
#define PS_GRAPH_SLAM_AMD_MAP_CLOUD_GENERATOR_HPP

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../sslam.h"
#include "information_matrix_calculator.hpp"

namespace ps_graph_slam {

class MapCloudGenerator {
 public:
  int min_points = 1;   // voxels with fewer points are dropped

  struct Map {
    std::vector<float> xyz;        // 3 per voxel: the centroid
    std::vector<int32_t> cells;    // 3 per voxel: the global cell indices
    std::vector<int32_t> counts;   // points per voxel
    float resolution = 0;
    sslam_map_stats stats{};
    size_t size() const { return counts.size(); }
    // hdl's output: the centre of voxel k (octree getOccupiedVoxelCenters)
    std::array<float, 3> centre(size_t k) const {
      return {((float)cells[3 * k] + 0.5f) * resolution, ((float)cells[3 * k + 1] + 0.5f) * resolution, ((float)cells[3 * k + 2] + 0.5f) * resolution};
    }
  };

  // one cloud of a call: packed xyz and its pose
  struct Item {
    const float* xyz; int n;
    double pose[12];
  };

  Map generate(const std::vector<Item>& items, float resolution) const {
    std::vector<float> xyz;
    std::vector<int32_t> start{0};
    std::vector<double> T;
    for (const Item& I : items) {
      xyz.insert(xyz.end(), I.xyz, I.xyz + 3 * (size_t)I.n);
      start.push_back(start.back() + I.n);
      T.insert(T.end(), I.pose, I.pose + 12);
    }
    Map M;
    M.resolution = resolution;
    const int cap = start.back();   // a voxel holds at least one point
    M.xyz.resize(3 * (size_t)cap); M.cells.resize(3 * (size_t)cap); M.counts.resize((size_t)cap);
    const int m = sslam_seg_map_cloud(InformationMatrixCalculator::handle(), xyz.data(), start.data(), (int)items.size(), T.data(), resolution, min_points,
                                      M.xyz.data(), M.cells.data(), M.counts.data(), cap, &M.stats);
    if (m < 0) throw std::runtime_error(std::string("sslam_seg_map_cloud: ") + sslam_last_error());
    M.xyz.resize(3 * (size_t)m); M.cells.resize(3 * (size_t)m); M.counts.resize((size_t)m);
    return M;
  }
  // hdl's signature over plain vectors: clouds[k] at poses[k]
  template <class Cloud, class Pose>
  Map generate(const std::vector<Cloud>& clouds, const std::vector<Pose>& poses, float resolution) const {
    if (clouds.size() != poses.size()) throw std::invalid_argument("MapCloudGenerator::generate: one pose per cloud");
    std::vector<std::vector<float>> packed(clouds.size());
    std::vector<Item> items(clouds.size());
    for (size_t k = 0; k < clouds.size(); ++k) {
      packed[k] = InformationMatrixCalculator::packed(clouds[k]);
      items[k].xyz = packed[k].data(); items[k].n = (int)(packed[k].size() / 3);
      InformationMatrixCalculator::pose12(poses[k], items[k].pose);
    }
    return generate(items, resolution);
  }
};

}  // namespace ps_graph_slam

#endif
