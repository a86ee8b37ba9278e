// The map cloud over inputs that already sit on the device: the entry sslam_seg_map_cloud stages its arguments for, and the one
// sslam_slam_map_cloud calls with the clouds the tick keeps resident.  Internal: a C++ symbol, not part of the exported C-ABI.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/sslam.h"
#include "sslam_common.hpp"

namespace sslam {
struct MapCloudIn {
  const float* d_xyz;          // device: the clouds one after the other, 3 floats per point
  const int32_t* d_start;      // device: n_clouds + 1 entries, as cloud_start of sslam_seg_map_cloud
  const float* d_pose;         // device: 12 floats per cloud (R row-major, then t), already cast from double
  const int32_t* h_start;      // host copy of d_start: sizes the launches
  int n_clouds;
};
// the argument rules of sslam_seg_map_cloud that need neither the clouds nor the device
inline int map_cloud_check_args(float resolution, int min_points, const float* xyz_out, int max_out) {
  if (max_out < 0 || min_points < 0 || (!xyz_out && max_out > 0)) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (!(std::isfinite(resolution) && resolution > 0) || !std::isfinite(1.0f / resolution))
    return set_error(SSLAM_ERR_INVALID, "map cloud: resolution %g must be finite and positive, with a finite 1 / resolution", (double)resolution);
  return 0;
}
// The device the frontend handle allocates and launches on.  seg_map_cloud_device dereferences its inputs there, so a caller that owns
// them (the orchestrator's resident map clouds) must have allocated them on the same device.
int seg_device_index(const sslam_seg* s);
// Checks resolution, min_points, max_out / xyz_out and the handle's state as sslam_seg_map_cloud states them, runs the passes on the
// frontend handle's stream and waits for them.  Fills *stats except upload_bytes, which it sets to 0: it moves nothing to the device.
// The inputs must be complete on the device (their copies waited for) before the call.
int seg_map_cloud_device(sslam_seg* s, const MapCloudIn& in, float resolution, int min_points, float* xyz_out, int32_t* cells_out, int32_t* counts_out,
                         int max_out, sslam_map_stats* stats);
}  // namespace sslam
