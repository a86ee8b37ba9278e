// The occupancy map over inputs that already sit on the device: the entries sslam_seg_occupancy_map and sslam_seg_occupancy_map_scans stage
// their arguments for, and the ones sslam_slam_occupancy_map and sslam_slam_occupancy_map_scans call with the clouds the tick keeps resident.
// Internal: C++ symbols, not part of the exported C-ABI.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/sslam.h"
#include "map_cloud.hpp"
#include "sslam_common.hpp"

namespace sslam {
// R of sslam_seg_occupancy_map: max_range in 1/1024 cell; 0 when it is outside 1 .. 2^20
inline long long occupancy_range_units(const sslam_occ_params& p) {
  const double r = std::floor((double)p.max_range * (double)(1.0f / p.resolution) * 1024.0);
  return (r >= 1.0 && r <= 1048576.0) ? (long long)r : 0;
}
// the argument rules of sslam_seg_occupancy_map that need neither the clouds nor the device
inline int occupancy_check_args(const sslam_occ_params* p, int max_out) {
  if (!p || max_out < 0) return set_error(SSLAM_ERR_INVALID, "bad argument");
  if (!(std::isfinite(p->resolution) && p->resolution > 0) || !std::isfinite(1.0f / p->resolution))
    return set_error(SSLAM_ERR_INVALID, "occupancy map: resolution %g must be finite and positive, with a finite 1 / resolution", (double)p->resolution);
  if (!(std::isfinite(p->max_range) && p->max_range > 0))
    return set_error(SSLAM_ERR_INVALID, "occupancy map: max_range %g must be finite and positive", (double)p->max_range);
  if (occupancy_range_units(*p) == 0)
    return set_error(SSLAM_ERR_INVALID, "occupancy map: max_range %g at resolution %g is outside 1 .. 2^20 units of 1/1024 cell (at most 1024 cells)",
                     (double)p->max_range, (double)p->resolution);
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(p->sensor_origin[k])) return set_error(SSLAM_ERR_INVALID, "occupancy map: sensor_origin is not finite");
  if (!(std::isfinite(p->l_hit) && p->l_hit > 0) || !(std::isfinite(p->l_miss) && p->l_miss < 0))
    return set_error(SSLAM_ERR_INVALID, "occupancy map: l_hit %g must be positive and l_miss %g negative", (double)p->l_hit, (double)p->l_miss);
  if (!(p->l_min <= p->l_max) || !(p->z_min <= p->z_max) || std::isnan(p->l_occ))
    return set_error(SSLAM_ERR_INVALID, "occupancy map: l_min <= l_max and z_min <= z_max must hold, and l_occ must be a number");
  if (p->emit < 0 || p->emit > 2) return set_error(SSLAM_ERR_INVALID, "occupancy map: emit %d is not 0, 1 or 2", (int)p->emit);
  return 0;
}
// Checks params, max_out and the handle's state as sslam_seg_occupancy_map states them, runs the passes on the frontend handle's stream and
// waits for them.  Fills *stats except upload_bytes, which it sets to 0: it moves nothing to the device.  The inputs (MapCloudIn, as for
// seg_map_cloud_device) must be complete on the device before the call.
int seg_occupancy_map_device(sslam_seg* s, const MapCloudIn& in, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out, int32_t* misses_out,
                             float* logodds_out, int max_out, sslam_occ_stats* stats);
// The same for sslam_seg_occupancy_map_scans: the same checks and passes 0 and 1 (one copy of their host code), then mark and fold per chunk
// of clouds in place of the accumulate pass.  Per cell of a touched brick: hits, misses and log-odds (12 bytes) and the two 64-bit masks of
// a chunk (16 bytes), 28 bytes; 2^20 touched bricks, the limit, are 2^29 cells or 15 GB of tables, which the device holds (288 GB).
// A table that cannot be allocated fails the call with the runtime's error, as in the ray entry.
int seg_occupancy_map_scans_device(sslam_seg* s, const MapCloudIn& in, const sslam_occ_params* p, int32_t* cells_out, int32_t* hits_out,
                                   int32_t* misses_out, float* logodds_out, int max_out, sslam_occ_stats* stats);
}  // namespace sslam
