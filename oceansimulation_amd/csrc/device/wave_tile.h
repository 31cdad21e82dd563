// device/wave_tile.h — what the one-wave-per-item kernels share (device/k_hulls.h, device/k_hulls_step.h,
// device/k_moorings.h, the folds of device/k_bounds.h): the lane's place in a work item of HullTile's packing,
// and the min / max step of a wave fold. One definition of each.
#pragma once

#include <hip/hip_runtime.h>

#include "device/lane_xchg.h"
#include "ocean_internal.h"

namespace oceanfft
{

// min (MAX false) or max (MAX true) of v and the value of lane (lane ^ STRIDE), in every lane
template <int STRIDE, bool MAX>
__device__ __forceinline__ float bounds_fold_step(float v)
{
  float a, b;
  xor_lane_pair<STRIDE>(v, a, b);
  return MAX ? fmaxf(a, b) : fminf(a, b);
}

// HullTile, HullBody and HullCall: ocean_internal.h (the host builds the tables)

// The lane's body, point and point_out row in a work item: a tile of one body, or (tile.seg > 0) tile.count
// small bodies from tile.body on, one per aligned segment of tile.seg lanes
struct HullLane
{
  int64_t row;
  int body, point;
  bool active, active_segment;  // the lane holds a point; its segment holds a body
};

__device__ __forceinline__ HullLane hull_tile_lane(const HullBody* bodies, const HullTile& tile, int lane)
{
  HullLane l{tile.offset + lane, tile.body, tile.first + lane, lane < tile.count, true};
  if (tile.seg > 0)
  {
    const int j = lane >> (31 - __clz(tile.seg)), i = lane & (tile.seg - 1);
    l.active = false;
    l.active_segment = j < tile.count;
    if (l.active_segment)
    {
      l.body += j;
      const HullBody hb = bodies[l.body];
      l.active = i < hb.count;
      l.point = hb.first + i;
      l.row = hb.offset + i;
    }
  }
  return l;
}

}  // namespace oceanfft
