// launch_kinematics.hip — the depth layers of a whole-grid generator (device/k_kinematics.h): the packed
// images of every cascade and layer in one launch (the batched EncodeIFFT that turns them into the layer
// maps is the caller's, ocean_generator_calculate_kinematics), and the sampler ocean_water_kinematics.
#include <cstdint>

#include "device/k_kinematics.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_kinematics_pack(int logn, const FrameParams& fp, const KinematicsDepths& kd, int h0_blk,
                                  const float4* h0, float4* out, hipStream_t stream, int cus)
{
  int logb = 0;
  while ((1 << logb) < h0_blk)
    logb++;
  if (logn < 4 || logn > 14 || h0_blk < 1 || (1 << logb) != h0_blk || logb > logn || fp.cascades < 1 ||
      fp.cascades > kMaxCascades || kd.layers < 1 || kd.layers > kMaxDepthLayers)
    return hipErrorInvalidValue;
  // k_rates_pack's shapes and block width (launch_rates.hip): the block shape for every N >= 64
  int lcw = logb + 2 < 3 ? 3 : (logb + 2 > 6 ? 6 : logb + 2);  // CW = min(max(4 B, 8), 64)
  const bool block = lcw <= logn && 10 - lcw <= logn;
  const int items = fp.cascades << (2 * logn - (block ? 10 : 8));  // <= 64 * 2^20
  if (block)
  {
    const int grid = persistent_grid(k_kinematics_pack<true>, kKinematicsTile, 0, items, cus);
    hipLaunchKernelGGL(k_kinematics_pack<true>, dim3((unsigned)grid), dim3(kKinematicsTile), 0, stream, fp, kd, logn,
                       logb, lcw, h0, out, items);
  }
  else
  {
    const int grid = persistent_grid(k_kinematics_pack<false>, kKinematicsTile, 0, items, cus);
    hipLaunchKernelGGL(k_kinematics_pack<false>, dim3((unsigned)grid), dim3(kKinematicsTile), 0, stream, fp, kd, logn,
                       logb, lcw, h0, out, items);
  }
  return hipGetLastError();
}

// One thread per point on at most cus * 8 workgroups of 256, the item loop takes the rest (launch_points,
// launch_surface.hip)
hipError_t launch_water_kinematics(const SurfaceParams& p, const WaterLayers& w, const float* xyz, int64_t count,
                                   int iterations, float tolerance, float4* out, hipStream_t stream, int cus)
{
  if (count <= 0)
    return hipSuccess;
  long blocks = (long)((count + 255) / 256);
  const long cap = (long)cus * 8;
  if (blocks > cap)
    blocks = cap;
  hipLaunchKernelGGL(k_water_kinematics, dim3((unsigned)blocks), dim3(256), 0, stream, p, w, xyz, count, iterations,
                     tolerance, out);
  return hipGetLastError();
}

}  // namespace oceanfft
