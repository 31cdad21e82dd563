// launch_kinematics.hip — the depth layers of a whole-grid generator (device/k_kinematics.h): the packed
// images of every cascade and layer in one launch, in the shape pack_shape (launch_common.h) gives (the
// batched EncodeIFFT that turns them into the layer maps is the caller's,
// ocean_generator_calculate_kinematics), and the sampler ocean_water_kinematics on launch_points' grid.
#include <cstdint>

#include "device/k_kinematics.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_kinematics_pack(int logn, const FrameParams& fp, const KinematicsDepths& kd, int h0_blk,
                                  const float4* h0, float4* out, hipStream_t stream, int cus)
{
  PackShape s;  // k_rates_pack's shapes and block width
  if (pack_shape(logn, h0_blk, fp.cascades, s) != hipSuccess || kd.layers < 1 || kd.layers > kMaxDepthLayers)
    return hipErrorInvalidValue;
  auto launch = [&](auto kernel) {
    const int grid = persistent_grid(kernel, kKinematicsTile, 0, s.items, cus);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kKinematicsTile), 0, stream, fp, kd, logn, s.logb, s.lcw,
                       h0, out, s.items);
  };
  if (s.block)
    launch(k_kinematics_pack<true>);
  else
    launch(k_kinematics_pack<false>);
  return hipGetLastError();
}

hipError_t launch_water_kinematics(const SurfaceParams& p, const WaterLayers& w, const float* xyz, int64_t count,
                                   int iterations, float tolerance, float4* out, hipStream_t stream, int cus)
{
  return launch_points(k_water_kinematics, 256, count, stream, cus, p, w, xyz, count, iterations, tolerance, out);
}

}  // namespace oceanfft
