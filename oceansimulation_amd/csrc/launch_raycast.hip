// launch_raycast.hip — ocean_surface_raycast (device/k_raycast.h): one launch, 256 rays per work item,
// sampling the maps directly (no atlas).
#include "device/k_raycast.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_surface_raycast(const SurfaceParams& p, const RaycastParams& rc, const float4* rays, int64_t n_rays,
                                  float4* out, hipStream_t stream, int cus)
{
  if (n_rays <= 0)
    return hipSuccess;
  const int64_t items = (n_rays + kRaycastThreads - 1) / kRaycastThreads;
  const int capped = items > (1 << 24) ? (1 << 24) : (int)items;  // the item loop takes the rest
  const int grid = persistent_grid(k_surface_raycast, kRaycastThreads, 0, capped, cus);
  hipLaunchKernelGGL(k_surface_raycast, dim3((unsigned)grid), dim3(kRaycastThreads), 0, stream, p, rc, rays, n_rays,
                     out);
  return hipGetLastError();
}

}  // namespace oceanfft
