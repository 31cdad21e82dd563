// launch_camera.hip — ocean_camera_render and ocean_camera_rays (device/k_camera.h): one launch each; the
// render runs a 16 x 16 pixel tile per work item under the plan's CU budget, sampling the maps directly.
#include "device/k_camera.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_camera_rays(const CameraParams& cam, float4* rays, hipStream_t stream)
{
  const int64_t n = (int64_t)cam.width * cam.height;
  const int64_t blocks = (n + kCameraThreads - 1) / kCameraThreads;
  const int grid = blocks > (1 << 20) ? (1 << 20) : (int)blocks;  // the stride loop takes the rest
  hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)grid), dim3(kCameraThreads), 0, stream, cam, rays);
  return hipGetLastError();
}

hipError_t launch_camera_render(const SurfaceParams& p, const RaycastParams& rc, const CameraParams& cam,
                                const ShadingParams& sh, float4* image, float4* aux, uint32_t* image8,
                                hipStream_t stream, int cus)
{
  const int items = ((cam.width + kCameraTile - 1) / kCameraTile) * ((cam.height + kCameraTile - 1) / kCameraTile);
  if (cam.lod_scale > 0.0f)
  {
    const int grid = persistent_grid(k_camera_render<true>, kCameraThreads, 0, items, cus);
    hipLaunchKernelGGL(k_camera_render<true>, dim3((unsigned)grid), dim3(kCameraThreads), 0, stream, p, rc, cam, sh,
                       image, aux, image8);
  }
  else
  {
    const int grid = persistent_grid(k_camera_render<false>, kCameraThreads, 0, items, cus);
    hipLaunchKernelGGL(k_camera_render<false>, dim3((unsigned)grid), dim3(kCameraThreads), 0, stream, p, rc, cam, sh,
                       image, aux, image8);
  }
  return hipGetLastError();
}

}  // namespace oceanfft
