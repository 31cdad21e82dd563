// launch_camera.hip — ocean_camera_render and ocean_camera_rays (device/k_camera.h): one launch each; the
// render runs a 16 x 16 pixel tile per work item under the plan's CU budget, sampling the maps directly.
// ocean_camera_render_layers: the same water pass with the foam stage (k_camera_render<LOD, true>), then with
// records the splat and the composite (device/k_camera_spray.h): at most three launches. Both water passes
// are launch_render; the per-record and per-pixel kernels run on launch_points' grid (launch_common.h).
#include "device/k_camera.h"
#include "device/k_camera_spray.h"
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

// k_camera_render<LOD, FOAM> on a 16 x 16 pixel tile per work item; `last` are the kernel's last two arguments
template <bool FOAM, typename... Last>
static hipError_t launch_render(const SurfaceParams& p, const RaycastParams& rc, const CameraParams& cam,
                                const ShadingParams& sh, float4* image, float4* aux, uint32_t* image8,
                                hipStream_t stream, int cus, const Last&... last)
{
  const int items = ((cam.width + kCameraTile - 1) / kCameraTile) * ((cam.height + kCameraTile - 1) / kCameraTile);
  auto launch = [&](auto kernel) {
    const int grid = persistent_grid(kernel, kCameraThreads, 0, items, cus);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kCameraThreads), 0, stream, p, rc, cam, sh, image, aux,
                       image8, last...);
  };
  if (cam.lod_scale > 0.0f)
    launch(k_camera_render<true, FOAM>);
  else
    launch(k_camera_render<false, FOAM>);
  return hipGetLastError();
}

hipError_t launch_camera_render(const SurfaceParams& p, const RaycastParams& rc, const CameraParams& cam,
                                const ShadingParams& sh, float4* image, float4* aux, uint32_t* image8,
                                hipStream_t stream, int cus)
{
  return launch_render<false>(p, rc, cam, sh, image, aux, image8, stream, cus, CameraNoArg{}, CameraNoArg{});
}

hipError_t launch_camera_render_foam(const SurfaceParams& p, const RaycastParams& rc, const CameraParams& cam,
                                     const ShadingParams& sh, const SurfaceFoam& fm, const CameraWaterLayers& lw,
                                     float4* image, float4* aux, uint32_t* image8, hipStream_t stream, int cus)
{
  return launch_render<true>(p, rc, cam, sh, image, aux, image8, stream, cus, fm, lw);
}

// key uint64[pixels] | hits uint32[pixels] | foam float[pixels] | image float4[pixels] | aux float4[pixels]:
// every array starts on a multiple of 16 bytes whatever the pixel count is
static size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

size_t camera_layers_scratch_bytes(int width, int height)
{
  const size_t n = (size_t)width * height;
  return pad16(n * 8) + 2 * pad16(n * 4) + 2 * n * 16;
}

void camera_layers_scratch(void* scratch, int width, int height, unsigned long long*& key, uint32_t*& hits,
                           float*& foam, float4*& image, float4*& aux)
{
  unsigned char* b = static_cast<unsigned char*>(scratch);
  const size_t n = (size_t)width * height;
  key = reinterpret_cast<unsigned long long*>(b);
  hits = reinterpret_cast<uint32_t*>(b + pad16(n * 8));
  foam = reinterpret_cast<float*>(b + pad16(n * 8) + pad16(n * 4));
  image = reinterpret_cast<float4*>(b + pad16(n * 8) + 2 * pad16(n * 4));
  aux = image + n;
}

hipError_t launch_camera_aux2_none(const CameraParams& cam, float4* aux2, hipStream_t stream, int cus)
{
  const int64_t n = (int64_t)cam.width * cam.height;
  return launch_points(k_camera_aux2_none, kCameraSprayThreads, n, stream, cus, n, aux2);
}

hipError_t launch_camera_spray(const CameraParams& cam, const ShadingParams& sh, const CameraSpray& s, float4* image,
                               uint32_t* image8, float4* aux2, hipStream_t stream, int cus)
{
  if (!s.records || s.max_records < 1 || s.max_records > ((int64_t)1 << 28) || !s.key || !s.hits || !s.foam ||
      !s.base || !s.aux || s.max_half < 0 || s.max_half > 8)
    return hipErrorInvalidValue;
  // a lane per record / pixel (launch_points, launch_common.h); the splat's grid is sized from max_records:
  // the count stays on the device
  const hipError_t e = launch_points(k_camera_splat, kCameraSprayThreads, s.max_records, stream, cus, cam, s);
  if (e != hipSuccess)
    return e;
  return launch_points(k_camera_composite, kCameraSprayThreads, (int64_t)cam.width * cam.height, stream, cus, cam, sh,
                       s, image, image8, aux2);
}

}  // namespace oceanfft
