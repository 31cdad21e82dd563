// device/k_raycast.h — ocean_surface_raycast (include/oceanfft.h): where a ray meets the displaced water
// surface. One lane per ray. The ray is clipped to the slab [sum of the cascades' minimum h - pad, sum of
// their maximum h + pad] read from the generators' bounds tables (device/k_bounds.h), then marched: every
// step is one evaluation E(t) of the gap between the ray and the water above its point, which is
// ocean_surface_query's fixed point on the vertex stage started from the previous evaluation's offset
// p - q (one step back along the ray the base point has moved little, so about one vertex stage per
// evaluation instead of the query's cold start). A lane is a small state machine (ray_march in
// device/ray_march.h, shared with device/k_camera.h: first evaluation, march, bisection, final evaluation)
// around ONE call site of E: lanes of a wave that are in different phases
// still run the vertex stage together, and a wave runs until its last lane is done, as in k_surface_query.
// Everything is unfused fp32 and follows the header's contract operation by operation
// (tests/raycast_ref.py restates it in numpy).
#pragma once

#include <hip/hip_runtime.h>

#include "device/ray_march.h"
#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kRaycastThreads = 256;  // rays per work item

// grid: items = ceil(n_rays / 256), item loop
__global__ __launch_bounds__(kRaycastThreads) void k_surface_raycast(SurfaceParams p, RaycastParams rc,
                                                                     const float4* __restrict__ rays, int64_t n_rays,
                                                                     float4* __restrict__ out)
{
#pragma clang fp contract(off)
  float ylo, yhi;
  ray_slab(p, rc, ylo, yhi);
  const int64_t items = (n_rays + kRaycastThreads - 1) / kRaycastThreads;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int64_t idx = item * kRaycastThreads + threadIdx.x;
    if (idx >= n_rays)
      continue;
    const float4 ro = rays[2 * idx], rd = rays[2 * idx + 1];
    const float ox = ro.x, oy = ro.y, oz = ro.z, dx = rd.x, dy = rd.y, dz = rd.z;
    RayMarch m;
    if (!ray_march(p, rc, ylo, yhi, ox, oy, oz, ro.w, dx, dy, dz, rd.w, m))
    {
      out[4 * idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      out[4 * idx + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      out[4 * idx + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      out[4 * idx + 3] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
      continue;
    }
    const float4 f = surface_fragment_stage<false>(p, m.vx, m.vz);
    out[4 * idx] = make_float4(ox + m.t * dx, oy + m.t * dy, oz + m.t * dz, m.t);
    out[4 * idx + 1] = make_float4(f.x, f.y, f.z, f.w);
    out[4 * idx + 2] = make_float4(m.bx, m.vy, m.bz, surface_residual(m.qx, m.qz, m.vx, m.vz));
    out[4 * idx + 3] = make_float4((float)m.status, m.below ? 1.0f : 0.0f, (float)m.steps, m.g);
  }
}

}  // namespace oceanfft
