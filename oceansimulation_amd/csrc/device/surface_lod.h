// device/surface_lod.h — the vertex and fragment stages on the mip pyramid (device/k_mips.h): what
// k_surface_lod (device/k_surface.h) and k_camera_render (device/k_camera.h) both run, defined once.
// Unfused fp32, as device/surface_sample.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/mip_index.h"
#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

// Footprint-aware sampling (ocean_surface_sample_lod, include/oceanfft.h): a sample whose neighbours sit
// `footprint` metres away covers r = footprint * N / planeSize texels of cascade c's level 0, so it reads
// level l = floor(log2 r) and level l + 1 of the mip pyramid (device/k_mips.h) and blends them by
// f = r / 2^l - 1 in [0, 1): linear in the footprint, continuous across levels. l is r's exponent field
// and f is exact (a scaling by a power of two and a subtraction in [1, 2)), so no log2f is involved.
struct SurfaceLod
{
  int l;
  float f;
};

__device__ __forceinline__ SurfaceLod surface_lod(float footprint, int n, int top, float plane)
{
#pragma clang fp contract(off)
  const float r = (footprint * (float)n) / plane;
  if (!(r >= 1.0f))  // also NaN
    return SurfaceLod{0, 0.0f};
  if (r >= (float)(1 << top))  // also +inf
    return SurfaceLod{top, 0.0f};
  const int l = (int)(__float_as_uint(r) >> 23) - 127;
  return SurfaceLod{l, r * __uint_as_float((uint32_t)(127 - l) << 23) - 1.0f};
}

// Level l of a map whose chain (levels >= 1) is `mip`, CH floats per texel
template <int CH>
__device__ __forceinline__ const float* surface_level(const void* map, const void* mip, int n, int l)
{
  return l == 0 ? static_cast<const float*>(map) : static_cast<const float*>(mip) + mip_level_offset(n, l) * CH;
}

__device__ __forceinline__ float lod_blend(float a, float b, float f)
{
#pragma clang fp contract(off)
  return a + f * (b - a);
}

// surface_vertex_stage with cascade c's (l, f): A = level l, B = level l + 1 (read only when f != 0;
// l == top has f == 0)
__device__ __forceinline__ void surface_vertex_stage_lod(const SurfaceParams& p, int top, float footprint, float& px,
                                                         float& py, float& pz)
{
#pragma clang fp contract(off)
  for (int c = 0; c < p.count; c++)
  {
    const SurfaceLod lod = surface_lod(footprint, p.n, top, p.c[c].plane);
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n >> lod.l, u, v);
    const float* hm = surface_level<4>(p.c[c].height, p.c[c].height_mip, p.n, lod.l);
    const float* dm = surface_level<4>(p.c[c].disp, p.c[c].disp_mip, p.n, lod.l);
    float h = linear_channel<4>(hm, k, 0), dx = linear_channel<4>(hm, k, 3), dz = linear_channel<4>(dm, k, 0);
    if (lod.f != 0.0f)
    {
      const LinearTaps kb = linear_repeat_taps(p.n >> (lod.l + 1), u, v);
      const float* hb = surface_level<4>(p.c[c].height, p.c[c].height_mip, p.n, lod.l + 1);
      const float* db = surface_level<4>(p.c[c].disp, p.c[c].disp_mip, p.n, lod.l + 1);
      h = lod_blend(h, linear_channel<4>(hb, kb, 0), lod.f);
      dx = lod_blend(dx, linear_channel<4>(hb, kb, 3), lod.f);
      dz = lod_blend(dz, linear_channel<4>(db, kb, 0), lod.f);
    }
    px += p.c[c].scale * dx;
    py += h;
    pz += p.c[c].scale * dz;
  }
}

// surface_fragment_stage with the same (l, f) per cascade, at the displaced position
__device__ __forceinline__ float4 surface_fragment_stage_lod(const SurfaceParams& p, int top, float footprint, float px,
                                                             float pz)
{
#pragma clang fp contract(off)
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, jac = 0.0f;
  for (int c = 0; c < p.count; c++)
  {
    const SurfaceLod lod = surface_lod(footprint, p.n, top, p.c[c].plane);
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n >> lod.l, u, v);
    const float* hm = surface_level<4>(p.c[c].height, p.c[c].height_mip, p.n, lod.l);
    const float* dm = surface_level<4>(p.c[c].disp, p.c[c].disp_mip, p.n, lod.l);
    const float* jm = surface_level<1>(p.c[c].jac, p.c[c].jac_mip, p.n, lod.l);
    float hx = linear_channel<4>(hm, k, 1), dxx = linear_channel<4>(dm, k, 1), hz = linear_channel<4>(hm, k, 2),
          dzz = linear_channel<4>(dm, k, 2), j = linear_channel<1>(jm, k, 0);
    if (lod.f != 0.0f)
    {
      const LinearTaps kb = linear_repeat_taps(p.n >> (lod.l + 1), u, v);
      const float* hb = surface_level<4>(p.c[c].height, p.c[c].height_mip, p.n, lod.l + 1);
      const float* db = surface_level<4>(p.c[c].disp, p.c[c].disp_mip, p.n, lod.l + 1);
      const float* jb = surface_level<1>(p.c[c].jac, p.c[c].jac_mip, p.n, lod.l + 1);
      hx = lod_blend(hx, linear_channel<4>(hb, kb, 1), lod.f);
      dxx = lod_blend(dxx, linear_channel<4>(db, kb, 1), lod.f);
      hz = lod_blend(hz, linear_channel<4>(hb, kb, 2), lod.f);
      dzz = lod_blend(dzz, linear_channel<4>(db, kb, 2), lod.f);
      j = lod_blend(j, linear_channel<1>(jb, kb, 0), lod.f);
    }
    jac += j / (float)p.count;
    const float f = p.c[c].scale;
    d[0] += hx;        // dh/dx
    d[1] += dxx * f;   // dDx/dx
    d[2] += hz;        // dh/dz
    d[3] += dzz * f;   // dDz/dz
  }
  return surface_normal(d[0], d[1], d[2], d[3], jac);
}

}  // namespace oceanfft
