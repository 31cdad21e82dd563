// device/k_raycast.h — ocean_surface_raycast (include/oceanfft.h): where a ray meets the displaced water
// surface. One lane per ray. The ray is clipped to the slab [sum of the cascades' minimum h - pad, sum of
// their maximum h + pad] read from the generators' bounds tables (device/k_bounds.h), then marched: every
// step is one evaluation E(t) of the gap between the ray and the water above its point, which is
// ocean_surface_query's fixed point on the vertex stage started from the previous evaluation's offset
// p - q (one step back along the ray the base point has moved little, so about one vertex stage per
// evaluation instead of the query's cold start). A lane is a small state machine (first evaluation, march,
// bisection, final evaluation) around ONE call site of E: lanes of a wave that are in different phases
// still run the vertex stage together, and a wave runs until its last lane is done, as in k_surface_query.
// Everything is unfused fp32 and follows the header's contract operation by operation
// (tests/raycast_ref.py restates it in numpy).
#pragma once

#include <hip/hip_runtime.h>

#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kRaycastThreads = 256;  // rays per work item

// IEEE minimum / maximum: NaN if either operand is NaN (numpy's np.minimum / np.maximum)
__device__ __forceinline__ float ray_min(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float ray_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

// grid: items = ceil(n_rays / 256), item loop
__global__ __launch_bounds__(kRaycastThreads) void k_surface_raycast(SurfaceParams p, RaycastParams rc,
                                                                     const float4* __restrict__ rays, int64_t n_rays,
                                                                     float4* __restrict__ out)
{
#pragma clang fp contract(off)
  enum { FIRST, MARCH, REFINE, FINAL, DONE };
  // the slab (wave-uniform)
  float ylo = 0.0f, yhi = 0.0f;
  for (int c = 0; c < p.count; c++)
  {
    ylo += rc.bounds[c][0];
    yhi += rc.bounds[c][1];
  }
  ylo -= rc.pad;
  yhi += rc.pad;
  const int64_t items = (n_rays + kRaycastThreads - 1) / kRaycastThreads;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int64_t idx = item * kRaycastThreads + threadIdx.x;
    if (idx >= n_rays)
      continue;
    const float4 ro = rays[2 * idx], rd = rays[2 * idx + 1];
    const float ox = ro.x, oy = ro.y, oz = ro.z, dx = rd.x, dy = rd.y, dz = rd.z;
    // clip
    float t0 = ro.w, t1 = rd.w;
    bool outside = false;
    if (dy == 0.0f)
      outside = !(ylo <= oy && oy <= yhi);
    else
    {
      const float a = (ylo - oy) / dy, b = (yhi - oy) / dy;
      t0 = ray_max(t0, ray_min(a, b));
      t1 = ray_min(t1, ray_max(a, b));
    }
    if (!(t0 <= t1))
      outside = true;
    if (outside)
    {
      out[4 * idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      out[4 * idx + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      out[4 * idx + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      out[4 * idx + 3] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
      continue;
    }
    const float inv = rc.slope == __builtin_inff() ? 0.0f : 1.0f / (fabsf(dy) + rc.slope * sqrtf(dx * dx + dz * dz));
    int phase = FIRST, status = 0, steps = 0, left = rc.refine;
    bool below = false;
    float te = t0, ta = t0, ga = 0.0f, tb = t0, gb = 0.0f;
    float offx = 0.0f, offz = 0.0f;                              // the warm start p - q
    float qx = 0.0f, qz = 0.0f, bx = 0.0f, bz = 0.0f;            // the last evaluation's q and base point p
    float vx = 0.0f, vy = 0.0f, vz = 0.0f, g = 0.0f;             // its V(p) and gap
    while (phase != DONE)
    {
      // E(te)
      qx = ox + te * dx;
      qz = oz + te * dz;
      bx = qx + offx;
      bz = qz + offz;
      surface_base_point<false>(p, qx, qz, rc.iterations, rc.tolerance, bx, bz, vx, vy, vz);
      offx = bx - qx;
      offz = bz - qz;
      g = (oy + te * dy) - vy;
      // the lane's next evaluation
      bool advance = false;  // take the next marching step from (ta, ga)
      if (phase == FIRST)
      {
        ga = g;
        below = g <= 0.0f;
        phase = MARCH;
        advance = true;  // max_steps >= 1
      }
      else if (phase == MARCH)
      {
        gb = g;
        steps++;
        if ((gb <= 0.0f) != below)
          phase = REFINE;  // a crossing in (ta, tb]: status 0
        else
        {
          ta = tb;
          ga = gb;
          if (tb >= t1)
          {
            status = 2;
            phase = FINAL;
            te = ta;
          }
          else if (steps == rc.max_steps)
          {
            status = 3;
            phase = FINAL;
            te = ta;
          }
          else
            advance = true;
        }
      }
      else if (phase == REFINE)
      {
        if ((g <= 0.0f) == below)
        {
          ta = te;
          ga = g;
        }
        else
        {
          tb = te;
          gb = g;
        }
        left--;
      }
      else
        phase = DONE;
      if (advance)
      {
        tb = ray_min(ta + ray_max(rc.step, fabsf(ga) * inv), t1);
        te = tb;
      }
      if (phase == REFINE)
      {
        if (left > 0)
          te = 0.5f * (ta + tb);
        else
        {
          te = ta + (tb - ta) * (ga / (ga - gb));
          phase = FINAL;
        }
      }
    }
    const float4 f = surface_fragment_stage<false>(p, vx, vz);
    out[4 * idx]= make_float4(ox + te * dx, oy + te * dy, oz + te * dz, te);
    out[4 * idx + 1] = make_float4(f.x, f.y, f.z, f.w);
    out[4 * idx + 2] = make_float4(bx, vy, bz, surface_residual(qx, qz, vx, vz));
    out[4 * idx + 3] = make_float4((float)status, below ? 1.0f : 0.0f, (float)steps, g);
  }
}

}  // namespace oceanfft
