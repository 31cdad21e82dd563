// device/ray_march.h — one lane's ray against the displaced water surface: the slab, the clip and the state
// machine of ocean_surface_raycast's contract (include/oceanfft.h), defined once for the two kernels that
// march rays, k_surface_raycast (device/k_raycast.h) and k_camera_render (device/k_camera.h). Unfused fp32.
#pragma once

#include <hip/hip_runtime.h>

#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

// IEEE minimum / maximum: NaN if either operand is NaN (numpy's np.minimum / np.maximum)
__device__ __forceinline__ float ray_min(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float ray_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

// What the march of one ray leaves: the header's rows before they are laid out
struct RayMarch
{
  int status, steps;
  bool below;
  float t;                 // of the final evaluation
  float qx, qz, bx, bz;    // its q and base point p
  float vx, vy, vz, g;     // its V(p) and gap
};

// The slab of a call (wave-uniform): [sum of the minima - pad, sum of the maxima + pad]
__device__ __forceinline__ void ray_slab(const SurfaceParams& p, const RaycastParams& rc, float& ylo, float& yhi)
{
#pragma clang fp contract(off)
  ylo = 0.0f;
  yhi = 0.0f;
  for (int c = 0; c < p.count; c++)
  {
    ylo += rc.bounds[c][0];
    yhi += rc.bounds[c][1];
  }
  ylo -= rc.pad;
  yhi += rc.pad;
}

// One lane's ray: clip and state machine (k_surface_raycast and device/k_camera.h's k_camera_render run
// it, so E has one call site in either). False: OUTSIDE, m untouched.
__device__ __forceinline__ bool ray_march(const SurfaceParams& p, const RaycastParams& rc, float ylo, float yhi,
                                          float ox, float oy, float oz, float tmin, float dx, float dy, float dz,
                                          float tmax, RayMarch& m)
{
#pragma clang fp contract(off)
  enum { FIRST, MARCH, REFINE, FINAL, DONE };
  // clip
  float t0 = tmin, t1 = tmax;
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
    return false;
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
  m = RayMarch{status, steps, below, te, qx, qz, bx, bz, vx, vy, vz, g};
  return true;
}

}  // namespace oceanfft
