// device/surface_sample.h — the GL_LINEAR + GL_REPEAT sampling of the generator's maps and the stages
// built on it that more than one translation unit runs: the vertex stage (ocean_kernels.hip's surface
// kernels, device/k_hulls.h, device/k_raycast.h), the fragment stage (ocean_kernels.hip, device/k_raycast.h)
// and the velocity of a water particle (k_surface_velocity, device/k_hulls.h).
// Everything is unfused fp32: the oracle and the numpy references are matched bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include "ocean_internal.h"

namespace oceanfft
{

// The four taps and weights of one sample: the texel indices of (i0, j0), (i1, j0), (i0, j1), (i1, j1).
struct LinearTaps
{
  int o00, o10, o01, o11;
  float w00, w10, w01, w11;
};

__device__ __forceinline__ LinearTaps linear_repeat_taps(int n, float u, float v)
{
#pragma clang fp contract(off)
  const float s = u * (float)n - 0.5f, t = v * (float)n - 0.5f;
  const float fs = floorf(s), ft = floorf(t);
  const float a = s - fs, b = t - ft;
  const int m = n - 1;  // n is a power of two: & m is the repeat wrap, also for negative indices
  const int i0 = (int)fs & m, j0 = (int)ft & m, i1 = (i0 + 1) & m, j1 = (j0 + 1) & m;
  return LinearTaps{j0 * n + i0, j0 * n + i1, j1 * n + i0, j1 * n + i1, (1.0f - a) * (1.0f - b), a * (1.0f - b),
                    (1.0f - a) * b, a * b};
}

// Channel ch of a map of CH floats per texel, filtered: each stage loads only the channels it uses, one
// dword per tap (the vertex stage 3 of 8, the normal stage 5 of 9): 2.95 -> 2.49 ms for the 4096^2-quad
// mesh, bit-identical (tools/microbench/surfbench, profiles/r06_surfbench.log). A sampling wave's taps
// are scattered (the camera warp spreads far vertices ~10 texels apart on a 5 m cascade), so the cost
// is per load instruction: ATLAS repacks the channels each stage uses into one 16-B texel (one load per
// tap and stage, plus the Jacobian's dword): 2.47 -> 1.35 ms with the repack included, 0.212 -> 0.121 ms
// for the 1024^2-quad mesh, bit-identical (profiles/r06_surfbench2.log).
template <int CH>
__device__ __forceinline__ float linear_channel(const float* __restrict__ tex, const LinearTaps& k, int ch)
{
#pragma clang fp contract(off)
  const float q00 = tex[k.o00 * CH + ch], q10 = tex[k.o10 * CH + ch], q01 = tex[k.o01 * CH + ch],
              q11 = tex[k.o11 * CH + ch];
  return k.w00 * q00 + k.w10 * q10 + k.w01 * q01 + k.w11 * q11;
}

// The bilinear sum of the four taps' lanes x, y, z, w (each as linear_channel's sum)
__device__ __forceinline__ float4 linear_texel(const float4* __restrict__ tex, const LinearTaps& k)
{
#pragma clang fp contract(off)
  const float4 q00 = tex[k.o00], q10 = tex[k.o10], q01 = tex[k.o01], q11 = tex[k.o11];
  return make_float4(k.w00 * q00.x + k.w10 * q10.x + k.w01 * q01.x + k.w11 * q11.x,
                     k.w00 * q00.y + k.w10 * q10.y + k.w01 * q01.y + k.w11 * q11.y,
                     k.w00 * q00.z + k.w10 * q10.z + k.w01 * q01.z + k.w11 * q11.z,
                     k.w00 * q00.w + k.w10 * q10.w + k.w01 * q01.w + k.w11 * q11.w);
}

// Vertex stage (waveShader.glsl:101-110): cascade c samples at the position cascades < c displaced and
// adds (scale * Dx, h, scale * Dz). (px, pz) enters as the base position, py as 0.
template <bool ATLAS>
__device__ __forceinline__ void surface_vertex_stage(const SurfaceParams& p, float& px, float& py, float& pz)
{
#pragma clang fp contract(off)
  const int nn = p.n * p.n;
  for (int c = 0; c < p.count; c++)
  {
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n, u, v);
    float h, dx, dz;
    if constexpr (ATLAS)
    {
      const float4 a = linear_texel(p.atlas + (size_t)(2 * c) * nn, k);
      h = a.x;
      dx = a.y;
      dz = a.z;
    }
    else
    {
      const float* hm = reinterpret_cast<const float*>(p.c[c].height);
      const float* dm = reinterpret_cast<const float*>(p.c[c].disp);
      h = linear_channel<4>(hm, k, 0);
      dx = linear_channel<4>(hm, k, 3);
      dz = linear_channel<4>(dm, k, 0);
    }
    px += p.c[c].scale * dx;
    py += h;
    pz += p.c[c].scale * dz;
  }
}

// Fragment stage at the displaced position (waveShader.glsl:127-144): (nx, ny, nz, averaged Jacobian)
template <bool ATLAS>
__device__ __forceinline__ float4 surface_fragment_stage(const SurfaceParams& p, float px, float pz)
{
#pragma clang fp contract(off)
  const int nn = p.n * p.n;
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, jac = 0.0f;
  for (int c = 0; c < p.count; c++)
  {
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n, u, v);
    float hx, dxx, hz, dzz;
    if constexpr (ATLAS)
    {
      const float4 b = linear_texel(p.atlas + (size_t)(2 * c + 1) * nn, k);
      hx = b.x;
      hz = b.y;
      dxx = b.z;
      dzz = b.w;
    }
    else
    {
      const float* hm = reinterpret_cast<const float*>(p.c[c].height);
      const float* dm = reinterpret_cast<const float*>(p.c[c].disp);
      hx = linear_channel<4>(hm, k, 1);
      dxx = linear_channel<4>(dm, k, 1);
      hz = linear_channel<4>(hm, k, 2);
      dzz = linear_channel<4>(dm, k, 2);
    }
    jac += linear_channel<1>(p.c[c].jac, k, 0) / (float)p.count;
    const float f = p.c[c].scale;
    d[0] += hx;        // dh/dx
    d[1] += dxx * f;   // dDx/dx
    d[2] += hz;        // dh/dz
    d[3] += dzz * f;   // dDz/dz
  }
  const float sx = d[0] / (1.0f + d[1]), sz = d[2] / (1.0f + d[3]);
  const float nx = -sx, ny = 1.0f, nz = -sz;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  return make_float4(nx / len, ny / len, nz / len, jac);
}

// ocean_surface_velocity's loop (include/oceanfft.h): (px, pz) enters as the base point, py and u as 0;
// on return p is the displaced position (the vertex stage's bits) and u the particle's velocity.
__device__ __forceinline__ void surface_particle_velocity(const SurfaceParams& p, const SurfaceRates& r, float& px,
                                                          float& py, float& pz, float& ux, float& uy, float& uz)
{
#pragma clang fp contract(off)
  for (int c = 0; c < p.count; c++)
  {
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n, u, v);
    const float4 h = linear_texel(p.c[c].height, k), d = linear_texel(p.c[c].disp, k);
    const float* rh = reinterpret_cast<const float*>(r.height[c]);
    const float* rd = reinterpret_cast<const float*>(r.disp[c]);
    const float rh_h = linear_channel<4>(rh, k, 0), rh_dx = linear_channel<4>(rh, k, 3);
    const float rd_dz = linear_channel<4>(rd, k, 0);
    const float s = p.c[c].scale;
    const float vx = s * (rh_dx + (d.y * ux + d.w * uz));  // dDx/dt + grad Dx . u
    const float vy = rh_h + (h.y * ux + h.z * uz);         // dh/dt + grad h . u
    const float vz = s * (rd_dz + (d.w * ux + d.z * uz));  // dDz/dt + grad Dz . u
    px += s * h.w;
    py += h.x;
    pz += s * d.x;
    ux += vx;
    uy += vy;
    uz += vz;
  }
}

}  // namespace oceanfft
