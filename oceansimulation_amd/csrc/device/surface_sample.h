// device/surface_sample.h — the GL_LINEAR + GL_REPEAT sampling of the generator's maps and the stages
// built on it that more than one kernel runs: the vertex stage and the query's fixed point on it (device/
// k_surface.h, device/k_hulls.h, device/k_raycast.h), the fragment stage and its tail (device/k_surface.h,
// device/k_raycast.h), the plane mesh's warp (k_surface, k_surface_lod) and the velocity of a water particle
// (k_surface_velocity, device/k_hulls.h). Each operation is defined here once, so a hull point, a ray
// evaluation and a query are the same fp32 operations in the same order.
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

// The fragment stage's tail (waveShader.glsl:139-144): the summed slopes d = (dh/dx, dDx/dx, dh/dz, dDz/dz)
// and the averaged Jacobian -> (nx, ny, nz, jac)
__device__ __forceinline__ float4 surface_normal(float d0, float d1, float d2, float d3, float jac)
{
#pragma clang fp contract(off)
  const float sx = d0 / (1.0f + d1), sz = d2 / (1.0f + d3);
  const float nx = -sx, ny = 1.0f, nz = -sz;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  return make_float4(nx / len, ny / len, nz / len, jac);
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
  return surface_normal(d[0], d[1], d[2], d[3], jac);
}

// The persistent foam at the displaced position (ocean_surface_sample_foam): the cascades' foam maps
// accumulated exactly as the fragment stage above accumulates the Jacobian, same taps, weights and order
__device__ __forceinline__ float surface_foam_stage(const SurfaceParams& p, const SurfaceFoam& f, float px, float pz)
{
#pragma clang fp contract(off)
  float foam = 0.0f;
  for (int c = 0; c < p.count; c++)
  {
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n, u, v);
    foam += linear_channel<1>(f.foam[c], k, 0) / (float)p.count;
  }
  return foam;
}

// The query's fixed point (ocean_surface_query, include/oceanfft.h): the base point p whose displaced
// position V(p).xz is q, by p <- p + (q - V(p).xz), at most `iterations` steps, a lane stopping once
// max|q - V(p).xz| <= tolerance. base_x, base_z enter as the start (q itself for a cold start) and leave as
// the base point; out_v* leave as V(p). Only the vertex stage is iterated. Lanes of a wave stop at
// different steps: the wave runs until its last lane is done. |a| > tolerance is written as
// !(|a| <= tolerance), so a NaN residual keeps iterating instead of passing for converged.
template <bool ATLAS>
__device__ __forceinline__ void surface_base_point(const SurfaceParams& p, float qx, float qz, int iterations,
                                                   float tolerance, float& base_x, float& base_z, float& out_vx,
                                                   float& out_vy, float& out_vz)
{
#pragma clang fp contract(off)
  // The loop runs on locals: stores through the references, which may alias for all the compiler knows,
  // give the loop another shape than the one the three kernels had when each wrote it out.
  float bx = base_x, bz = base_z;
  float vx = bx, vy = 0.0f, vz = bz;
  surface_vertex_stage<ATLAS>(p, vx, vy, vz);
  for (int it = 0; it < iterations; it++)
  {
    const float rx = qx - vx, rz = qz - vz;
    if (fabsf(rx) <= tolerance && fabsf(rz) <= tolerance)
      break;
    bx += rx;
    bz += rz;
    vx = bx;
    vy = 0.0f;
    vz = bz;
    surface_vertex_stage<ATLAS>(p, vx, vy, vz);
  }
  base_x = bx;
  base_z = bz;
  out_vx = vx;
  out_vy = vy;
  out_vz = vz;
}

// max(|qx - vx|, |qz - vz|), NaN if either is: the residual a query reports
__device__ __forceinline__ float surface_residual(float qx, float qz, float vx, float vz)
{
#pragma clang fp contract(off)
  const float ex = fabsf(qx - vx), ez = fabsf(qz - vz);
  return (ex >= ez || ex != ex) ? ex : ez;
}

// The plane mesh (ocean_surface_sample_plane). The wave-uniform part, computed once ahead of the item
// loop: turnDir = normalize(forward.xz) rotated by 45 degrees (waveShader.glsl:84-88) and the clamped
// camera height; zeros for a request with positions (plane.res == 0).
struct SurfacePlaneTurn
{
  float tx, tz, cam_y;
};

__device__ __forceinline__ SurfacePlaneTurn surface_plane_turn(const SurfacePlane& plane)
{
#pragma clang fp contract(off)
  SurfacePlaneTurn t{0.0f, 0.0f, 0.0f};
  if (plane.res > 0)
  {
    const float fl = sqrtf(plane.fwd_x * plane.fwd_x + plane.fwd_z * plane.fwd_z);
    const float tx0 = plane.fwd_x / fl, tz0 = plane.fwd_z / fl;
    t.tx = (tx0 - tz0) * 0.70711f;
    t.tz = (tx0 + tz0) * 0.70711f;
    t.cam_y = fmaxf(plane.cam_y, 10.0f);
  }
  return t;
}

// Vertex idx of the mesh: the plane vertex (src/Renderer.cpp:18), + (15, 0, 15), rotate, distance scale,
// camera offset -> (px, pz); k is the vertex's warp factor (the LOD kernel's footprint is k * spacing)
__device__ __forceinline__ void surface_plane_point(const SurfacePlane& plane, const SurfacePlaneTurn& t, int64_t idx,
                                                    float& px, float& pz, float& k)
{
#pragma clang fp contract(off)
  const int side = plane.res + 1;
  const int i = (int)(idx % side), j = (int)(idx / side);
  const float x = -20.0f + 40.0f * (float)i / (float)plane.res + 15.0f;
  const float z = -20.0f + 40.0f * (float)j / (float)plane.res + 15.0f;
  const float rx = t.tx * x - t.tz * z, rz = x * t.tz + z * t.tx;
  const float len = sqrtf(rx * rx + rz * rz);
  k = powf(fmaxf(len, 1.0f), 1.2f) * t.cam_y * 0.04f;
  px = rx * k + plane.cam_x;
  pz = rz * k + plane.cam_z;
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
