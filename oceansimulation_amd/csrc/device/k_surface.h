// device/k_surface.h — the point kernels of the surface consumer: the atlas repack,
// ocean_surface_sample[_plane] (k_surface), ocean_surface_query, ocean_surface_velocity and the
// footprint-aware ocean_surface_sample[_plane]_lod (include/oceanfft.h). One thread per point, item loops
// on the grid of launch_common.h's launch_points.
//
// resources/waveShader.glsl evaluated per mesh vertex on the generator's maps. Vertex stage (:101-110):
// each cascade samples heightMap/displacementMap at pos.xz / planeSize, the position the earlier cascades
// already displaced, and adds (scale * Dx, h, scale * Dz). Fragment stage at the displaced position
// (:127-144): summed slopes -> normal, averaged Jacobian. Sampling is GL_LINEAR + GL_REPEAT
// (src/Generator.cpp:116-119) in fp32 with the specification's weights, unfused and with correctly
// rounded division / sqrt, so the oracle restatement (oracle_surface_vertex) is matched bit for bit.
// Memory: the maps of a scene (3 x 256^2 x 36 B) live in L2; per vertex 32 B are written.
//
// The taps, the filtered channel / texel, the two stages, the query's fixed point and the plane warp are
// in device/surface_sample.h (shared with device/k_hulls.h and device/k_raycast.h), the two stages on the mip
// pyramid in device/surface_lod.h (shared with device/k_camera.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/surface_lod.h"
#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

// the surface atlas of the cascades' maps (SurfaceParams::atlas)
__global__ __launch_bounds__(256) void k_surface_atlas(SurfaceParams p)
{
  const int nn = p.n * p.n;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < p.count * nn; idx += gridDim.x * blockDim.x)
  {
    const int c = idx / nn, t = idx - c * nn;
    const float4 h = p.c[c].height[t], d = p.c[c].disp[t];
    p.atlas[(size_t)(2 * c) * nn + t] = make_float4(h.x, h.w, d.x, 0.0f);
    p.atlas[(size_t)(2 * c + 1) * nn + t] = make_float4(h.y, h.z, d.y, d.z);
  }
}

template <bool ATLAS>
__global__ __launch_bounds__(256) void k_surface(SurfaceParams p, SurfacePlane plane, const float2* __restrict__ xz,
                                                 int64_t count, float4* __restrict__ out)
{
#pragma clang fp contract(off)
  const SurfacePlaneTurn turn = surface_plane_turn(plane);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < count;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    float px, pz;
    if (plane.res > 0)
    {
      float k;
      surface_plane_point(plane, turn, idx, px, pz, k);
    }
    else
    {
      const float2 q = xz[idx];
      px = q.x;
      pz = q.y;
    }
    float py = 0.0f;
    surface_vertex_stage<ATLAS>(p, px, py, pz);
    const float4 f = surface_fragment_stage<ATLAS>(p, px, pz);
    out[2 * idx] = make_float4(px, py, pz, f.w);
    out[2 * idx + 1] = make_float4(f.x, f.y, f.z, 0.0f);
  }
}

// k_surface<false> with the persistent foam (ocean_surface_sample_foam, include/oceanfft.h) in slot 7: the
// foam maps travel in an argument of their own, as the rate maps do; per tap and cascade one more dword
// beside the nine of the two stages.
__global__ __launch_bounds__(256) void k_surface_foam(SurfaceParams p, SurfaceFoam foam, SurfacePlane plane,
                                                      const float2* __restrict__ xz, int64_t count,
                                                      float4* __restrict__ out)
{
#pragma clang fp contract(off)
  const SurfacePlaneTurn turn = surface_plane_turn(plane);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < count;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    float px, pz;
    if (plane.res > 0)
    {
      float k;
      surface_plane_point(plane, turn, idx, px, pz, k);
    }
    else
    {
      const float2 q = xz[idx];
      px = q.x;
      pz = q.y;
    }
    float py = 0.0f;
    surface_vertex_stage<false>(p, px, py, pz);
    const float4 f = surface_fragment_stage<false>(p, px, pz);
    out[2 * idx] = make_float4(px, py, pz, f.w);
    out[2 * idx + 1] = make_float4(f.x, f.y, f.z, surface_foam_stage(p, foam, px, pz));
  }
}

// The inverse direction (ocean_surface_query, include/oceanfft.h): surface_base_point from a cold start
// (one 16-B load per tap and cascade from the atlas, three dwords from the maps); the fragment stage runs
// once, at the last V(p). A NaN residual keeps iterating and reaches slot 7.
template <bool ATLAS>
__global__ __launch_bounds__(256) void k_surface_query(SurfaceParams p, const float2* __restrict__ xz, int64_t count,
                                                       int iterations, float tolerance, float4* __restrict__ out)
{
#pragma clang fp contract(off)
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < count;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    const float2 q = xz[idx];
    float bx = q.x, bz = q.y;  // the base point p
    float vx, vy, vz;
    surface_base_point<ATLAS>(p, q.x, q.y, iterations, tolerance, bx, bz, vx, vy, vz);
    const float4 f = surface_fragment_stage<ATLAS>(p, vx, vz);
    out[2 * idx] = make_float4(bx, vy, bz, f.w);
    out[2 * idx + 1] = make_float4(f.x, f.y, f.z, surface_residual(q.x, q.y, vx, vz));
  }
}

// The velocity of the water particle whose rest position is the base point (ocean_surface_velocity,
// include/oceanfft.h): d/dt of the vertex stage V(p). Cascade c samples at the position the earlier
// cascades displaced, which itself moves with the velocity u accumulated so far, so its share is the
// rate maps' sample plus grad(field) . u, the gradients being map channels (dDx/dz = dDz/dx). The
// position advances exactly as in surface_vertex_stage (same taps, weights and sums), so slots 0-2 are
// ocean_surface_sample's bits. Per cascade and tap two 16-B loads (the maps) and three dwords (the rates).
__global__ __launch_bounds__(256) void k_surface_velocity(SurfaceParams p, SurfaceRates r, const float2* __restrict__ xz,
                                                          int64_t count, float4* __restrict__ out)
{
#pragma clang fp contract(off)
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < count;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    const float2 q = xz[idx];
    float px = q.x, py = 0.0f, pz = q.y;
    float ux = 0.0f, uy = 0.0f, uz = 0.0f;
    surface_particle_velocity(p, r, px, py, pz, ux, uy, uz);
    out[2 * idx] = make_float4(px, py, pz, 0.0f);
    out[2 * idx + 1] = make_float4(ux, uy, uz, 0.0f);
  }
}

// k_surface with a footprint per point: xzf = (x, z, footprint) triples, or on the plane mesh the spacing
// of the warped vertices, k * (40 / res) with k the vertex's warp factor. Slot 7: the footprint used.
__global__ __launch_bounds__(256) void k_surface_lod(SurfaceParams p, SurfacePlane plane, const float* __restrict__ xzf,
                                                     int64_t count, float4* __restrict__ out)
{
#pragma clang fp contract(off)
  const SurfacePlaneTurn turn = surface_plane_turn(plane);
  const int top = 31 - __clz(p.n);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < count;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    float px, pz, footprint;
    if (plane.res > 0)
    {
      float k;
      surface_plane_point(plane, turn, idx, px, pz, k);
      footprint = k * (40.0f / (float)plane.res);
    }
    else
    {
      px = xzf[3 * idx];
      pz = xzf[3 * idx + 1];
      footprint = xzf[3 * idx + 2];
    }
    float py = 0.0f;
    surface_vertex_stage_lod(p, top, footprint, px, py, pz);
    const float4 f = surface_fragment_stage_lod(p, top, footprint, px, pz);
    out[2 * idx] = make_float4(px, py, pz, f.w);
    out[2 * idx + 1] = make_float4(f.x, f.y, f.z, footprint);
  }
}

}  // namespace oceanfft
