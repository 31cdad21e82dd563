// launch_surface.hip — the point kernels of the surface consumer (device/k_surface.h): the atlas repack,
// ocean_surface_sample[_plane], _sample[_plane]_foam, _query, _velocity and _sample[_plane]_lod, and the rules that decide when a
// request samples the atlas. The point kernels run on launch_points' grid (launch_common.h).
#include <cstdint>

#include "device/k_surface.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

// the repack of the cascades' maps into p.atlas (k_surface_atlas), ahead of a request that samples it
void launch_surface_atlas(const SurfaceParams& p, hipStream_t stream, int cus)
{
  const long texels = (long)p.count * p.n * p.n;
  long ab = (texels + 255) / 256;
  if (ab > (long)cus * 4)
    ab = (long)cus * 4;
  hipLaunchKernelGGL(k_surface_atlas, dim3((unsigned)ab), dim3(256), 0, stream, p);
}

// launch_points (launch_common.h, workgroups of 256) for a kernel with an atlas and a direct instantiation:
// p.atlas non-null runs the repack, then the atlas one.
template <typename K, typename... Args>
static hipError_t launch_points_atlas(K atlas, K direct, const SurfaceParams& p, int64_t count, hipStream_t stream,
                                      int cus, const Args&... args)
{
  if (p.atlas && count > 0)
    launch_surface_atlas(p, stream, cus);
  return launch_points(p.atlas ? atlas : direct, 256, count, stream, cus, p, args...);
}

hipError_t launch_surface(const SurfaceParams& p, const SurfacePlane& plane, const float2* xz, int64_t count,
                          float4* out, hipStream_t stream, int cus)
{
  return launch_points_atlas(k_surface<true>, k_surface<false>, p, count, stream, cus, plane, xz, count, out);
}

hipError_t launch_surface_foam(const SurfaceParams& p, const SurfaceFoam& f, const SurfacePlane& plane, const float2* xz,
                               int64_t count, float4* out, hipStream_t stream, int cus)
{
  return launch_points(k_surface_foam, 256, count, stream, cus, p, f, plane, xz, count, out);
}

hipError_t launch_surface_query(const SurfaceParams& p, const float2* xz, int64_t count, int iterations,
                                float tolerance, float4* out, hipStream_t stream, int cus)
{
  return launch_points_atlas(k_surface_query<true>, k_surface_query<false>, p, count, stream, cus, xz, count,
                             iterations, tolerance, out);
}

hipError_t launch_surface_velocity(const SurfaceParams& p, const SurfaceRates& r, const float2* xz, int64_t count,
                                   float4* out, hipStream_t stream, int cus)
{
  return launch_points(k_surface_velocity, 256, count, stream, cus, p, r, xz, count, out);
}

hipError_t launch_surface_lod(const SurfaceParams& p, const SurfacePlane& plane, const float* xzf, int64_t count,
                              float4* out, hipStream_t stream, int cus)
{
  return launch_points(k_surface_lod, 256, count, stream, cus, p, plane, xzf, count, out);
}

size_t surface_atlas_texels(const SurfaceParams& p) { return (size_t)2 * p.count * p.n * p.n; }

// The repack reads 36 B and writes 32 B per map texel and launches one more kernel; sampling from the
// atlas saves ~90 ps per vertex (profiles/r06_surfbench2.log). Used when the request's vertices
// outnumber the maps' texels 4 : 1 (and are at least 64 Ki) and the atlas stays within 256 MiB.
bool surface_use_atlas(const SurfaceParams& p, int64_t points)
{
  const size_t texels = surface_atlas_texels(p);
  return points >= 65536 && (uint64_t)points >= 2 * (uint64_t)texels && texels * 16 <= ((size_t)256 << 20);
}

// A query samples the vertex stage up to iterations + 1 times per point, so the repack pays much sooner
// than for a forward sample: measured on 3 x 256^2 and 3 x 1024^2 maps with each path forced at 4 Ki ..
// 1 Mi points and 0 / 1 / 2 / 4 / 8 / 16 iterations (tools/surface_query_bench.py,
// profiles/surface_query_bench.log), the atlas wins from 16 Ki points (256^2) and 64 Ki points (1024^2) at
// 2 or more iterations, and from 64 Ki and 128 Ki points at 0 or 1: e.g. 8 iterations on 64 Ki points of
// the 256^2 scene 56 -> 29 us, on 1025^2 points 900 -> 339 us. The repack costs ~6 us at 256^2 and ~31 us
// at 1024^2, hence a floor and a share of the atlas texels (2 per map texel and cascade).
bool surface_query_use_atlas(const SurfaceParams& p, int64_t points, int iterations)
{
  const size_t texels = surface_atlas_texels(p);
  const int64_t floor_points = iterations >= 2 ? 16384 : 65536;
  const uint64_t per_point = iterations >= 2 ? 96 : 48;  // atlas texels one point pays for
  return points >= floor_points && (uint64_t)points * per_point >= (uint64_t)texels &&
         texels * 16 <= ((size_t)256 << 20);
}

}  // namespace oceanfft
