// launch_bounds.hip — the bounds of a whole-grid generator's maps (device/k_bounds.h): two launches per
// build, the tiles of every cascade into partial rows, then one item per cascade into the table; the kernel
// boundary is the ordering between them.
#include "device/k_bounds.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

int bounds_tiles(int n)
{
  const long nn = (long)n * n;
  return nn > kBoundsTile ? (int)(nn / kBoundsTile) : 1;
}

size_t bounds_floats(int n, int cascades) { return (size_t)cascades * kBoundsValues * (1 + (size_t)bounds_tiles(n)); }

hipError_t launch_build_bounds(int n, int cascades, const float4* maps, const float* jac, float* bounds,
                               hipStream_t stream, int cus)
{
  if (n < 16 || n > 16384 || (n & (n - 1)) != 0 || cascades < 1 || cascades > kMaxCascades)
    return hipErrorInvalidValue;
  BoundsBuild s{};
  s.maps = maps;
  s.jac = jac;
  s.table = bounds;
  s.partial = bounds + (size_t)cascades * kBoundsValues;
  s.nn = n * n;
  s.tiles = bounds_tiles(n);
  s.cascades = cascades;
  const int items = cascades * s.tiles;  // <= 64 * 2^17
  const int g1 = persistent_grid(k_bounds_tiles, kBoundsThreads, 0, items, cus);
  hipLaunchKernelGGL(k_bounds_tiles, dim3((unsigned)g1), dim3(kBoundsThreads), 0, stream, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return e;
  const int g2 = persistent_grid(k_bounds_fold, kBoundsFoldThreads, 0, cascades, cus);
  hipLaunchKernelGGL(k_bounds_fold, dim3((unsigned)g2), dim3(kBoundsFoldThreads), 0, stream, s);
  return hipGetLastError();
}

}  // namespace oceanfft
