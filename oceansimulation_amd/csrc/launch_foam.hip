// launch_foam.hip — the step of a whole-grid generator's persistent foam (device/k_foam.h): two launches per
// step, the tiles of every cascade (foam maps in place, partial counts), then one item per cascade into the
// count table; the kernel boundary is the ordering between them.
#include "device/k_foam.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

int foam_tiles(int n)
{
  const long nn = (long)n * n;
  return nn > kFoamTile ? (int)(nn / kFoamTile) : 1;
}

size_t foam_counts_bytes(int n, int cascades)
{
  return (size_t)cascades * kFoamCounts * (sizeof(int64_t) + (size_t)foam_tiles(n) * sizeof(uint32_t));
}

hipError_t launch_foam_step(int n, int cascades, const float* jac, float* foam, void* counts, const FoamCascade* c,
                            hipStream_t stream, int cus)
{
  if (n < 16 || n > 16384 || (n & (n - 1)) != 0 || cascades < 1 || cascades > kMaxCascades)
    return hipErrorInvalidValue;
  FoamStep s{};
  s.jac = jac;
  s.foam = foam;
  s.table = static_cast<int64_t*>(counts);
  s.partial = reinterpret_cast<uint32_t*>(s.table + (size_t)cascades * kFoamCounts);
  s.nn = n * n;
  s.tiles = foam_tiles(n);
  s.cascades = cascades;
  for (int i = 0; i < cascades; i++)
    s.c[i] = c[i];
  const int items = cascades * s.tiles;  // <= 64 * 2^17
  const int g1 = persistent_grid(k_foam_step, kFoamThreads, 0, items, cus);
  hipLaunchKernelGGL(k_foam_step, dim3((unsigned)g1), dim3(kFoamThreads), 0, stream, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return e;
  const int g2 = persistent_grid(k_foam_fold, kFoamFoldThreads, 0, cascades, cus);
  hipLaunchKernelGGL(k_foam_fold, dim3((unsigned)g2), dim3(kFoamFoldThreads), 0, stream, s);
  return hipGetLastError();
}

}  // namespace oceanfft
