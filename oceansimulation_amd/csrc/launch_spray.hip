// launch_spray.hip — spray emitters (device/k_spray.h): at most four launches per call, the count of every
// item, the scan over the items with the count table, and with a capacity the scatter of (d, id) and the
// dense fill of the records (on launch_points' grid, launch_common.h); the kernel boundaries are the ordering
// between them.
#include "device/k_spray.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

static size_t spray_items(int n) { return (size_t)kMaxSurfaceCascades * foam_tiles(n); }

// table (padded to 256 B) | offset int64[items] | partial uint32[items]
size_t spray_scratch_bytes(int n) { return 256 + spray_items(n) * (sizeof(int64_t) + sizeof(uint32_t)); }

void spray_scratch(void* scratch, int n, SprayCall& s)
{
  unsigned char* b = static_cast<unsigned char*>(scratch);
  s.table = reinterpret_cast<int64_t*>(b);
  s.offset = reinterpret_cast<int64_t*>(b + 256);
  s.partial = reinterpret_cast<uint32_t*>(s.offset + spray_items(n));
}

hipError_t launch_spray_emit(const SprayCall& s, const SurfaceParams& p, const SurfaceRates& r, const SprayTiles& tiles,
                             bool velocity, hipStream_t stream, int cus)
{
  const int n = s.n;
  if (n < 16 || n > 16384 || (n & (n - 1)) != 0 || s.nn != n * n || (1 << s.logn) != n || s.tiles != foam_tiles(n) ||
      s.pairs < 0 || s.pairs > kMaxSurfaceCascades || s.capacity < 0 || (s.capacity > 0 && !s.out) || p.n != n)
    return hipErrorInvalidValue;
  const int items = s.pairs * s.tiles;  // <= 16 * 2^17
  hipError_t e = hipSuccess;
  if (items > 0)
  {
    const int g1 = persistent_grid(k_spray_count, kSprayThreads, 0, items, cus);
    hipLaunchKernelGGL(k_spray_count, dim3((unsigned)g1), dim3(kSprayThreads), 0, stream, s);
    if ((e = hipGetLastError()) != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(k_spray_scan, dim3(1), dim3(kSprayScanThreads), 0, stream, s);
  if ((e = hipGetLastError()) != hipSuccess || s.capacity == 0)
    return e;
  if (items > 0)
  {
    const int g3 = persistent_grid(k_spray_scatter, kSprayThreads, 0, items, cus);
    hipLaunchKernelGGL(k_spray_scatter, dim3((unsigned)g3), dim3(kSprayThreads), 0, stream, s);
    if ((e = hipGetLastError()) != hipSuccess)
      return e;
  }
  // a thread per record (launch_points, launch_common.h), sized from the capacity: the count stays on the device
  if (velocity)
    return launch_points(k_spray_fill<true>, kSprayThreads, s.capacity, stream, cus, p, r, tiles,
                         (const int64_t*)s.table, s.logn, s.out);
  return launch_points(k_spray_fill<false>, kSprayThreads, s.capacity, stream, cus, p, r, tiles,
                       (const int64_t*)s.table, s.logn, s.out);
}

}  // namespace oceanfft
