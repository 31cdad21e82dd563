// launch_moorings.hip — mooring lines (device/k_moorings.h): the reset (one launch), and the step: one launch
// over the work items, a wave each, for all substeps of the call, then one over the bodies for their wrenches.
#include <algorithm>

#include "device/k_moorings.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_moorings_reset(const MooringCall& m, hipStream_t stream, int cus)
{
  if (m.items < 1 || !m.nodes)
    return hipErrorInvalidValue;
  // one-wave workgroups: a one-shot grid stays below HIP's 2^32 threads per launch
  const int grid = std::min(persistent_grid(k_moorings_reset, kMooringMaxNodes, 0, m.items, cus), 1 << 24);
  hipLaunchKernelGGL(k_moorings_reset, dim3((unsigned)grid), dim3(kMooringMaxNodes), 0, stream, m);
  return hipGetLastError();
}

template <bool WATER>
static void launch_lines(const SurfaceParams& p, const WaterLayers& w, const MooringCall& m, hipStream_t stream, int cus)
{
  const int grid = std::min(persistent_grid(k_moorings_step<WATER>, kMooringMaxNodes, 0, m.items, cus), 1 << 24);
  hipLaunchKernelGGL(k_moorings_step<WATER>, dim3((unsigned)grid), dim3(kMooringMaxNodes), 0, stream, p, w, m);
}

hipError_t launch_moorings_step(const SurfaceParams& p, const WaterLayers& w, bool water, const MooringCall& m,
                                const MooringWrench& q, hipStream_t stream, int cus)
{
  if (m.items < 1 || m.substeps < 1 || !m.nodes || !m.fm || q.bodies < 0 ||
      (water && (p.count < 1 || p.count > kMaxSurfaceCascades || w.layers < 1 || w.layers > kMaxDepthLayers)))
    return hipErrorInvalidValue;
  water ? launch_lines<true>(p, w, m, stream, cus) : launch_lines<false>(p, w, m, stream, cus);
  if (q.bodies > 0)
  {
    const hipError_t e = launch_points(k_moorings_wrench, 256, q.bodies, stream, cus, q);
    if (e != hipSuccess)
      return e;
  }
  return hipGetLastError();
}

}  // namespace oceanfft
