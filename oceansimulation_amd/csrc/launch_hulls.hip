// launch_hulls.hip — the loads on a hull set's bodies (device/k_hulls.h): one launch over the 64-point
// tiles, one wave each, and, when a body has more than one tile, one over those bodies' partials. The step
// (device/k_hulls_step.h): one launch for all substeps of a set of one-tile bodies, else two per substep.
#include <algorithm>

#include "device/k_hulls.h"
#include "device/k_hulls_step.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

template <bool ATLAS, bool VELOCITY>
static void launch_tiles(const SurfaceParams& p, const SurfaceRates& r, const HullCall& h, hipStream_t stream, int cus)
{
  // one-wave workgroups: a one-shot grid stays below HIP's 2^32 threads per launch
  const int grid = std::min(persistent_grid(k_hulls_loads<ATLAS, VELOCITY>, kHullTile, 0, h.items, cus), 1 << 24);
  hipLaunchKernelGGL((k_hulls_loads<ATLAS, VELOCITY>), dim3((unsigned)grid), dim3(kHullTile), 0, stream, p, r, h);
}

hipError_t launch_hulls_loads(const SurfaceParams& p, const SurfaceRates& r, bool velocity, const HullCall& h,
                              const HullFold* folds, int n_folds, hipStream_t stream, int cus)
{
  if (h.items < 1 || n_folds < 0 || p.count < 1 || p.count > kMaxSurfaceCascades)
    return hipErrorInvalidValue;
  if (p.atlas)
    velocity ? launch_tiles<true, true>(p, r, h, stream, cus) : launch_tiles<true, false>(p, r, h, stream, cus);
  else
    velocity ? launch_tiles<false, true>(p, r, h, stream, cus) : launch_tiles<false, false>(p, r, h, stream, cus);
  if (n_folds > 0)
  {
    const int grid = persistent_grid(k_hulls_fold, kHullFoldThreads, 0, n_folds, cus);
    hipLaunchKernelGGL(k_hulls_fold, dim3((unsigned)grid), dim3(kHullFoldThreads), 0, stream, folds, n_folds,
                       h.partial, h.loads);
  }
  return hipGetLastError();
}

template <bool ATLAS, bool VELOCITY>
static void launch_step_tiles(const SurfaceParams& p, const SurfaceRates& r, const HullCall& h, const HullStep& st,
                              hipStream_t stream, int cus)
{
  const int grid = std::min(persistent_grid(k_hulls_step<ATLAS, VELOCITY>, kHullTile, 0, h.items, cus), 1 << 24);
  hipLaunchKernelGGL((k_hulls_step<ATLAS, VELOCITY>), dim3((unsigned)grid), dim3(kHullTile), 0, stream, p, r, h, st);
}

hipError_t launch_hulls_step(const SurfaceParams& p, const SurfaceRates& r, bool velocity, const HullCall& h,
                             HullStep st, int substeps, const HullFold* folds, int n_folds, hipStream_t stream,
                             int cus)
{
  if (h.items < 1 || n_folds < 0 || substeps < 1 || !st.poses || !st.props || p.count < 1 ||
      p.count > kMaxSurfaceCascades)
    return hipErrorInvalidValue;
  // the substeps a launch of k_hulls_step runs: all of them when every body is one tile
  const int launches = n_folds > 0 ? substeps : 1;
  st.substeps = n_folds > 0 ? 1 : substeps;
  for (int s = 0; s < launches; s++)
  {
    st.last = s == launches - 1;
    if (p.atlas)
      velocity ? launch_step_tiles<true, true>(p, r, h, st, stream, cus)
               : launch_step_tiles<true, false>(p, r, h, st, stream, cus);
    else
      velocity ? launch_step_tiles<false, true>(p, r, h, st, stream, cus)
               : launch_step_tiles<false, false>(p, r, h, st, stream, cus);
    if (n_folds > 0)
    {
      const int grid = persistent_grid(k_hulls_step_fold, kHullFoldThreads, 0, n_folds, cus);
      hipLaunchKernelGGL(k_hulls_step_fold, dim3((unsigned)grid), dim3(kHullFoldThreads), 0, stream, folds, n_folds,
                         h.partial, st.last ? h.loads : nullptr, st);
    }
  }
  return hipGetLastError();
}

}  // namespace oceanfft
