// launch_wake.hip — the wake windows (device/k_wake.h). ocean_wake_step is the splat (skipped without records),
// one launch per substep (the 6-texel halo makes a substep a global dependency: the kernel boundary is the
// ordering) and the launch that zeroes the accumulators the splat touched: substeps + 2 launches at most. The
// record count stays on the device, so the splat's grids are sized from max_records.
#include "device/k_wake.h"
#include "launch_common.h"
#include "ocean_internal.h"

#include <utility>

namespace oceanfft
{

static bool wake_ok(const WakeCall& c)
{
  return c.h && c.h_prev && c.acc && c.m >= 32 && c.m <= 4096 && c.m % 16 == 0;
}

template <bool CLEAR>
static hipError_t splat(const WakeCall& c, hipStream_t stream, int cus)
{
  int64_t items = (c.max_records + kWakeThreads - 1) / kWakeThreads;  // <= 2^20
  if (items > kWakeSplatMaxGrid)
    items = kWakeSplatMaxGrid;
  const int grid = persistent_grid(k_wake_splat<CLEAR>, kWakeThreads, 0, (int)items, cus);
  hipLaunchKernelGGL(k_wake_splat<CLEAR>, dim3((unsigned)grid), dim3(kWakeThreads), 0, stream, c);
  return hipGetLastError();
}

template <bool FORCED>
static hipError_t substep(const WakeCall& c, hipStream_t stream, int cus)
{
  const int tiles = (c.m + kWakeTile - 1) / kWakeTile;
  const int grid = persistent_grid(k_wake_substep<FORCED>, kWakeThreads, 0, tiles * tiles, cus);
  hipLaunchKernelGGL(k_wake_substep<FORCED>, dim3((unsigned)grid), dim3(kWakeThreads), 0, stream, c);
  return hipGetLastError();
}

hipError_t launch_wake_step(WakeCall& c, int substeps, hipStream_t stream, int cus)
{
  if (!wake_ok(c) || substeps < 1 || substeps > 64 || c.max_records < 0 || c.max_records > ((int64_t)1 << 28) ||
      (c.max_records > 0 && !c.records))
    return hipErrorInvalidValue;
  const bool forced = c.max_records > 0;
  hipError_t e = forced ? splat<false>(c, stream, cus) : hipSuccess;
  for (int k = 0; k < substeps && e == hipSuccess; k++)
  {
    e = forced ? substep<true>(c, stream, cus) : substep<false>(c, stream, cus);
    std::swap(c.h, c.h_prev);  // the new h was written over h_prev
  }
  if (e == hipSuccess && forced)
    e = splat<true>(c, stream, cus);
  return e;
}

hipError_t launch_wake_shift(const WakeCall& c, int di, int dj, hipStream_t stream, int cus)
{
  if (!wake_ok(c))
    return hipErrorInvalidValue;
  const int64_t mm = (int64_t)c.m * c.m;
  hipError_t e = launch_points(k_wake_shift<0>, kWakeThreads, mm, stream, cus, c, di, dj);
  if (e == hipSuccess)
    e = launch_points(k_wake_shift<1>, kWakeThreads, mm, stream, cus, c, di, dj);
  if (e == hipSuccess)
    e = hipMemsetAsync(c.acc, 0, (size_t)mm * sizeof(long long), stream);
  return e;
}

hipError_t launch_wake_sample(const WakeCall& c, const float* xz, int64_t n, float* out, hipStream_t stream, int cus)
{
  if (!wake_ok(c) || n < 0 || (n > 0 && (!xz || !out)))
    return hipErrorInvalidValue;
  return launch_points(k_wake_sample, kWakeThreads, n, stream, cus, c, reinterpret_cast<const float2*>(xz), n,
                       reinterpret_cast<float4*>(out));
}

}  // namespace oceanfft
