// launch_rates.hip — the packed time-derivative images of a whole-grid generator (device/k_rates.h):
// one launch over every cascade; the batched EncodeIFFT that turns them into the rate maps is the
// caller's (ocean_generator_calculate_rates).
#include "device/k_rates.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_rates_pack(int logn, const FrameParams& fp, int h0_blk, const float4* h0, float4* rates,
                             hipStream_t stream, int cus)
{
  int logb = 0;
  while ((1 << logb) < h0_blk)
    logb++;
  if (logn < 4 || logn > 14 || h0_blk < 1 || (1 << logb) != h0_blk || logb > logn || fp.cascades < 1 ||
      fp.cascades > kMaxCascades)
    return hipErrorInvalidValue;
  // the block shape wherever its CW x 1024 / CW block fits the image (device/k_rates.h): every N >= 64
  int lcw = logb + 2 < 3 ? 3 : (logb + 2 > 6 ? 6 : logb + 2);  // CW = min(max(4 B, 8), 64)
  const bool block = lcw <= logn && 10 - lcw <= logn;
  const int items = fp.cascades << (2 * logn - (block ? 10 : 8));  // <= 64 * 2^20
  if (block)
  {
    const int grid = persistent_grid(k_rates_pack<true>, kRatesTile, 0, items, cus);
    hipLaunchKernelGGL(k_rates_pack<true>, dim3((unsigned)grid), dim3(kRatesTile), 0, stream, fp, logn, logb, lcw, h0,
                       rates, items);
  }
  else
  {
    const int grid = persistent_grid(k_rates_pack<false>, kRatesTile, 0, items, cus);
    hipLaunchKernelGGL(k_rates_pack<false>, dim3((unsigned)grid), dim3(kRatesTile), 0, stream, fp, logn, logb, lcw, h0,
                       rates, items);
  }
  return hipGetLastError();
}

}  // namespace oceanfft
