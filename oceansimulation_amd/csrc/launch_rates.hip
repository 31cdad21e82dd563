// launch_rates.hip — the packed time-derivative images of a whole-grid generator (device/k_rates.h):
// one launch over every cascade, in the shape pack_shape (launch_common.h) gives; the batched EncodeIFFT
// that turns them into the rate maps is the caller's (ocean_generator_calculate_rates).
#include "device/k_rates.h"
#include "launch_common.h"
#include "ocean_internal.h"

namespace oceanfft
{

hipError_t launch_rates_pack(int logn, const FrameParams& fp, int h0_blk, const float4* h0, float4* rates,
                             hipStream_t stream, int cus)
{
  PackShape s;
  if (pack_shape(logn, h0_blk, fp.cascades, s) != hipSuccess)
    return hipErrorInvalidValue;
  auto launch = [&](auto kernel) {
    const int grid = persistent_grid(kernel, kRatesTile, 0, s.items, cus);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kRatesTile), 0, stream, fp, logn, s.logb, s.lcw, h0, rates,
                       s.items);
  };
  if (s.block)
    launch(k_rates_pack<true>);
  else
    launch(k_rates_pack<false>);
  return hipGetLastError();
}

}  // namespace oceanfft
