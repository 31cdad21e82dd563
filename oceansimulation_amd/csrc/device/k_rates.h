// device/k_rates.h — the time derivative of the frame's two packed images
// (ocean_generator_calculate_rates, include/oceanfft.h). The frame evolves H(k, t) = a e^{iwt} + b e^{-iwt}
// from the h0 texel (a, b); everything after H (the packing of prepareFFT and EncodeIFFT) is linear
// and does not depend on t, so the rate maps are the same pipeline fed with
//     Hd = dH/dt = i w (a e^{iwt} - b e^{-iwt}),
// w, the phase w * t and its sin / cos being the frame's own (make_kvec, dispersion_evolve,
// sincos_phase on the CascadeFrame the last column pass used). The packing is pack_height /
// pack_displacement unchanged: the reference's spectrum is not Hermitian on the Nyquist row and column,
// which leaks between the two real fields of a complex lane, and only the frame's own packing gives the
// exact derivative of all eight channels of the maps the library shows.
//
// Memory: a stream of 16 B read (h0) and 32 B written (two row-major packed images) per point.
// h0 is strip-blocked, texel (x, y) at ((x / B) N + y) B + x % B, the images are row-major; all sizes
// are powers of two, N^2 >= 256. Two shapes:
//   BLOCK  a work item is a block of CW columns x 1024 / CW rows of one cascade, four texels per thread
//          (element e = 256 j + thread: column e % CW, row e / CW), all four loads issued before the
//          first texel is evolved. CW = min(max(4 B, 8), 64), so a wave's store instruction writes
//          64 / CW rows of CW * 16 B >= 128 B, whole lines, and its load instruction reads from each of
//          the CW / B strips it spans (64 / CW) B * 16 B >= 128 contiguous bytes, whole lines again
//          (one strip and 1 KB when B >= 64). Needs CW <= N and 1024 / CW <= N: every N >= 64.
//   linear a work item is 256 consecutive texels of the blocked image, one per thread: a contiguous
//          4 KB read = B columns x 256 / B rows of a strip (several whole strips when a strip is shorter
//          than 256 texels), each row stored as one B * 16-B span. Any B; used for N = 16, 32.
// Measured at 8 x 4096^2 (B = 4, tools/rates_bench.py, profiles/rates_bench.log): BLOCK 1.33 ms, 0.60 of
// 8 TB/s at 48 B per point (a plain copy of the same bytes takes 1.28 ms); linear 1.95 ms (0.41), its
// half-line (64-B) store pieces being the cost; four linear tiles of neighbouring strips per work item,
// which complete the lines within one workgroup but still store them in halves, 1.81 ms.
// The walk from a work item to its texels (pack_item_texel) and Hd (evolve_rate) are device/evolve.h's,
// shared with k_kinematics_pack; the shape rule on the host is pack_shape (launch_common.h).
#pragma once

#include <hip/hip_runtime.h>

#include "device/evolve.h"

namespace oceanfft
{

constexpr int kRatesTile = 256;  // texels per work item = threads per workgroup

// rates: [cascade][height-rate image, displacement-rate image][n * n], row-major, still in k space
// (the batched EncodeIFFT follows). items = cascades * n * n / (BLOCK ? 1024 : 256); lcw = log2 CW.
template <bool BLOCK>
__global__ __launch_bounds__(kRatesTile) void k_rates_pack(FrameParams fp, int logn, int logb, int lcw,
                                                           const float4* __restrict__ h0,
                                                           float4* __restrict__ rates, int items)
{
  constexpr int J = BLOCK ? 4 : 1;
  const int n = 1 << logn;
  const float dim = (float)n;
  const int litems = 2 * logn - (BLOCK ? 10 : 8);  // log2 of the items per cascade
  const size_t nn = (size_t)n * n;
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int c = item >> litems;
    const unsigned local = (unsigned)(item - (c << litems));
    const float4* hc = h0 + (size_t)c * nn;
    int x[J], y[J];
    float4 a[J];
#pragma unroll
    for (int j = 0; j < J; j++)  // every load issued before the first use
      a[j] = hc[pack_item_texel<BLOCK>(local, j, n, logn, logb, lcw, x[j], y[j])];
    const CascadeFrame f = fp.c[c];
    float4* oc = rates + (size_t)c * 2 * nn;
#pragma unroll
    for (int j = 0; j < J; j++)
    {
      const KVec q = make_kvec(x[j], y[j], dim, f.dk);
      const float2 hd = evolve_rate(a[j], q.k, f);
      const CPair ph = pack_height(hd, q), pd = pack_displacement(hd, q);
      float4* out = oc + ((size_t)y[j] << logn) + x[j];
      out[0] = make_float4(ph.re.x, ph.im.x, ph.re.y, ph.im.y);
      out[nn] = make_float4(pd.re.x, pd.im.x, pd.re.y, pd.im.y);
    }
  }
}

}  // namespace oceanfft
