// launch_half.hip — the half-spectrum generator frame of whole grids, N = 1024 .. 4096 (84 B per
// point): k_cols_half (evolve + y iFFT of the five field multiples of H over the kept
// columns) and k_rows_half (Hermitian rebuild + x iFFT + maps + Jacobian). Kernels:
// device/k_half_cols.h, device/k_half_rows.h. The A/B variants measured against these live in
// tools/microbench/ab_kernels.h, outside the library.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "oceanfft.h"
#include "ocean_internal.h"
#include "launch_common.h"
#include "device/grid.h"
#include "device/k_half_cols.h"
#include "device/k_half_rows.h"
#include "device/k_rows_hp.h"
#include "device/spectrum.h"

namespace oceanfft
{

bool half_spectrum_supported(int logn) { return logn >= 10 && logn <= 12; }

// Whole grids of 2048 / 4096 with <= 2 cascades per launch (the 4- and 8-GPU shares of the headline)
// run pass 1 on half strips into field strips FB = 2 columns wide (ColsHalfStrip), the row pass on that
// layout. Same per-column arithmetic as the 4-column strips, so the maps are bit-identical to them. At
// 4096 one cascade takes 0.319 against 0.339 ms, two 0.597 against 0.609, three and more lose
// (profiles/r04_halfbench_fb2h_{1,2,3,4,8}.log). At 2048 with one cascade the whole-strip pass has 257
// items for 256 CUs, and the CU that runs two sets the pass's time (0.0577 ms against 0.0345 with 256
// items, profiles/r06_halfbench_tail_11.log); the 513 half-strip items fit the 1024 slots at once:
// column pass 0.0431 -> 0.0311 ms, frame 0.0945 -> 0.0862 ms, at two cascades 0.1642 -> 0.1621 ms, at
// four it loses (0.2960 -> 0.3322), maps bit-identical (profiles/r06_halfbench_h2k_{1,2,4}.log).
constexpr bool half_strip_launch(int logn, int cascades) { return (logn == 12 || logn == 11) && cascades <= 2; }

// The column pass of one launch: visit(shape) with the k_cols_half shape for (N, cascades, re-seed
// frame?, h0's strip width). h0_blk = 0 asks for the width the pass reads best (half_h0_block).
// launch_half_columns launches the visited shape and ocean_frame_plan reports its members.
template <int LOGN, typename V>
hipError_t select_half_cols(int cascades, bool seed, int h0_blk, V&& visit)
{
  constexpr int B = ColFirstCfg<LOGN>::B;
  if constexpr (LOGN == 12 || LOGN == 11)
    if (half_strip_launch(LOGN, cascades))
    {
      if (h0_blk != 0 && h0_blk != 2 && h0_blk != B)
        return hipErrorInvalidValue;
      if (seed)  // h0 is not read
        return visit(ColsHalfStrip<LOGN, true, B>{});
      return h0_blk == B ? visit(ColsHalfStrip<LOGN, false, B>{}) : visit(ColsHalfStrip<LOGN, false, 2>{});
    }
  if (h0_blk != 0 && h0_blk != B)
    return hipErrorInvalidValue;  // 2-column h0 strips are read by the half-strip pass only
  return seed ? visit(ColsWhole<LOGN, true>{}) : visit(ColsWhole<LOGN, false>{});
}

// The row pass's shapes: the field layout it reads (FB, RG, RGC; the column shape's) and its kernel.
// RowsHp: k_rows_hp (4096), GRP rows per XCD group, EARLY / MINB as the kernel's. Whole strips: three
// workgroups per CU with image 1's (D, E) loads issued before image 0's stores (EARLY 1, MINB 3):
// 1.362 / 1.366 -> 1.345 / 1.351 ms per 8 x 4096^2 on two boxes, maps bit-identical
// (profiles/r05_halfbench_hpe2_8.log, r05_halfbench_hpe3_8.log).
template <int FB_, int RG_, int RGC_, int GRP_, int EARLY_, int MINB_>
struct RowsHp
{
  static constexpr bool HP = true;
  static constexpr int FB = FB_, RG = RG_, RGC = RGC_, GRP = GRP_, EARLY = EARLY_, MINB = MINB_;
};
// RowsHalf: k_rows_half (below 4096), default-policy loads.
template <int FB_, int RG_, int RGC_>
struct RowsHalf
{
  static constexpr bool HP = false;
  static constexpr int FB = FB_, RG = RG_, RGC = RGC_;
};

// The row pass of one launch: visit(shape) for (N, cascades). launch_half_rows launches the visited
// shape and ocean_frame_plan reports its members.
template <int LOGN, typename V>
hipError_t select_half_rows(int cascades, V&& visit)
{
  const bool hs = half_strip_launch(LOGN, cascades);
  if constexpr (LOGN == 12)
    return hs ? visit(RowsHp<2, kHalfRG2, kHalfRGC2, kHalfRGC2, 0, 4>{}) : visit(RowsHp<4, kHalfRG, kHalfRGC, 4, 1, 3>{});
  else if constexpr (LOGN == 11)
    return hs ? visit(RowsHalf<2, kHalfRG2, kHalfRGC2>{}) : visit(RowsHalf<4, kHalfRG, kHalfRGC>{});
  else
    return visit(RowsHalf<4, kHalfRG, kHalfRGC>{});
}

int half_h0_block(int logn, int cascades)
{
  int hb = spectrum_block(logn);
  (void)with_logn(logn, [&](auto L) -> hipError_t {
    constexpr int LOGN = decltype(L)::value;
    if constexpr (HalfCfg<LOGN>::SUPPORTED)
      return select_half_cols<LOGN>(cascades, false, 0, [&](auto sh) {
        hb = decltype(sh)::HB;
        return hipSuccess;
      });
    else
      return hipSuccess;
  });
  return hb;
}

size_t half_field_texels(int logn)
{
  const size_t n = (size_t)1 << logn;
  return (n / 8 + 1) * n * 4;  // HalfCfg: STRIPS * N * B per cascade (B = 4)
}

size_t half_hs_bytes(int logn, int blocks)
{
  return half_slab_supported(logn) ? (size_t)blocks * 16 * 1024 * sizeof(float2) : 0;  // WG1 <= 1024
}

hipError_t launch_half_columns(int logn, const FrameParams& fp, const float4* h0, float4* gab, float4* gcd, float2* ge,
                               float4* spec, const float2* tw, hipStream_t stream, int cus, float2* hs, int hs_blocks,
                               const void* seed_consts, int h0_blk)
{
  if (!hs)  // the H scratch (half_hs_bytes): H evolved once per item instead of once per field round
    return hipErrorInvalidValue;
  const SpectrumConsts* seed = static_cast<const SpectrumConsts*>(seed_consts);
  return with_logn(logn, [&](auto L) -> hipError_t {
    constexpr int LOGN = decltype(L)::value;
    if constexpr (!HalfCfg<LOGN>::SUPPORTED)
      return hipErrorInvalidValue;
    else
      // gcd / ge: the (D, E) and C fields. The Nyquist-row term (one row spectrum per image) is written
      // by pass 1 itself (NYQ), into `spec` passed as the kernel's `send`.
      return select_half_cols<LOGN>(fp.cascades, seed != nullptr, h0_blk > 0 ? h0_blk : ColFirstCfg<LOGN>::B, [&](auto sh) {
        return launch_cols_half<decltype(sh)>(fp, HalfCfg<LOGN>::STRIPS, h0, gab, gcd, ge, tw, hs, hs_blocks, HalfSlab{},
                                              reinterpret_cast<unsigned char*>(spec), 1, seed, stream, cus);
      });
  });
}

hipError_t launch_half_rows(int logn, const FrameParams& fp, const float4* gab, const float4* gcd, const float2* ge,
                            const float4* rcorr, float4* maps, float* jac, const FoamParams& foam, const float2* tw,
                            hipStream_t stream, int cus)
{
  return with_logn(logn, [&](auto L) -> hipError_t {
    constexpr int LOGN = decltype(L)::value;
    if constexpr (!HalfCfg<LOGN>::SUPPORTED)
      return hipErrorInvalidValue;
    else
      return select_half_rows<LOGN>(fp.cascades, [&](auto sh) {
        using R = decltype(sh);
        using S = FftShape<LOGN>;
        if constexpr (R::HP)
        {
          auto kern = k_rows_hp<R::RG, R::RGC, false, R::FB, R::GRP, R::EARLY, R::MINB>;
          const int grid = persistent_grid(kern, 256, HpCfg::LDS, fp.cascades * S::N, cus);
          hipLaunchKernelGGL(kern, dim3(grid), dim3(256), HpCfg::LDS, stream, fp, gab, gcd, ge, rcorr, maps, jac, foam, tw, 0,
                             RowSrc{});
        }
        else
        {
          auto kern = k_rows_half<LOGN, 0, false, R::RG, R::RGC, R::FB>;
          const int lds = ((S::TW_ENTRIES * 8 + 15) / 16) * 16 + lds_row_slots<LOGN>(2) * 8;
          const int grid = persistent_grid(kern, S::T * 2, lds, fp.cascades * (S::N / 2), cus);
          hipLaunchKernelGGL(kern, dim3(grid), dim3(S::T * 2), lds, stream, fp, gab, gcd, ge, rcorr, maps, jac, foam, tw, S::N,
                             RowSrc{});
        }
        return hipGetLastError();
      });
  });
}

}  // namespace oceanfft

// The pairing table (include/oceanfft.h ocean_frame_plan): host only, no device needed. Both halves are
// read from the shape types the launchers instantiate their kernels from.
extern "C" int ocean_frame_plan(size_t texture_size, int cascades, int32_t out[8])
{
  using namespace oceanfft;
  int logn = 0;
  while (logn < 15 && ((size_t)1 << logn) < texture_size)
    logn++;
  if (!out || ((size_t)1 << logn) != texture_size || !half_spectrum_supported(logn) || cascades < 1 ||
      cascades > kMaxCascades)
    return OCEAN_ERR_INVALID;
  const hipError_t e = with_logn(logn, [&](auto L) -> hipError_t {
    constexpr int LOGN = decltype(L)::value;
    if constexpr (!HalfCfg<LOGN>::SUPPORTED)
      return hipErrorInvalidValue;
    else
    {
      const hipError_t ec = select_half_cols<LOGN>(cascades, false, 0, [&](auto sh) {
        using C = decltype(sh);
        out[0] = C::FB, out[1] = C::RG, out[2] = C::RGC, out[3] = C::HB;
        return hipSuccess;
      });
      const hipError_t er = select_half_rows<LOGN>(cascades, [&](auto sh) {
        using R = decltype(sh);
        out[4] = R::FB, out[5] = R::RG, out[6] = R::RGC;
        return hipSuccess;
      });
      return ec != hipSuccess ? ec : er;
    }
  });
  if (e != hipSuccess)
    return OCEAN_ERR_INVALID;
  out[7] = half_h0_block(logn, cascades);
  return OCEAN_OK;
}
