// device/k_half_rows.h — the half-spectrum row pass: rebuild the reference's four packed lanes
// from the kept half (Hermitian symmetry + the Nyquist-row term), x iFFT, maps and Jacobian
// (resources/spectrum.compute:246-259).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ocean_internal.h"
#include "device/evolve.h"
#include "device/fft.h"
#include "device/grid.h"
#include "device/memory.h"
#include "device/spectrum.h"
#include "device/k_half_cols.h"

namespace oceanfft
{

// Pass 2: one item = two rows (a 2T-thread workgroup), both images (image 0, then image 1). Element m
// of the x transform is column x = ((m + 8) & 15) T + i, u = x - N/2: m < 8 -> u = m T + i >= 0 (stored
// column u), m >= 8 -> u < 0. Every thread loads only its 8 direct elements (and thread 0 the Nyquist
// column for m = 8) and computes the lanes both at u (its own) and at -u, adding there the
// Nyquist-row term (-1)^y S(-u); the -u lanes go through LDS to the thread that holds -u: element
// 15 - m of thread T - i (thread 0: element 16 - m of itself). Each stored value is read once from
// HBM: C is loaded for image 0 and kept in VGPRs (16) for image 1. Then the x-iFFT, maps + Jacobian.
// Two rows per workgroup: 512-thread workgroups at 4096, two per CU, so one workgroup's loads overlap
// the other's transform (the LDS mirror exchange adds a barrier the 1024-thread, one-per-CU shape
// cannot hide: 1.92 -> 1.69 ms at 8 x 4096^2, tools/microbench/genbench).
// LA: the fields' load policy (whole grids: the default, so the gc lines shared by neighbouring items
// survive until the partner's read; streamed loads: -5 %).
// RM (row-major fields; RowSrc): element u in [0, N/2) of local row y of cascade c lies in source
// block u / cpr at ((c rows + y) lp + u % cpr), the Nyquist column u = -N/2 in block nyq_src at column
// cpr; the pass covers `rows` rows (a slab's w). The strip-dealt path (after k_half_to_rows) is one
// block [c][rows][N/2 + B]; the four-step path reads the exchange blocks of every source rank directly.
// cpr is a multiple of the 32 consecutive u one wave loads, so the block index is wave-uniform.
// RG / RGC / FB (whole grids): the field layout pass 1 wrote (half_group_offset; the column shape's).
template <int LOGN, int LA, bool RM, int RG = 1, int RGC = 1, int FB = 4>
__global__ __launch_bounds__(FftShape<LOGN>::T * 2) void k_rows_half(
    FrameParams fp, const float4* __restrict__ gab, const float4* __restrict__ gde, const float2* __restrict__ gc,
    const float4* __restrict__ spec, float4* __restrict__ maps, float* __restrict__ jac, FoamParams foam,
    const float2* __restrict__ tw_glob, int rows, RowSrc rs)
{
  using S = FftShape<LOGN>;
  using K = ColFirstCfg<LOGN>;
  using HC = HalfCfg<LOGN>;
  constexpr int N = S::N, T = S::T, B = K::B, RPW = 2, STRIPS = HC::STRIPS, WG = T * RPW;
  static_assert(WG <= 1024, "two rows per workgroup: N <= 8192");
  static_assert(WG * 8 * 16 <= lds_row_slots<LOGN>(RPW) * 8, "mirror exchange fits the transform's LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* tw = reinterpret_cast<float2*>(smem);
  void* xch = smem + ((S::TW_ENTRIES * 8 + 15) / 16) * 16;
  CPair* mir = reinterpret_cast<CPair*>(xch);  // [m < 8][thread]: lanes at -u for the partner
  load_twiddles<LOGN>(tw, tw_glob);

  const int blocks = (RM ? rows : N) / RPW;
  const int b0 = threadIdx.x % B, r0 = (threadIdx.x / B) % RPW, ihi0 = threadIdx.x / (B * RPW);
  // After the first exchange the two rows are interleaved (lanes: row fastest) and their LDS
  // regions (CI = 2, slot = 2 pa + row), so a wave's reads of 32 consecutive positions never straddle
  // a pad slot: conflict-free exchanges at 4096 (the row layout cost one extra cycle per 32-lane read
  // group, 262 K LDS cycles per CU per frame = SQ_LDS_BANK_CONFLICT; tools/lds_banks.py models both).
  // (A/B, halfbench rows: 1.449 -> 1.417 ms at 8 x 4096^2, 0.341 -> 0.335 at 2048; at 1024 the row
  // layout stays: 0.079 vs 0.083 ms).
  constexpr int CI = T >= 128 ? 2 : 0;
  const int i20 = CI ? (threadIdx.x / RPW) % T : threadIdx.x % T, r20 = CI ? threadIdx.x % RPW : threadIdx.x / T;
  const int total = fp.cascades * blocks;
  const float dim = (float)N;
  // C's row pairs are 64-B halves of 128-B lines; items 2p, 2p+1 (the same line) run together on one
  // XCD so the line is fetched once
  for (int item = xcd_pair_slot(blockIdx.x, gridDim.x); item < total; item += gridDim.x)
  {
    const int c = item / blocks, y0 = (item - c * blocks) * RPW;
    float2 ckeep[8];  // image 0's C loads, reused by image 1
    float2 cnyq;
#pragma unroll
    for (int img = 0; img < 2; img++)
    {
    const int cimg = c * 2 + img;
    const int b = opaque(b0), ihi = opaque(ihi0), r = opaque(r0);
    const int i = ihi * B + b;
    const float dk = fp.c[c].dk;
    // RM: the item's first row in every source block (texels); element (r, u) at r lp + u % cpr
    const size_t base = RM ? ((size_t)c * rows + y0) * rs.lp : (size_t)c * STRIPS * N * B;
    const int y = y0 + r;
    const float sgy = (y & 1) ? -1.0f : 1.0f;  // (-1)^q of the Nyquist-row term
    const float4* sp = spec + (size_t)cimg * N;
    const int tid = opaque((int)threadIdx.x);
    CPair v[16];
#pragma unroll
    for (int m = 0; m < 8; m++)
    {
      const int u = m * T + i;               // >= 0, column x = N/2 + u
      // source block (wave-uniform; cpr a power of two, launch_rm_rows): a shift, not a division
      const int src = RM ? __builtin_amdgcn_readfirstlane(u >> (31 - __builtin_clz(rs.cpr))) : 0;
      const int off = RM ? r * rs.lp + (u & (rs.cpr - 1)) : half_group_offset<LOGN, RG, FB>(y, u / FB, u % FB);
      const int offc = RM ? off : half_group_offset<LOGN, RGC, FB>(y, u / FB, u % FB);
      const float4* fab = RM ? reinterpret_cast<const float4*>(rs.ab + src * rs.src_stride) + base : gab + base;
      const float4* fde = RM ? reinterpret_cast<const float4*>(rs.de + src * rs.src_stride) + base : gde + base;
      const float2* fc = RM ? reinterpret_cast<const float2*>(rs.c + src * rs.src_stride) + base : gc + base;
      const float kx = (float)u * dk;        // ((float)x - N/2) dk, x - N/2 exact
      const float4 s4 = ld4<0>(sp, (N / 2 - u) * 16);  // the -u column's Nyquist-row term (x = N/2 - u)
      CPair own, neg;
      if (img == 0)
      {
        const CPair p = raw_pair(ld4<LA>(fab, off * 16));  // (A, B)
        const float2 cc = ld2<LA>(fc, offc * 8);             // C
        ckeep[m] = cc;
        const float Ar = p.re.x, Ai = p.im.x, Br = p.re.y, Bi = p.im.y, Cr = cc.x, Ci = cc.y;
        // at u: lane0 = (1 - kx) A, lane1 = i B - kx C
        own = CPair{f2v{(1.0f - kx) * Ar, -Bi - kx * Cr}, f2v{(1.0f - kx) * Ai, Br - kx * Ci}};
        // at -u (kx -> -kx, A -> conj A, B -> -conj B, C -> conj C): lane0 = (1 + kx) conj A,
        // lane1 = i (-conj B) + kx conj C
        neg = CPair{f2v{(1.0f + kx) * Ar + sgy * s4.x, -Bi + kx * Cr + sgy * s4.z},
                    f2v{-(1.0f + kx) * Ai + sgy * s4.y, -Br - kx * Ci + sgy * s4.w}};
      }
      else
      {
        const CPair q = raw_pair(ld4<LA>(fde, off * 16));  // (D, E)
        const float2 cc = ckeep[m];  // C
        const float Cr = cc.x, Ci = cc.y, Dr = q.re.x, Di = q.im.x, Er = q.re.y, Ei = q.im.y;
        const float kx2 = kx * kx;
        // at u: lane2 = i (D - kx^2 C), lane3 = -E - i kx D
        own = CPair{f2v{-(Di - kx2 * Ci), -Er + kx * Di}, f2v{Dr - kx2 * Cr, -Ei - kx * Dr}};
        // at -u (D -> -conj D, C -> conj C, E -> conj E, kx -> -kx): lane2 = i (-conj D - kx^2 conj C),
        // lane3 = -conj E + i kx (-conj D)
        neg = CPair{f2v{-(Di + kx2 * Ci) + sgy * s4.x, -Er - kx * Di + sgy * s4.z},
                    f2v{-Dr - kx2 * Cr + sgy * s4.y, Ei - kx * Dr + sgy * s4.w}};
      }
      v[m] = own;
      mir[m * WG + tid] = neg;
    }
    __syncthreads();
    // own elements m >= 8 (u < 0): from the partner's mirror slots; thread 0's m = 8 is the Nyquist
    // column (u = -N/2), read directly
    const int tp = i == 0 ? tid : tid + (((T - i) / B - ihi) * B * RPW) + ((T - i) % B - b);
#pragma unroll
    for (int m = 8; m < 16; m++)
    {
      if (i == 0 && m == 8)
      {
        // Nyquist column: first column of the last strip
        const int off = RM ? r * rs.lp + rs.cpr : half_group_offset<LOGN, RG, FB>(y, N / 2 / FB);
        const int offc = RM ? off : half_group_offset<LOGN, RGC, FB>(y, N / 2 / FB);
        const size_t ns = RM ? (size_t)rs.nyq_src * rs.src_stride : 0;
        const float4* fab = RM ? reinterpret_cast<const float4*>(rs.ab + ns) + base : gab + base;
        const float4* fde = RM ? reinterpret_cast<const float4*>(rs.de + ns) + base : gde + base;
        const float2* fc = RM ? reinterpret_cast<const float2*>(rs.c + ns) + base : gc + base;
        const float kx = -(dim / 2.0f) * dk;
        float2 cc;
        if (img == 1)
          cc = cnyq;
        else
          cc = ld2<LA>(fc, offc * 8);  // C
        if (img == 0)
          cnyq = cc;
        if (img == 0)
        {
          const CPair p = raw_pair(ld4<LA>(fab, off * 16));  // (A, B)
          v[m] = CPair{f2v{(1.0f - kx) * p.re.x, -p.im.y - kx * cc.x},
                       f2v{(1.0f - kx) * p.im.x, p.re.y - kx * cc.y}};
        }
        else
        {
          const CPair q = raw_pair(ld4<LA>(fde, off * 16));  // (D, E): D = (re.x, im.x)
          const float kx2 = kx * kx;
          v[m] = CPair{f2v{-(q.im.x - kx2 * cc.y), -q.re.y + kx * q.im.x},
                       f2v{q.re.x - kx2 * cc.x, -q.im.y - kx * q.re.x}};
        }
      }
      else
        v[m] = mir[(i == 0 ? 16 - m : 15 - m) * WG + tp];
    }
    __syncthreads();  // the transform's first exchange reuses the LDS
    const int i2 = opaque(i20), r2 = opaque(r20);
    fft_run<LOGN, CI, true>(v, i, r, i2, r2, xch, tw);
    float4* dst = maps + ((size_t)cimg * (RM ? rows : N) + y0) * N;
    const int woff = ((r2 << LOGN) + i2) * 16;
#pragma unroll
    for (int m = 0; m < 16; m++)
      st4<kStream>(dst + m * T, woff, from_pair(v[m]));
    if (img & 1)
    {
      // displacementMap (Dz, dDx/dx, dDz/dz, dDx/dz) = (re0, im0, re1, im1): Jacobian,
      // spectrum.compute:246-259
      const float lam = foam.displacement[c];
      float* jb = jac + ((size_t)c * (RM ? rows : N) + y0) * N;
      const int joff = ((r2 << LOGN) + i2) * 4;
#pragma unroll
      for (int m = 0; m < 16; m++)
        st1<kStream>(jb + m * T, joff,
                (1.0f + lam * v[m].im.x) * (1.0f + lam * v[m].re.y) - lam * lam * v[m].im.y * v[m].im.y);
    }
    }
  }
}

}  // namespace oceanfft
