// device/k_half_cols.h — the half-spectrum column pass (whole grids of 1024 .. 4096, and the
// strip-dealt slabs): evolve (resources/spectrum.compute:183-240) + the y iFFT of the five Hermitian
// field multiples of H.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ocean_internal.h"
#include "launch_common.h"
#include "device/evolve.h"
#include "device/fft.h"
#include "device/grid.h"
#include "device/memory.h"
#include "device/spectrum.h"

namespace oceanfft
{

// ------------------------------------------------------------------------------------------------
// Generator path, half spectrum (whole grids, B = 4, one strip per pass-1 item: N = 1024 .. 4096).
// All eight output fields are real multipliers of the one Hermitian field H (tests/
// half_spectrum_ref.py): lane0 = (1 - kx) A, lane1 = i B - kx C, lane2 = i (D - kx^2 C),
// lane3 = -E - i kx D with A = H, B = kz H, C = H/|k|, D = kz H/|k|, E = kz^2 H/|k|. The kx factors
// commute with the y transform, and H(-k) = conj(H(k)) makes each y-transformed field
// (anti-)Hermitian in u = x - N/2, so pass 1 transforms only the columns u >= 0 and the Nyquist
// column u = -N/2 (half the columns, half of h0 read), storing 5 complex fields (20 B per grid
// point instead of 32); pass 2 rebuilds u < 0 as s_F conj(G_F(q, -u)). The reference's Nyquist row
// is not Hermitian-paired (its partner is evaluated at +N/2, spectrum.compute:165); its share is the
// rank-1 term (-1)^q R(p), R the x-transform of a one-row spectrum built by k_half_nyquist.
// Frame bytes: h0 8 + fields 20 + 20 + maps 32 + Jacobian 4 = 84 per point (the full path: 116).
// ------------------------------------------------------------------------------------------------

template <int LOGN>
struct HalfCfg
{
  static constexpr int N = 1 << LOGN;
  static constexpr int B = ColFirstCfg<LOGN>::B;
  static constexpr int STRIPS = N / (2 * B) + 1;  // u in [0, N/2), then the strip of x = 0..B-1
  static constexpr bool SUPPORTED = B == 4 && ColFirstCfg<LOGN>::SPW == 1;  // blocked whole-grid path
  static constexpr bool SLAB_SUPPORTED = ColFirstCfg<LOGN>::SPW == 1;      // strip-dealt path, any B
};

// Whole-grid half-spectrum field layout, texel offset of (row y, strip, column b of the strip) in a
// cascade. RG = 1: strips [strip][y][B], a strip one contiguous run (pass 1 stores 1-KiB wave runs,
// pass 2 reads one RPW * B-texel piece per strip). RG > 1: row groups [y / RG][strip][y % RG][B], so a
// pass-2 item of RG rows reads one contiguous run and pass 1 stores RG * B-texel pieces. The offset is
// linear in (y, strip) for y a multiple of RG: offset(y0 + i, s, b) = offset(y0, s) + offset(i, 0, b).
// Whole strips: RG = 2, RGC = 4. A pass-2 item (2 rows) reads whole 128-B lines of gab/gde in one
// contiguous run per image, and gc's 128-B lines are shared by the two items paired on one XCD
// (xcd_pair_slot); pass 1 stores 128-B pieces. Against strips (RG = 1): pass 2 1.637 -> 1.506 ms,
// pass 1 0.934 -> 0.960 ms, frame 2.581 -> 2.477 ms at 8 x 4096^2 (tools/microbench/halfbench).
constexpr int kHalfRG = 2, kHalfRGC = 4;
constexpr int kHalfRG2 = 4, kHalfRGC2 = 8;  // the half-strip (FB = 2) layout's row groups: whole-line stores
// Pass 1's H pairs outside the scratch (k_cols_half HL / HK): one pair per thread in the LDS the
// exchange leaves free, four in VGPRs (128 VGPRs at N = 4096, no spills); the scratch keeps 3 of 8.
// 0.945 -> 0.817 ms per 8 x 4096^2, frame 2.332 -> 2.206 ms, fields bit-identical (halfbench hkeep).
constexpr int kHalfHL = 1, kHalfHK = 4, kHalfHKSeed = 2;
// FB: columns per field strip (4 = the h0 strip; 2 = half strips, FS = 2 STRIPS).
template <int LOGN, int RG, int FB = 4>
__device__ __forceinline__ int half_group_offset(int y, int strip, int b = 0)
{
  constexpr int N = HalfCfg<LOGN>::N, FS = HalfCfg<LOGN>::STRIPS * HalfCfg<LOGN>::B / FB;
  return RG == 1 ? (strip * N + y) * FB + b : (((y / RG) * FS + strip) * RG + (y % RG)) * FB + b;
}

// ------------------------------------------------------------------------------------------------
// The shapes k_cols_half is launched in. A shape is a type whose static members are the kernel's
// compile-time parameters:
//   LOGN      log2 N
//   LA        load policy of h0 (memory.h)
//   SLAB      strip-dealt layout (HalfSlab): this rank transforms global strips [strip0, strip0 +
//             nstrips) and writes its output in destination-block order into `send` (block q = rows
//             [q w, q w + w): gab | gde | gc parts of C * S * w * B elements, element ((c S + sl) w + yl)
//             B + b), so one equal-split all-to-all hands every rank the rows of its row pass. h0 is the
//             whole grid's blocked image when h0_full, else the rank's strips in order ([c][sl][N][B]).
//   SEED      the fused re-seed frame (CalculateOcean(dt, true) on whole grids): round 0 evaluates each
//             texel's two amplitudes (seed[c], the host's settings constants) instead of loading h0, so
//             h0 is neither written nor read this frame.
//   RG, RGC   whole grids: rows per group of the gab / gde and of the gc layout (half_group_offset)
//   CPI       columns per item: B (whole strips), or B / 2 (half strips: T * CPI threads, several
//             workgroups per CU so one's loads and stores overlap another's transform; the strip's two
//             halves are items 2p, 2p + 1 on one XCD)
//   HL, HK    of the thread's 8 H pairs, pairs [0, HL) live in the LDS left over by the exchange (16 B
//             per thread each) and pairs [HL, HL + HK) in VGPRs from round 0 to round 2; the rest goes
//             through the scratch, whose HBM traffic costs 0.118 of 0.912 ms at 8 x 4096^2
//   FB        whole grids: the field strips' width (half_group_offset<.., FB>). FB = CPI = 2: a half-strip
//             item's stores are whole lines when RG * FB * 16 B = 128 B (gab, gde) and RGC * FB * 8 B =
//             128 B (gc); the row pass reads the same layout
//   PUT       SLAB only (the one-sided exchange, ocean_peers): `send` is the device table of the ranks'
//             destinations, ((const uint64_t*)send)[q] = this rank's block in rank q's receive slot, and
//             block q is stored there instead of at send + q * block bytes
//   HB        h0's strip width. HB = CPI = 2 (half strips): h0 is blocked in 2-column strips, so an item
//             reads its own contiguous strip instead of the 32-B halves of 64-B row pieces that its
//             partner item reads the other halves of (0.122 -> 0.114 ms per 4096^2 cascade)
//   NYQ       whole grids: the Nyquist-row term (k_half_nyquist's spec, written to `send` as
//             float4[C][2][N]) is computed by the workgroup of the last item slot, which has the fewest
//             items, after them: one launch per frame fewer (half_nyquist_texel, the same arithmetic as
//             the kernel the slab paths use)
// ------------------------------------------------------------------------------------------------

// Whole grids, whole strips (three and more cascades per launch at 2048 / 4096, every count at 1024).
// The frame keeps kHalfHK pairs in VGPRs at 4096 and 2 below (128 VGPRs, so two (2048) or four (1024)
// workgroups share a CU) and streams h0 (nt), which leaves the XCD's L2 to the scratch.
template <int LOGN_, bool SEED_>
struct ColsWhole
{
  static constexpr int LOGN = LOGN_, LA = SEED_ ? 0 : kStream;
  static constexpr bool SLAB = false, SEED = SEED_, PUT = false, NYQ = true;
  static constexpr int RG = kHalfRG, RGC = kHalfRGC, FB = 4;
  static constexpr int CPI = ColFirstCfg<LOGN_>::B, HB = ColFirstCfg<LOGN_>::B;
  static constexpr int HL = kHalfHL, HK = SEED_ ? kHalfHKSeed : LOGN_ == 12 ? kHalfHK : 2;
};

// Whole grids of 2048 / 4096 with <= 2 cascades per launch: half strips into FB = 2 fields, 2T-thread
// workgroups (512 at 4096, two per CU with a 68-KiB exchange each; 256 at 2048, up to four per CU, two
// H pairs in VGPRs: with four, 8 B of spills). HB_ = 2: h0 in 2-column strips (half_h0_block); the
// re-seed frame does not read h0 and is built with HB_ = B only.
template <int LOGN_, bool SEED_, int HB_>
struct ColsHalfStrip
{
  static constexpr int LOGN = LOGN_, LA = SEED_ ? 0 : kStream;
  static constexpr bool SLAB = false, SEED = SEED_, PUT = false, NYQ = true;
  static constexpr int RG = kHalfRG2, RGC = kHalfRGC2, FB = 2;
  static constexpr int CPI = 2, HB = HB_;
  static constexpr int HL = kHalfHL, HK = SEED_ ? kHalfHKSeed : LOGN_ == 12 ? kHalfHK : 2;
};

// Strip-dealt slabs (1024 .. 16384). Slab items keep fewer pairs in VGPRs: with four, the SLAB store
// addressing spills 8-16 B (at N = 8192 already with two; one fits).
template <int LOGN_, bool PUT_>
struct ColsSlab
{
  static constexpr int LOGN = LOGN_, LA = kStream;
  static constexpr bool SLAB = true, SEED = false, PUT = PUT_, NYQ = false;
  static constexpr int RG = 1, RGC = 1, FB = 4;
  static constexpr int CPI = ColFirstCfg<LOGN_>::B, HB = ColFirstCfg<LOGN_>::B;
  static constexpr int HL = kHalfHL, HK = LOGN_ == 13 ? 1 : kHalfHK - 1;
};

// Launch geometry of a shape (launch_cols_half, below the kernel): workgroup size, dynamic LDS
// (twiddles | exchange | the HL pairs), work items, and how many workgroups `hs_blocks` scratch slices
// of 16 x 1024 entries (half_hs_bytes) serve: a workgroup uses 16 x WG entries. The slab launches keep
// one workgroup per slice at every size.
template <typename Sh>
struct ColsLaunch
{
  using S = FftShape<Sh::LOGN>;
  static constexpr int WG = S::T * Sh::CPI;
  static constexpr int LDS = ((S::TW_ENTRIES * 8 + 15) / 16) * 16 + Sh::CPI * S::PADDED * 8 + Sh::HL * WG * 16;
  static constexpr int items(int cascades, int nstrips) { return cascades * nstrips * (ColFirstCfg<Sh::LOGN>::B / Sh::CPI); }
  static constexpr int max_grid(int hs_blocks) { return Sh::SLAB ? hs_blocks : hs_blocks * (1024 / WG); }
};

// Pass 1: per strip of B columns (u >= 0, or the Nyquist strip), three y-iFFT rounds of CPairs:
// (A, B), (D, E), (C, 0), stored as gab, gde (float4) and gc (float2): pass 2 reads (A, B) + C for
// image 0 and C + (D, E) for image 1. Round 0 evolves H once; keeping all 16 H (32 VGPRs) next to the
// transform's ~107 spills in a 1024-thread workgroup, so H is kept as 8 pairs (H(m), H(m + 1)) per
// thread: HL in LDS, HK in VGPRs, the rest parked in a per-workgroup scratch slice (16-B entries,
// [m / 2][thread], L2/MALL-resident) that rounds 1 and 2 load back (nt: served by L2, never a stale L1
// line from the previous item) instead of re-reading h0 (16 B) and re-evolving.
template <typename Sh>
__global__ __launch_bounds__(ColsLaunch<Sh>::WG, Sh::CPI < ColFirstCfg<Sh::LOGN>::B ? 4 : 1) void k_cols_half(
    FrameParams fp, const float4* __restrict__ h0, float4* __restrict__ gab, float4* __restrict__ gde,
    float2* __restrict__ gc, const float2* __restrict__ tw_glob, float2* __restrict__ hs, HalfSlab hsl,
    unsigned char* __restrict__ send, int h0_full, const SpectrumConsts* __restrict__ seed)
{
  constexpr int LOGN = Sh::LOGN, LA = Sh::LA, RG = Sh::RG, RGC = Sh::RGC, CPI = Sh::CPI, HL = Sh::HL, HK = Sh::HK,
                FB = Sh::FB, HB = Sh::HB;
  constexpr bool SLAB = Sh::SLAB, SEED = Sh::SEED, PUT = Sh::PUT, NYQ = Sh::NYQ;
  using S = FftShape<LOGN>;
  using K = ColFirstCfg<LOGN>;
  using HC = HalfCfg<LOGN>;
  constexpr int N = S::N, T = S::T, B = K::B, STRIPS = HC::STRIPS, WG = T * CPI, HALVES = B / CPI;
  static_assert(SLAB ? HC::SLAB_SUPPORTED : HC::SUPPORTED, "half-spectrum path: one strip per item (B = 4 unless SLAB)");
  static_assert(CPI * HALVES == B && HALVES <= 2 && (HALVES == 1 || !SLAB), "whole or half strips");
  static_assert(HL >= 0 && HK >= 0 && HL + HK <= 8, "H pairs outside the scratch");
  static_assert(FB == 4 || (FB == CPI && HALVES == 2 && !SLAB && RG > 1 && RGC > 1), "FB: half-strip fields");
  static_assert(!PUT || SLAB, "PUT: the strip-dealt slab stores");
  static_assert(HB == B || (HB == CPI && HALVES == 2 && !SLAB), "HB: half strips over 2-column h0 strips");
  static_assert(!NYQ || !SLAB, "NYQ: whole grids (send is the spec output)");
  constexpr int XB = CPI * S::PADDED * 8;  // the exchange's bytes (K::LDS1 for whole strips)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* tw = reinterpret_cast<float2*>(smem);
  void* xch = smem + ((S::TW_ENTRIES * 8 + 15) / 16) * 16;
  float4* hlds = reinterpret_cast<float4*>(static_cast<unsigned char*>(xch) + XB);  // HL pairs [p][thread]
  load_twiddles<LOGN>(tw, tw_glob);

  const int nstrips = SLAB ? hsl.nstrips : STRIPS;
  const int total = fp.cascades * nstrips * HALVES;
  const float dim = (float)N;
  for (int item = HALVES > 1 ? xcd_pair_slot(blockIdx.x, gridDim.x) : (int)blockIdx.x; item < total; item += gridDim.x)
  {
    const int hh = HALVES > 1 ? item % HALVES : 0, si = HALVES > 1 ? item / HALVES : item;
    const int c = si / nstrips, s = si - c * nstrips;  // s: the rank's strip index
    const int sg = SLAB ? hsl.strip0 + s : s;           // global strip
    if (HALVES > 1 && sg == STRIPS - 1 && hh != 0)
      continue;  // Nyquist strip: only column 0 (u = -N/2) is kept (uniform per workgroup)
    const int b = opaque((int)threadIdx.x) % CPI + hh * CPI;  // column within the strip
    const int xb = sg == STRIPS - 1 ? 0 : N / (2 * B) + sg;
    const CascadeFrame f = fp.c[c];
    const float4* src = HB != B                  ? h0 + ((size_t)c * (N / HB) + xb * (B / HB) + hh) * N * HB
                        : (!SLAB || h0_full) ? h0 + ((size_t)c * (N / B) + xb) * N * B
                                             : h0 + ((size_t)c * nstrips + s) * N * B;
    // the strip's first texel in the cascade's fields (whole grids); + half_group_offset(m T, 0) per m
    const int fs = FB == 4 ? s : 2 * s + hh;  // field strip
    const size_t gbase = RG == 1 ? ((size_t)c * STRIPS + s) * N * B
                                 : (size_t)c * STRIPS * N * B + half_group_offset<LOGN, RG, FB>(0, fs);
    const size_t cgbase = RGC == 1 ? ((size_t)c * STRIPS + s) * N * B
                                   : (size_t)c * STRIPS * N * B + half_group_offset<LOGN, RGC, FB>(0, fs);
    const int bf = FB == 4 ? b : b - hh * CPI;  // column within the field strip
    const int x = xb * B + b;
    float4 hk[HK > 0 ? HK : 1];  // HK: H pairs kept in VGPRs across the rounds
    // one field round: (A, B), (D, E) or (C, 0) of the 16 texels, y-iFFT, store
    auto run_round = [&](int round) __attribute__((always_inline)) {
      const int i = (opaque((int)threadIdx.x) / CPI) % T;
      const int voff = (i * B + b) * 16;
      CPair v[16];
      auto pack = [&](int m, float2 H, const KVec& q) __attribute__((always_inline)) {
        if (round == 0)  // (A, B) = (H, kz H)
          v[m] = CPair{f2v{H.x, q.kz * H.x}, f2v{H.y, q.kz * H.y}};
        else if (round == 1)  // (D, E) = (kz H / |k|, kz^2 H / |k|)
        {
          const float e = q.kz * q.dirz;
          v[m] = CPair{f2v{q.dirz * H.x, e * H.x}, f2v{q.dirz * H.y, e * H.y}};
        }
        else  // (C, 0) = (H / |k|, 0)
          v[m] = CPair{f2v{q.inv * H.x, 0.0f}, f2v{q.inv * H.y, 0.0f}};
      };
      if (SEED && round == 0)
      {
        float2* hsb = hs + (size_t)blockIdx.x * 16 * WG;
        const int hoff = opaque((int)threadIdx.x) * 8;
        const SpectrumConsts q = seed[c];
        // the evaluator is too large to unroll 16 times: a rolled loop parks each H in the scratch,
        // then the round reads them back like rounds 1 and 2 (its own stores, from L2)
#pragma unroll 1
        for (int m = 0; m < 16; m++)
        {
          const int y = i + ((m + 8) & 15) * T;
          const float2 H = evolve(seed_texel(q, x, y, dim), make_kvec(x, y, dim, f.dk).k, f);
          if ((m >> 1) < HL)  // HL pairs: the LDS slot (a dynamic index is fine there)
            reinterpret_cast<float2*>(hlds)[((m >> 1) * WG + threadIdx.x) * 2 + (m & 1)] = H;
          else
            st2s<0>(hsb, hoff * 2 + (m & 1) * 8, (m >> 1) * WG * 16, H);
        }
        __threadfence_block();  // this thread's scratch stores are complete before it reads them back
        // read back by pairs; the HK pairs stay in VGPRs for rounds 1 and 2
#pragma unroll
        for (int m = 0; m < 16; m += 2)
        {
          const int y = i + ((m + 8) & 15) * T, p = m >> 1;
          const float4 pp = p < HL ? hlds[p * WG + threadIdx.x] : ld4s<kStream>(hsb, hoff * 2, p * WG * 16);
          if (p >= HL && p < HL + HK)
            hk[p < HL + HK && p >= HL ? p - HL : 0] = pp;
          pack(m, make_float2(pp.x, pp.y), make_kvec(x, y, dim, f.dk));
          pack(m + 1, make_float2(pp.z, pp.w), make_kvec(x, y + T, dim, f.dk));
        }
      }
      else if (round == 0)
      {
        float2* hsb = hs + (size_t)blockIdx.x * 16 * WG;
        const int hoff = opaque((int)threadIdx.x) * 8;
        float4 a[16];
        float2 hprev = make_float2(0.0f, 0.0f);
        // HB = 2: the half strip's own 2-column h0 strip (contiguous 32-B row pieces)
        const int loff = HB == B ? voff : (i * HB + (b - hh * CPI)) * 16;
#pragma unroll
        for (int m = 0; m < 16; m++)  // fftShift on y folded into the load
          a[m] = ld4s<LA>(src, loff, ((m + 8) & 15) * T * HB * 16);
#pragma unroll
        for (int m = 0; m < 16; m++)
        {
          const int y = i + ((m + 8) & 15) * T;
          const KVec q = make_kvec(x, y, dim, f.dk);
          const float2 H = evolve(a[m], q.k, f);
          const int p = m >> 1;
          if ((m & 1) && p < HL)
            hlds[p * WG + threadIdx.x] = make_float4(hprev.x, hprev.y, H.x, H.y);
          else if ((m & 1) && p < HL + HK)
            hk[p - HL] = make_float4(hprev.x, hprev.y, H.x, H.y);
          else if (m & 1)
            st4s<0>(hsb, hoff * 2, p * WG * 16, make_float4(hprev.x, hprev.y, H.x, H.y));
          else
            hprev = H;
          pack(m, H, q);
        }
      }
      else
      {
        const float2* hsb = hs + (size_t)blockIdx.x * 16 * WG;
        const int hoff = opaque((int)threadIdx.x) * 8;
#pragma unroll
        for (int m = 0; m < 16; m += 2)
        {
          const int y = i + ((m + 8) & 15) * T, pi = m >> 1;
          const float4 p = pi < HL        ? hlds[pi * WG + threadIdx.x]
                           : pi < HL + HK ? hk[pi < HL + HK ? pi - HL : 0]
                                          : ld4s<kStream>(hsb, hoff * 2, pi * WG * 16);
          pack(m, make_float2(p.x, p.y), make_kvec(x, y, dim, f.dk));
          pack(m + 1, make_float2(p.z, p.w), make_kvec(x, y + T, dim, f.dk));
        }
      }
      const int reg = HALVES > 1 ? opaque((int)threadIdx.x) % CPI : b;
      fft_run<LOGN, CPI, true>(v, i, reg, xch, tw);
      const int vo = (i * B + b) * 16;  // the thread's output rows i + m T
#pragma unroll
      for (int m = 0; m < 16; m++)
      {
        if constexpr (SLAB)
        {
          // row y = m T + i lies in block q = m T / w (w is a multiple of T), at yl = m T % w + i
          const size_t part = (size_t)fp.cascades * hsl.S * hsl.w * B;  // elements per part
          const int q = (m * T) / hsl.w, yl0 = (m * T) % hsl.w;
          const size_t el = (((size_t)c * hsl.S + s) * hsl.w + yl0) * B;
          // block = the three parts, then the Nyquist-row term [c][2][N] (half_slab_block_bytes).
          // The block base is built at its store (sopaque): hoisted, the 16 descriptors spilled SGPRs.
          unsigned char* blk =
              PUT ? reinterpret_cast<unsigned char*>(sopaque((size_t)reinterpret_cast<const uint64_t*>(send)[q]))
                  : send + sopaque((size_t)q * (part * 40 + (size_t)fp.cascades * 2 * N * 16));
          if (round == 0)
            st4<kStream>(blk + el * 16, vo, pair_raw(v[m]));
          else if (round == 1)
            st4<kStream>(blk + part * 16 + el * 16, vo, pair_raw(v[m]));
          else
            st2<kStream>(blk + part * 32 + el * 8, (i * B + b) * 8, make_float2(v[m].re.x, v[m].im.x));
        }
        else if constexpr (RG == 1 && RGC == 1)
        {
          if (round == 0)
            st4s<kStream>(gab + gbase, vo, m * T * B * 16, pair_raw(v[m]));
          else if (round == 1)
            st4s<kStream>(gde + gbase, vo, m * T * B * 16, pair_raw(v[m]));
          else
            st2s<kStream>(gc + gbase, (i * B + b) * 8, m * T * B * 8, make_float2(v[m].re.x, v[m].im.x));
        }
        else if (round == 0)  // one descriptor per field; the row group of m T in soffset
          st4s<kStream>(gab + gbase, half_group_offset<LOGN, RG, FB>(i, 0, bf) * 16, half_group_offset<LOGN, RG, FB>(m * T, 0) * 16,
                        pair_raw(v[m]));
        else if (round == 1)
          st4s<kStream>(gde + gbase, half_group_offset<LOGN, RG, FB>(i, 0, bf) * 16, half_group_offset<LOGN, RG, FB>(m * T, 0) * 16,
                        pair_raw(v[m]));
        else
          st2s<kStream>(gc + cgbase, half_group_offset<LOGN, RGC, FB>(i, 0, bf) * 8, half_group_offset<LOGN, RGC, FB>(m * T, 0) * 8,
                        make_float2(v[m].re.x, v[m].im.x));
      }
    };
#pragma unroll
    for (int round = 0; round < 3; round++)  // specialised per round
      run_round(round);
  }
  if constexpr (NYQ)
    if ((HALVES > 1 ? xcd_pair_slot(blockIdx.x, gridDim.x) : (int)blockIdx.x) == (int)gridDim.x - 1)
      for (int idx = threadIdx.x; idx < fp.cascades * N; idx += WG)
        half_nyquist_texel(fp, N, HB, h0, reinterpret_cast<float4*>(send), nullptr, 1, 0, seed, nullptr, 0, idx);
}

// Launch a shape over `nstrips` strips per cascade: persistent_grid's grid, capped by the scratch slices.
template <typename Sh>
hipError_t launch_cols_half(const FrameParams& fp, int nstrips, const float4* h0, float4* gab, float4* gde, float2* gc,
                            const float2* tw, float2* hs, int hs_blocks, const HalfSlab& hsl, unsigned char* send,
                            int h0_full, const SpectrumConsts* seed, hipStream_t stream, int cus)
{
  using G = ColsLaunch<Sh>;
  auto kern = k_cols_half<Sh>;
  int grid = persistent_grid(kern, G::WG, G::LDS, G::items(fp.cascades, nstrips), cus);
  if (grid > G::max_grid(hs_blocks))
    grid = G::max_grid(hs_blocks);
  if (grid < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(G::WG), G::LDS, stream, fp, h0, gab, gde, gc, tw, hs, hsl, send, h0_full, seed);
  return hipGetLastError();
}

}  // namespace oceanfft
