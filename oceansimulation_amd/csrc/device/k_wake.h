// device/k_wake.h — the wake windows (ocean_wake, include/oceanfft.h): a square height field h in base-point
// space, forced by the vertical loads of hull points and stepped with Tessendorf's local deep-water operator,
//     h_tt = -(g / dx) G * (h + P),
// G a 13 x 13 convolution whose symbol approximates |k|. All arithmetic is unfused fp32 in the order the
// header writes it; the scatter is integer, so a call replays bit for bit.
//
// k_wake_splat: a lane per record, an item is kWakeThreads records. The record's head m = F.y * inv is spread
// over the four texels around its base point with bilinear weights, each tap as a no-return agent-scope 64-bit
// integer add of (int64)(clamp(m w) * 2^20) into the texel's accumulator (a tap of 0 units issues nothing).
// With CLEAR the same lanes visit the same taps after the last substep and store 0, so the accumulators are
// zero again at a cost that scales with the records, not with the window.
//
// k_wake_substep: an item is a kWakeTile x kWakeTile tile of outputs. The workgroup stages e = h + P of the
// tile and its 6-texel halo in LDS once (44 x 44 values; zeros outside the window), then a lane produces four
// outputs in a row from registers: for every row distance a = 0..6 it reads the two rows j + a and j - a of its
// 16-wide window (13 + 4 - 1) with four ds_read_b128 each, so one LDS read of 16 B feeds 13 taps (52 reads per
// lane for 4 x 169 taps). The contract sums T[a][b] S(a, b) for a = 0..6, b = 0..a with S the eight-fold (four-fold on the axes and the
// diagonal) symmetric sum; with Q(c, d) = (e[i+c, j+d] + e[i-c, j-d]) + (e[i+c, j-d] + e[i-c, j+d]),
// S(a, b) = Q(a, b) + Q(b, a) for 0 < b < a and S(a, a) = Q(a, a). Q(c, d) needs only the rows j +- d, so at row
// distance a the lane forms Q(b, a), b <= a, adds the terms of a in order, and keeps Q(c, a), c > a, for the
// later distances: 15 values per output, 60 registers, beside the row 0 window and the two current rows.
// LDS: a lane's window starts at float 4 * lx of its rows, 16-B aligned; lanes are 8 across x 8 rows per wave.
// ds_read_b128 serves four groups of 16 lanes ({0-3, 12-15, 20-27}, ..): with the row pitch 96 floats (24
// slots of 16 B, 8 mod 16) the four rows of a group start 8 slots apart, and its lanes read 16 distinct slots of
// the 16 of a bank row: conflict free. 44 rows x 96 floats = 16896 B per workgroup.
//
// k_wake_shift: both maps moved by whole texels through the accumulators' storage (8 B per texel: two floats).
// k_wake_sample: a lane per point, bilinear h, its gradient and (h - h_prev) / hs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kWakeSpan = kWakeTile + 2 * kWakeRadius;  // 44: the staged rows and columns
constexpr int kWakePitch = 96;                          // floats per staged row (see above)
constexpr int kWakeRun = 4;                             // outputs per lane, along x
constexpr float kWakeUnits = 1048576.0f;                // 2^20

__host__ __device__ constexpr int wake_tap(int a, int b) { return a * (a + 1) / 2 + b; }            // b <= a
__host__ __device__ constexpr int wake_kept(int c, int d) { return (c - 1) * (c - 2) / 2 + d - 1; }  // 1 <= d < c

// n = min(*count_device, max_records), not below 0
__device__ __forceinline__ int64_t wake_records(const WakeCall& s)
{
  int64_t n = s.max_records;
  if (s.count_device)
  {
    const int64_t c = *s.count_device;
    n = c < n ? c : n;
  }
  return n < 0 ? 0 : n;
}

// grid: at most kWakeSplatMaxGrid, item loop
template <bool CLEAR>
__global__ __launch_bounds__(kWakeThreads) void k_wake_splat(WakeCall s)
{
#pragma clang fp contract(off)
  const int64_t n = wake_records(s);
  const int64_t items = (n + kWakeThreads - 1) / kWakeThreads;
  const float fm = (float)s.m;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int64_t r = item * kWakeThreads + threadIdx.x;
    if (r >= n)
      continue;
    const float* rec = s.records + 8 * r;
    const float m = rec[5] * s.inv;
    const float u = (rec[0] - s.ox) / s.dx, v = (rec[2] - s.oz) / s.dx;
    if (!(u >= -1.0f && u < fm && v >= -1.0f && v < fm))  // a NaN culls
      continue;
    const float fi = floorf(u), fj = floorf(v);
    const float fx = u - fi, fz = v - fj;
    const int i0 = (int)fi, j0 = (int)fj;
    const float w[4] = {(1.0f - fx) * (1.0f - fz), fx * (1.0f - fz), (1.0f - fx) * fz, fx * fz};
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
      const int i = i0 + (k & 1), j = j0 + (k >> 1);
      if (i < 0 || i >= s.m || j < 0 || j >= s.m)
        continue;
      long long* a = s.acc + ((size_t)j * s.m + i);
      if constexpr (CLEAR)
        *a = 0;
      else
      {
        const float p = m * w[k];
        const float q = p == p ? fminf(fmaxf(p, -kWakeUnits), kWakeUnits) : 0.0f;
        const long long units = (long long)(q * kWakeUnits);  // |q * 2^20| <= 2^40; truncates toward zero
        if (units != 0)
          (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a), (unsigned long long)units,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// Q(c, d) of the header comment for output x of the window rows rp = j + d, rm = j - d
__device__ __forceinline__ float wake_quad(const float (&rp)[16], const float (&rm)[16], int x, int c)
{
#pragma clang fp contract(off)
  return (rp[x + c] + rm[x - c]) + (rm[x + c] + rp[x - c]);
}

__device__ __forceinline__ void wake_row(const float* e, int row, int lx, float (&w)[16])
{
  const float4* p = reinterpret_cast<const float4*>(e + row * kWakePitch + kWakeRun * lx);
#pragma unroll
  for (int k = 0; k < 4; k++)
  {
    const float4 v = p[k];
    w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
  }
}

// grid: persistent_grid over ceil(m / 32)^2 tiles, item loop. FORCED: the call has records, P is read.
template <bool FORCED>
__global__ __launch_bounds__(kWakeThreads) void k_wake_substep(WakeCall s)
{
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float e[kWakeSpan * kWakePitch];
  const int tid = threadIdx.x;
  const int lx = tid & 7, ly = tid >> 3;  // 8 lanes x 4 outputs across, 32 rows
  const int m = s.m;
  const int tiles = (m + kWakeTile - 1) / kWakeTile;
  const float fborder = (float)s.border;
  for (int item = blockIdx.x; item < tiles * tiles; item += gridDim.x)
  {
    const int ty = item / tiles, tx = item - ty * tiles;
    const int x0 = tx * kWakeTile, y0 = ty * kWakeTile;
    for (int idx = tid; idx < kWakeSpan * kWakeSpan; idx += kWakeThreads)
    {
      const int r = idx / kWakeSpan, c = idx - r * kWakeSpan;
      const int gi = x0 - kWakeRadius + c, gj = y0 - kWakeRadius + r;
      float v = 0.0f;
      if ((unsigned)gi < (unsigned)m && (unsigned)gj < (unsigned)m)
      {
        const size_t t = (size_t)gj * m + gi;
        float p = 0.0f;
        if constexpr (FORCED)
          p = (float)s.acc[t] * 0x1p-20f;
        v = s.h[t] + p;
      }
      e[r * kWakePitch + c] = v;
    }
    __syncthreads();
    const int i = x0 + kWakeRun * lx, j = y0 + ly;
    if (i < m && j < m)  // m is a multiple of 16: a lane's run is inside or outside as a whole
    {
      float w0[16], rp[16], rm[16], acc[kWakeRun], kept[kWakeRun][15];
      wake_row(e, ly + kWakeRadius, lx, w0);
#pragma unroll
      for (int o = 0; o < kWakeRun; o++)
        acc[o] = 0.0f + s.taps[0] * w0[kWakeRadius + o];
#pragma unroll
      for (int a = 1; a <= kWakeRadius; a++)
      {
        wake_row(e, ly + kWakeRadius + a, lx, rp);
        wake_row(e, ly + kWakeRadius - a, lx, rm);
#pragma unroll
        for (int o = 0; o < kWakeRun; o++)
        {
          const int x = kWakeRadius + o;
          acc[o] = acc[o] + s.taps[wake_tap(a, 0)] * ((w0[x + a] + w0[x - a]) + (rp[x] + rm[x]));
#pragma unroll
          for (int b = 1; b < a; b++)
            acc[o] = acc[o] + s.taps[wake_tap(a, b)] * (kept[o][wake_kept(a, b)] + wake_quad(rp, rm, x, b));
          acc[o] = acc[o] + s.taps[wake_tap(a, a)] * wake_quad(rp, rm, x, a);
#pragma unroll
          for (int c = a + 1; c <= kWakeRadius; c++)
            kept[o][wake_kept(c, a)] = wake_quad(rp, rm, x, c);
        }
      }
      const size_t t = (size_t)j * m + i;
      const float4 h4 = *reinterpret_cast<const float4*>(s.h + t);
      const float4 p4 = *reinterpret_cast<const float4*>(s.h_prev + t);
      const float hv[kWakeRun] = {h4.x, h4.y, h4.z, h4.w}, pv[kWakeRun] = {p4.x, p4.y, p4.z, p4.w};
      float out[kWakeRun];
      const int dj = min(j, m - 1 - j);
#pragma unroll
      for (int o = 0; o < kWakeRun; o++)
      {
        const int ii = i + o;
        const float d = (float)min(min(ii, m - 1 - ii), dj);
        const float r = s.border > 0 ? fmaxf(fborder - d, 0.0f) / fborder : 0.0f;
        const float alpha = s.damp + s.edge_damp * (r * r);
        const float b = s.hb * alpha;
        out[o] = (((2.0f * hv[o]) - (1.0f - b) * pv[o]) - s.c * acc[o]) / (1.0f + b);
      }
      *reinterpret_cast<float4*>(s.h_prev + t) = make_float4(out[0], out[1], out[2], out[3]);
    }
    __syncthreads();  // the next item's fill overwrites e
  }
}

// grid: one thread per texel, stride loop. PHASE 0: tmp = the shifted maps (tmp: the accumulators' storage, two
// float maps); PHASE 1: the maps = tmp. The launcher zeroes the accumulators afterwards.
template <int PHASE>
__global__ __launch_bounds__(kWakeThreads) void k_wake_shift(WakeCall s, int di, int dj)
{
  const int64_t mm = (int64_t)s.m * s.m;
  float* tmp = reinterpret_cast<float*>(s.acc);
  for (int64_t t = (int64_t)blockIdx.x * kWakeThreads + threadIdx.x; t < mm; t += (int64_t)gridDim.x * kWakeThreads)
  {
    if constexpr (PHASE == 0)
    {
      const int j = (int)(t / s.m), i = (int)(t - (int64_t)j * s.m);
      const int si = i + di, sj = j + dj;  // |di|, |dj| <= 2^20
      const bool inside = si >= 0 && si < s.m && sj >= 0 && sj < s.m;
      const size_t src = (size_t)sj * s.m + si;
      tmp[t] = inside ? s.h[src] : 0.0f;
      tmp[mm + t] = inside ? s.h_prev[src] : 0.0f;
    }
    else
    {
      s.h[t] = tmp[t];
      s.h_prev[t] = tmp[mm + t];
    }
  }
}

// The bilinear form of ocean_wake_sample over the four taps
__device__ __forceinline__ float wake_bilinear(float f00, float f10, float f01, float f11, float fx, float fz)
{
#pragma clang fp contract(off)
  const float x0 = f00 + fx * (f10 - f00);
  const float x1 = f01 + fx * (f11 - f01);
  return x0 + fz * (x1 - x0);
}

// grid: one thread per point, stride loop
__global__ __launch_bounds__(kWakeThreads) void k_wake_sample(WakeCall s, const float2* xz, int64_t n, float4* out)
{
#pragma clang fp contract(off)
  const int m = s.m;
  const float top = (float)(m - 1);
  for (int64_t k = (int64_t)blockIdx.x * kWakeThreads + threadIdx.x; k < n; k += (int64_t)gridDim.x * kWakeThreads)
  {
    const float2 q = xz[k];
    const float u = (q.x - s.ox) / s.dx, v = (q.y - s.oz) / s.dx;
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (u >= 0.0f && u <= top && v >= 0.0f && v <= top)  // a NaN is outside
    {
      const int i0 = min((int)floorf(u), m - 2), j0 = min((int)floorf(v), m - 2);
      const float fx = u - (float)i0, fz = v - (float)j0;
      const size_t t = (size_t)j0 * m + i0;
      const float h00 = s.h[t], h10 = s.h[t + 1], h01 = s.h[t + m], h11 = s.h[t + m + 1];
      r.x = wake_bilinear(h00, h10, h01, h11, fx, fz);
      r.y = ((h10 - h00) + fz * ((h11 - h01) - (h10 - h00))) / s.dx;
      r.z = ((h01 - h00) + fx * ((h11 - h10) - (h01 - h00))) / s.dx;
      if (s.hs > 0.0f)
      {
        const float d00 = h00 - s.h_prev[t], d10 = h10 - s.h_prev[t + 1], d01 = h01 - s.h_prev[t + m],
                    d11 = h11 - s.h_prev[t + m + 1];
        r.w = wake_bilinear(d00, d10, d01, d11, fx, fz) / s.hs;
      }
    }
    out[k] = r;
  }
}

}  // namespace oceanfft
