// device/k_foam.h — persistent foam (ocean_generator_advance_foam): per cascade one R32F map F beside the
// Jacobian J, stepped in place once per frame, and three counts of the step. Per texel, in unfused fp32
// (include/oceanfft.h has the contract):
//     s = max(bias - J, 0) * gain;   t = F * a + s * dt;   F' = min(t, 1)
//     breaking += (bias - J > 0);   covered += (F' >= level);   saturated += (t >= 1)
// with a = exp(-decay * dt) rounded once on the host. Counts are integers, so they do not depend on the
// order of the sums; no atomics and no "last block" counter: two launches, as device/k_bounds.h.
// Stage 1 (k_foam_step): an item is kFoamTile consecutive texels of one cascade, a linear range of the
// row-major maps, so every N has the same shape. A workgroup of 256 threads issues all of the item's loads
// at once: per thread 2 float4 of J (read once: non-temporal, as bounds_load) and 2 float4 of F (texels
// 4 * (k * 256 + tid) ..: a wave instruction reads 1 KiB, eight whole 128-B lines), then steps its eight
// texels and stores F with two 16-B stores. The update is in place, so unlike k_bounds_tiles a range that
// ends past the map (N = 16, 32: 256 and 1024 texels) is predicated, not clamped: a texel read twice would
// be stepped twice; and an item's range is disjoint from every other item's. Each predicate is counted by
// wave ballot and popcount (scalar adds), the waves' three counts cross through LDS and the item's row goes
// to partial[item] (uint32: an item has 2048 texels).
// Stage 2 (k_foam_fold): an item is one cascade; 1024 threads add the cascade's partial rows (up to 2^17
// at N = 16384) into the int64 table.
// Cache policy. J is read once per step: non-temporal loads (they skip the CU's L1, the line is served by
// L2 as a plain load's). F's loads and stores are plain: a plain store leaves the line in the XCD's L2, so
// at 3 x 256^2 (0.75 MB) the next frame's step and the foam sampler find F there; a write-through store
// would drop it. At 8 x 4096^2 (537 MB) nothing survives a frame in any cache whatever the policy, and
// a step is one pass over 12 B per texel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/memory.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kFoamThreads = 256;       // stage 1
constexpr int kFoamTile = 2048;         // texels per stage-1 item
constexpr int kFoamFoldThreads = 1024;  // stage 2
constexpr int kFoamCounts = 3;          // breaking, covered, saturated

// grid: items = cascades * tiles, item loop
__global__ __launch_bounds__(kFoamThreads) void k_foam_step(FoamStep s)
{
#pragma clang fp contract(off)
  __shared__ uint32_t lds[kFoamThreads / 64][kFoamCounts];
  const int tid = threadIdx.x, items = s.cascades * s.tiles;
  constexpr int K = kFoamTile / (4 * kFoamThreads);  // float4 per thread and map
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int cas = item / s.tiles, tile = item - cas * s.tiles;
    const FoamCascade q = s.c[cas];
    const f4v* __restrict__ jm = reinterpret_cast<const f4v*>(s.jac + (size_t)cas * s.nn);
    f4v* fm = reinterpret_cast<f4v*>(s.foam + (size_t)cas * s.nn);
    const int first = tile * (kFoamTile / 4);  // in float4: < nn / 4 <= 2^26
    f4v j[K], f[K];
    bool live[K];
#pragma unroll
    for (int k = 0; k < K; k++)
    {
      const int t = first + k * kFoamThreads + tid;
      live[k] = t < s.nn / 4;
      j[k] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
      f[k] = j[k];
      if (live[k])
      {
        j[k] = __builtin_nontemporal_load(jm + t);
        f[k] = fm[t];
      }
    }
    uint32_t n_break = 0, n_cover = 0, n_sat = 0;  // wave-uniform
#pragma unroll
    for (int k = 0; k < K; k++)
    {
      f4v out;
#pragma unroll
      for (int e = 0; e < 4; e++)
      {
        const float d = q.bias - j[k][e];
        const float inj = fmaxf(d, 0.0f) * q.gain;
        const float t = f[k][e] * q.a + inj * q.dt;
        const float r = fminf(t, 1.0f);
        out[e] = r;
        n_break += (uint32_t)__popcll(__ballot(live[k] && d > 0.0f));
        n_cover += (uint32_t)__popcll(__ballot(live[k] && r >= q.level));
        n_sat += (uint32_t)__popcll(__ballot(live[k] && t >= 1.0f));
      }
      if (live[k])
        fm[first + k * kFoamThreads + tid] = out;
    }
    if ((tid & 63) == 0)
    {
      lds[tid >> 6][0] = n_break;
      lds[tid >> 6][1] = n_cover;
      lds[tid >> 6][2] = n_sat;
    }
    __syncthreads();
    if (tid < kFoamCounts)
    {
      uint32_t v = lds[0][tid];
#pragma unroll
      for (int w = 1; w < kFoamThreads / 64; w++)
        v += lds[w][tid];
      s.partial[(size_t)item * kFoamCounts + tid] = v;
    }
    __syncthreads();
  }
}

// grid: items = cascades, item loop
__global__ __launch_bounds__(kFoamFoldThreads) void k_foam_fold(FoamStep s)
{
  __shared__ unsigned long long lds[kFoamFoldThreads / 64][kFoamCounts];
  const int tid = threadIdx.x;
  for (int cas = blockIdx.x; cas < s.cascades; cas += gridDim.x)
  {
    const uint32_t* __restrict__ rows = s.partial + (size_t)cas * s.tiles * kFoamCounts;
    unsigned long long v[kFoamCounts] = {0, 0, 0};
    for (int r = tid; r < s.tiles; r += kFoamFoldThreads)
#pragma unroll
      for (int c = 0; c < kFoamCounts; c++)
        v[c] += rows[(size_t)r * kFoamCounts + c];
#pragma unroll
    for (int c = 0; c < kFoamCounts; c++)
#pragma unroll
      for (int stride = 32; stride >= 1; stride >>= 1)
        v[c] += __shfl_xor(v[c], stride);
    if ((tid & 63) == 0)
#pragma unroll
      for (int c = 0; c < kFoamCounts; c++)
        lds[tid >> 6][c] = v[c];
    __syncthreads();
    if (tid < kFoamCounts)
    {
      unsigned long long t = lds[0][tid];
#pragma unroll
      for (int w = 1; w < kFoamFoldThreads / 64; w++)
        t += lds[w][tid];
      s.table[(size_t)cas * kFoamCounts + tid] = (int64_t)t;
    }
    __syncthreads();
  }
}

}  // namespace oceanfft
