// device/k_bounds.h — the bounds of a generator's maps (ocean_generator_build_bounds): per cascade the
// minimum and maximum of the nine channels (heightMap x, y, z, w, displacementMap x, y, z, w, jacobian)
// over the N^2 texels, 18 floats [2j] = min, [2j + 1] = max. Min and max are exact, so the values do not
// depend on the order of the reduction; no float atomics and no "last block" counter: two launches.
// Stage 1 (k_bounds_tiles): an item is kBoundsTile consecutive texels of one cascade, a linear range of the
// row-major maps, so every N has the same shape. A workgroup of 256 threads issues all of the item's loads
// at once, non-temporal: 8 float4 of heightMap and 8 of displacementMap per thread (texel k * 256 + tid: a
// wave instruction reads 1 KiB, eight whole 128-B lines) and 2 float4 of the Jacobian (four texels each:
// which thread sees which texel does not matter to a minimum). A range that ends past the map (N = 16, 32:
// 256 and 1024 texels) clamps its indices to the last texel, which is read again: no predicate, same result.
// Each thread keeps 18 running values; a wave folds them in registers (permlane32 / permlane16 swaps,
// bank-masked DPP row shifts, quad_perm: xor_lane_pair of device/lane_xchg.h, which k_hulls.h's fold64
// combines with an add and this file with min / max); the
// waves' 18 values cross through LDS and the item's row goes to partial[item].
// Stage 2 (k_bounds_fold): an item is one cascade; 1024 threads fold the cascade's partial rows the same way
// into the table.
#pragma once

#include <hip/hip_runtime.h>

#include "device/lane_xchg.h"
#include "device/memory.h"
#include "device/wave_tile.h"

namespace oceanfft
{

constexpr int kBoundsValues = 18;
constexpr int kBoundsThreads = 256;       // stage 1
constexpr int kBoundsTile = 2048;         // texels per stage-1 item
constexpr int kBoundsFoldThreads = 1024;  // stage 2

struct BoundsBuild
{
  const float4* maps;  // [cascade][heightMap, displacementMap][nn]
  const float* jac;    // [cascade][nn]
  float* partial;      // [cascade][tiles][18]
  float* table;        // [cascade][18]
  int nn;              // texels per map (a power of two >= 256)
  int tiles;           // stage-1 items per cascade: max(nn / kBoundsTile, 1)
  int cascades;
};

// bounds_fold_step: device/wave_tile.h (device/k_moorings.h folds a line's largest tension with it)
template <bool MAX>
__device__ __forceinline__ float bounds_wave_fold(float v)
{
  v = bounds_fold_step<32, MAX>(v);
  v = bounds_fold_step<16, MAX>(v);
  v = bounds_fold_step<8, MAX>(v);
  v = bounds_fold_step<4, MAX>(v);
  v = bounds_fold_step<2, MAX>(v);
  return bounds_fold_step<1, MAX>(v);
}

// The workgroup's 18 values from every thread's b[18] (even: min, odd: max) into row[0..18). lds: WAVES rows.
// Every lane stays active through the cross-lane reads. Ends with a barrier, so lds can be reused at once.
template <int WAVES>
__device__ __forceinline__ void bounds_block_fold(float (&b)[kBoundsValues], float (*lds)[kBoundsValues],
                                                  float* __restrict__ row, int tid)
{
#pragma unroll
  for (int j = 0; j < kBoundsValues; j += 2)
  {
    b[j] = bounds_wave_fold<false>(b[j]);
    b[j + 1] = bounds_wave_fold<true>(b[j + 1]);
  }
  if ((tid & 63) == 0)
#pragma unroll
    for (int j = 0; j < kBoundsValues; j++)
      lds[tid >> 6][j] = b[j];
  __syncthreads();
  if (tid < kBoundsValues)
  {
    float v = lds[0][tid];
    for (int w = 1; w < WAVES; w++)
      v = (tid & 1) ? fmaxf(v, lds[w][tid]) : fminf(v, lds[w][tid]);
    row[tid] = v;
  }
  __syncthreads();
}

__device__ __forceinline__ void bounds_init(float (&b)[kBoundsValues])
{
#pragma unroll
  for (int j = 0; j < kBoundsValues; j += 2)
  {
    b[j] = __builtin_inff();
    b[j + 1] = -__builtin_inff();
  }
}

__device__ __forceinline__ void bounds_take(float (&b)[kBoundsValues], int ch, float v)
{
  b[2 * ch] = fminf(b[2 * ch], v);
  b[2 * ch + 1] = fmaxf(b[2 * ch + 1], v);
}

__device__ __forceinline__ f4v bounds_load(const float4* p)
{
  return __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
}

// grid: items = cascades * tiles, item loop
__global__ __launch_bounds__(kBoundsThreads) void k_bounds_tiles(BoundsBuild s)
{
  __shared__ float lds[kBoundsThreads / 64][kBoundsValues];
  const int tid = threadIdx.x, items = s.cascades * s.tiles;
  constexpr int K = kBoundsTile / kBoundsThreads;  // float4 loads per thread of a 4-channel map
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int cas = item / s.tiles, tile = item - cas * s.tiles;
    const float4* __restrict__ hm = s.maps + (size_t)(2 * cas) * s.nn;
    const float4* __restrict__ dm = hm + s.nn;
    const float4* __restrict__ jm = reinterpret_cast<const float4*>(s.jac + (size_t)cas * s.nn);
    const int first = tile * kBoundsTile;  // < nn <= 2^28
    f4v h[K], d[K], j[K / 4];
#pragma unroll
    for (int k = 0; k < K; k++)
    {
      const int t = min(first + k * kBoundsThreads + tid, s.nn - 1);
      h[k] = bounds_load(hm + t);
      d[k] = bounds_load(dm + t);
    }
#pragma unroll
    for (int k = 0; k < K / 4; k++)
      j[k] = bounds_load(jm + min(first / 4 + k * kBoundsThreads + tid, s.nn / 4 - 1));
    float b[kBoundsValues];
    bounds_init(b);
#pragma unroll
    for (int k = 0; k < K; k++)
    {
      bounds_take(b, 0, h[k].x);
      bounds_take(b, 1, h[k].y);
      bounds_take(b, 2, h[k].z);
      bounds_take(b, 3, h[k].w);
      bounds_take(b, 4, d[k].x);
      bounds_take(b, 5, d[k].y);
      bounds_take(b, 6, d[k].z);
      bounds_take(b, 7, d[k].w);
    }
#pragma unroll
    for (int k = 0; k < K / 4; k++)
    {
      bounds_take(b, 8, j[k].x);
      bounds_take(b, 8, j[k].y);
      bounds_take(b, 8, j[k].z);
      bounds_take(b, 8, j[k].w);
    }
    bounds_block_fold<kBoundsThreads / 64>(b, lds, s.partial + (size_t)item * kBoundsValues, tid);
  }
}

// grid: items = cascades, item loop
__global__ __launch_bounds__(kBoundsFoldThreads) void k_bounds_fold(BoundsBuild s)
{
  __shared__ float lds[kBoundsFoldThreads / 64][kBoundsValues];
  const int tid = threadIdx.x;
  for (int cas = blockIdx.x; cas < s.cascades; cas += gridDim.x)
  {
    const float* __restrict__ rows = s.partial + (size_t)cas * s.tiles * kBoundsValues;
    float b[kBoundsValues];
    bounds_init(b);
    for (int r = tid; r < s.tiles; r += kBoundsFoldThreads)
#pragma unroll
      for (int j = 0; j < kBoundsValues; j += 2)
      {
        const float2 q = *reinterpret_cast<const float2*>(rows + (size_t)r * kBoundsValues + j);
        b[j] = fminf(b[j], q.x);
        b[j + 1] = fmaxf(b[j + 1], q.y);
      }
    bounds_block_fold<kBoundsFoldThreads / 64>(b, lds, s.table + (size_t)cas * kBoundsValues, tid);
  }
}

}  // namespace oceanfft
