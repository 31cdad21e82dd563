// device/k_spray.h — spray emitters (ocean_spray_emit): the texels of the pairs' Jacobian maps that emit in
// this step, compacted in (pair, texel) order into 8-float records with the position and the velocity of
// their water particles. Per texel (x, y) of pair i, in unfused fp32 (include/oceanfft.h has the contract):
//     d = threshold - J;   p = min((max(d, 0) * rate) * dt, 1)
//     u = hash_uniform(hash_raw(x, y) ^ seed, step).x;   emits = d > 0 && (p >= 1 || u < p)
// The list is dense and ordered, and it is built with no atomics and no "last block" counter, so a call
// replays bit for bit: four launches, the kernel boundaries are the ordering (as device/k_foam.h).
// Stage 1 (k_spray_count): an item is k_foam_step's, kFoamTile consecutive texels of one emitting pair, a
// linear range of the row-major map; 256 threads issue the item's 2 float4 of J each at once (read once:
// non-temporal) and a range that ends past the map (N = 16, 32) is predicated. The predicate is counted by
// wave ballot and popcount, the four waves' counts cross through LDS into partial[item].
// Stage 2 (k_spray_scan): one workgroup of 1024 threads walks partial in chunks of 1024 items with a carry:
// a wave scan by shuffles, the 16 waves' sums through LDS (two buffers, one barrier per chunk), the next
// chunk's load in flight across the barrier. offset[item] is the exclusive prefix; the 18 count words
// follow from the carry and from the offsets at the pairs' first items. Any grid gives the same result:
// workgroups other than 0 return.
// Stage 3 (k_spray_scatter): stage 1's items. An item that found nothing, or whose first record is past
// the capacity, reads nothing. Otherwise J is read again and the predicate recomputed; an emitting texel's
// rank within the item, in texel order (k, then thread, then element), is the earlier waves' counts (LDS)
// plus the earlier lanes' (mbcnt of the elements' ballots) plus the earlier elements of its own thread. It
// stores d and the id into slots 3 and 7 of record offset + rank when that is below the capacity.
// Stage 4 (k_spray_fill): a point kernel over the records, one thread each up to `written`, which it reads
// from the table: id -> base point -> surface_particle_velocity or the vertex stage (device/
// surface_sample.h, unchanged), the record written whole with two 16-B stores. The evaluation is here and
// not in stage 3 because the emitting share is typically a few per cent: fused, the eight-tap chains of
// every cascade would run with most lanes idle.
// Bytes: stage 1 reads 4 B per texel; stage 3 at most 4 B per texel (nothing for empty items) and writes 8 B
// per record; stage 4 reads 8 B and writes 32 B per record beside its taps. Stages 1 to 3 move 12 B per
// item of scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/memory.h"
#include "device/spectrum.h"
#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kSprayThreads = 256;       // stages 1, 3 and 4
constexpr int kSprayTile = 2048;         // texels per item of stages 1 and 3: kFoamTile, so foam_tiles(n) items per pair
constexpr int kSprayScanThreads = 1024;  // stage 2: its chunk, one item per thread
constexpr int kSprayCounts = 18;         // written, found, found per pair
constexpr int kSprayIdShift = 28;        // id = pair << 28 | texel
static_assert(kMaxSurfaceCascades <= (1 << (32 - kSprayIdShift)), "the pair fits the id's top bits");
static_assert((int64_t)16384 * 16384 <= ((int64_t)1 << kSprayIdShift), "the texel fits the id's low bits");
static_assert(kSprayTile == 8 * kSprayThreads, "an item is two float4 per thread");

// The predicate of texel (x, y) with Jacobian j; d leaves as threshold - j
__device__ __forceinline__ bool spray_emits(const SprayPair& q, float dt, uint32_t step, float j, uint32_t x,
                                            uint32_t y, float& d)
{
#pragma clang fp contract(off)
  d = q.threshold - j;
  const float p = fminf((fmaxf(d, 0.0f) * q.rate) * dt, 1.0f);
  const float u = hash_uniform(hash_raw(x, y) ^ q.seed, step).x;
  return d > 0.0f && (p >= 1.0f || u < p);
}

constexpr int kSprayK = kSprayTile / (4 * kSprayThreads);  // float4 per thread

// The item's J: float4 k of thread tid holds texels 4 * t[k] .. + 3 of the pair's map, live[k] inside it
struct SprayItem
{
  f4v j[kSprayK];
  int t[kSprayK];
  bool live[kSprayK];
};

__device__ __forceinline__ SprayItem spray_load(const SprayCall& s, const SprayPair& q, int tile, int tid)
{
  SprayItem it;
  const f4v* __restrict__ jm = reinterpret_cast<const f4v*>(q.jac);
  const int first = tile * (kSprayTile / 4);  // in float4: < nn / 4 <= 2^26
#pragma unroll
  for (int k = 0; k < kSprayK; k++)
  {
    it.t[k] = first + k * kSprayThreads + tid;
    it.live[k] = it.t[k] < s.nn / 4;
    it.j[k] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
    if (it.live[k])
      it.j[k] = __builtin_nontemporal_load(jm + it.t[k]);
  }
  return it;
}

// grid: items = pairs * tiles, item loop
__global__ __launch_bounds__(kSprayThreads) void k_spray_count(SprayCall s)
{
#pragma clang fp contract(off)
  __shared__ uint32_t lds[kSprayThreads / 64];
  const int tid = threadIdx.x, items = s.pairs * s.tiles;
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int e = item / s.tiles, tile = item - e * s.tiles;
    const SprayPair q = s.c[e];
    const SprayItem it = spray_load(s, q, tile, tid);
    uint32_t count = 0;  // wave-uniform
#pragma unroll
    for (int k = 0; k < kSprayK; k++)
#pragma unroll
      for (int el = 0; el < 4; el++)
      {
        const uint32_t texel = (uint32_t)(4 * it.t[k] + el);
        float d;
        const bool emits =
            it.live[k] && spray_emits(q, s.dt, s.step, it.j[k][el], texel & (uint32_t)(s.n - 1), texel >> s.logn, d);
        count += (uint32_t)__popcll(__ballot(emits));
      }
    if ((tid & 63) == 0)
      lds[tid >> 6] = count;
    __syncthreads();
    if (tid == 0)
    {
      uint32_t v = lds[0];
#pragma unroll
      for (int w = 1; w < kSprayThreads / 64; w++)
        v += lds[w];
      s.partial[item] = v;
    }
    __syncthreads();
  }
}

// one workgroup (others return): the exclusive prefix of partial in item order, then the count table
__global__ __launch_bounds__(kSprayScanThreads) void k_spray_scan(SprayCall s)
{
  constexpr int W = kSprayScanThreads / 64;
  __shared__ uint32_t sums[2][W];
  if (blockIdx.x != 0)
    return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, items = s.pairs * s.tiles;
  unsigned long long carry = 0;  // the items before this chunk: the same in every thread
  uint32_t next = tid < items ? s.partial[tid] : 0u;
  int buf = 0;
  for (int base = 0; base < items; base += kSprayScanThreads, buf ^= 1)
  {
    const int i = base + tid;
    const uint32_t own = next;
    next = i + kSprayScanThreads < items ? s.partial[i + kSprayScanThreads] : 0u;
    uint32_t inc = own;  // inclusive over the wave: a chunk holds at most 1024 * 2048 texels
#pragma unroll
    for (int delta = 1; delta < 64; delta <<= 1)
    {
      const uint32_t o = __shfl_up(inc, delta);
      if (lane >= delta)
        inc += o;
    }
    if (lane == 63)
      sums[buf][wave] = inc;
    __syncthreads();
    uint32_t below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < W; w++)
    {
      const uint32_t t = sums[buf][w];
      below += w < wave ? t : 0u;
      total += t;
    }
    if (i < items)
      s.offset[i] = (int64_t)(carry + below + (inc - own));
    carry += total;
  }
  __syncthreads();  // the offsets at the pairs' first items, written by other threads of this workgroup
  if (tid < kSprayCounts)
  {
    int64_t v = 0;
    if (tid == 0)
      v = (int64_t)carry < s.capacity ? (int64_t)carry : s.capacity;
    else if (tid == 1)
      v = (int64_t)carry;
    else
      for (int e = 0; e < s.pairs; e++)
        if (s.c[e].index == tid - 2)
        {
          const int64_t lo = s.offset[(size_t)e * s.tiles];
          const int64_t hi = e + 1 < s.pairs ? s.offset[(size_t)(e + 1) * s.tiles] : (int64_t)carry;
          v = hi - lo;
        }
    s.table[tid] = v;
  }
}

// grid: items = pairs * tiles, item loop
__global__ __launch_bounds__(kSprayThreads) void k_spray_scatter(SprayCall s)
{
#pragma clang fp contract(off)
  constexpr int W = kSprayThreads / 64;
  __shared__ uint32_t lds[kSprayK][W];
  const int tid = threadIdx.x, wave = tid >> 6, items = s.pairs * s.tiles;
  uint32_t* out_bits = reinterpret_cast<uint32_t*>(s.out);
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int64_t first = s.offset[item];
    if (s.partial[item] == 0u || first >= s.capacity)  // the same in every thread of the workgroup
      continue;
    const int e = item / s.tiles, tile = item - e * s.tiles;
    const SprayPair q = s.c[e];
    const SprayItem it = spray_load(s, q, tile, tid);
    float d[kSprayK][4];
    uint32_t mask[kSprayK], before[kSprayK];  // the thread's emitting elements; emitting texels of earlier lanes
#pragma unroll
    for (int k = 0; k < kSprayK; k++)
    {
      uint32_t wave_count = 0;
      mask[k] = 0;
      before[k] = 0;
#pragma unroll
      for (int el = 0; el < 4; el++)
      {
        const uint32_t texel = (uint32_t)(4 * it.t[k] + el);
        const bool emits = it.live[k] && spray_emits(q, s.dt, s.step, it.j[k][el], texel & (uint32_t)(s.n - 1),
                                                     texel >> s.logn, d[k][el]);
        const unsigned long long b = __ballot(emits);
        before[k] += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        wave_count += (uint32_t)__popcll(b);
        mask[k] |= (emits ? 1u : 0u) << el;
      }
      if ((tid & 63) == 0)
        lds[k][wave] = wave_count;
    }
    __syncthreads();
    uint32_t base = 0;  // emitting texels before float4 k = 0 of this wave; then before k = 1, ..
#pragma unroll
    for (int k = 0; k < kSprayK; k++)
    {
      uint32_t rank = base + before[k];
#pragma unroll
      for (int w = 0; w < W; w++)
      {
        const uint32_t c = lds[k][w];
        rank += w < wave ? c : 0u;
        base += c;
      }
#pragma unroll
      for (int el = 0; el < 4; el++)
        if ((mask[k] >> el) & 1u)
        {
          const int64_t rec = first + rank;
          rank++;
          if (rec < s.capacity)
          {
            s.out[rec * 8 + 3] = d[k][el];
            out_bits[rec * 8 + 7] = ((uint32_t)q.index << kSprayIdShift) | (uint32_t)(4 * it.t[k] + el);
          }
        }
    }
    __syncthreads();
  }
}

// grid: launch_spray_emit's, from the capacity; a thread per record up to table[0], item loop
template <bool VELOCITY>
__global__ __launch_bounds__(kSprayThreads) void k_spray_fill(SurfaceParams p, SurfaceRates r, SprayTiles tiles,
                                                              const int64_t* __restrict__ table, int logn, float* out)
{
#pragma clang fp contract(off)
  const int64_t written = table[0];
  float4* rows = reinterpret_cast<float4*>(out);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < written;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    const float d = out[8 * idx + 3], id_bits = out[8 * idx + 7];
    const uint32_t id = __float_as_uint(id_bits);
    const int i = (int)(id >> kSprayIdShift);
    const uint32_t texel = id & ((1u << kSprayIdShift) - 1u);
    const uint32_t x = texel & (uint32_t)(p.n - 1), y = texel >> logn;
    const float plane = p.c[i].plane;
    const float cell = plane / (float)p.n;
    float px = ((float)x + 0.5f) * cell + (float)tiles.t[i][0] * plane;
    float pz = ((float)y + 0.5f) * cell + (float)tiles.t[i][1] * plane;
    float py = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if constexpr (VELOCITY)
      surface_particle_velocity(p, r, px, py, pz, ux, uy, uz);
    else
      surface_vertex_stage<false>(p, px, py, pz);
    rows[2 * idx] = make_float4(px, py, pz, d);
    rows[2 * idx + 1] = make_float4(ux, uy, uz, id_bits);
  }
}

}  // namespace oceanfft
