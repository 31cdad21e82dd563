// device/k_foam_deposit.h — ocean_foam_deposit (include/oceanfft.h): the impacts of a particle step splatted
// into the persistent foam of the call's pairs. The deposit is the transpose of the foam sampler: a record at
// the world position (px, pz) adds to the four texels surface_foam_stage would read there, with the weights it
// would read them with (linear_repeat_taps, device/surface_sample.h). Per record, pair and tap, in unfused fp32:
//     d = amount + per_speed * max(-uy, 0);   m = min(d * w, 1);   u = (uint64)(m * 2^24)
// A scatter with heavy collisions (a coarse cascade's texel receives hundreds of taps of one step) whose result
// must replay bit for bit, so no float atomics: the contributions are integers, units of 2^-24, and integer
// sums commute exactly.
// Accumulators: one uint64 per texel and cascade of every generator that has received a deposit, 8 B per point
// (1 GiB at 8 x 4096^2), all zero between calls.
// Launch 1 (k_foam_deposit_add): a lane per record, an item is kFoamDepositItem records. Per pair and tap slot
// a no-return agent-scope 64-bit integer add of u into the texel's accumulator; u == 0 issues nothing. With
// MERGE, runs of neighbouring lanes on the same texel (an impact list keeps the pool's order, so neighbouring
// records land in the same texel of a coarse cascade) are folded within the wave first by k_camera_splat's
// segmented scan (device/k_camera_spray.h), and the last lane of a run issues one add: a wave's sum is at most
// 64 * 2^24 and fits the scan's 32 bits, and + is exact, so the words are what the unmerged adds give.
// Launch 2 (k_foam_deposit_apply): the same lanes visit the same taps. A lane whose load of the accumulator is
// non-zero exchanges it with 0 (returning, agent scope); the lane that receives a non-zero value owns the texel
// for this call and applies
//     F = min(F + (float)min(A, 2^24) * 2^-24, 1)
// with a plain load and store: exactly one lane per texel and call can receive non-zero (nothing adds during
// this launch), so F needs no atomic, the accumulators are zero again without a clearing pass, and the work
// scales with the records, not with N^2. Correctness rests on the exchange's result alone: the load before it
// is a filter (relaxed, agent scope: served by L2, which may hold the line from before another XCD's exchange;
// a stale value is non-zero and costs one exchange that returns 0; a kernel boundary lies between the adds and
// this launch, so a non-zero word is never seen as zero). With MERGE only the first lane of a run probes.
// Counts: taps with u > 0 (launch 1), texels owned and owned texels with F + add >= 1 (launch 2), by wave
// ballot into the workgroup's LDS row and from there into one partial row per workgroup, so the scratch does
// not grow with the record count; launch 3 (k_foam_deposit_fold) adds the rows into the int64 table, as
// k_foam_fold does.
// Traffic per record: 12 B read of its 32-B record in each of the two launches (whole lines when the list is
// dense: 64 B), and per active pair 4 adds of 8 B, 4 loads of 8 B, and per owned texel an 8-B exchange and 4 B
// of F read and written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kFoamDepositThreads = kFoamDepositItem;
constexpr int kFoamDepositFoldThreads = 256;
constexpr uint32_t kFoamDepositOne = 1u << 24;  // the units of 1.0
constexpr uint32_t kFoamDepositNoTexel = 0xFFFFFFFFu;

// n = min(*count_device, max_records), not below 0
__device__ __forceinline__ int64_t foam_deposit_records(const FoamDepositCall& s)
{
  int64_t n = s.max_records;
  if (s.count_device)
  {
    const int64_t c = *s.count_device;
    n = c < n ? c : n;
  }
  return n < 0 ? 0 : n;
}

// What the two launches share: a record's three floats
struct FoamDepositRecord
{
  float px, pz, speed;  // speed = max(-uy, 0)
  bool live;
};

__device__ __forceinline__ FoamDepositRecord foam_deposit_record(const FoamDepositCall& s, int64_t r, int64_t n)
{
  FoamDepositRecord v{0.0f, 0.0f, 0.0f, r < n};
  if (v.live)
  {
    const float* rec = s.records + 8 * r;
    v.px = rec[0];
    v.pz = rec[2];
    v.speed = fmaxf(-rec[5], 0.0f);
  }
  return v;
}

// The units of one tap: within 0 .. 2^24 whatever the inputs (a NaN product gives 2^24)
__device__ __forceinline__ uint32_t foam_deposit_units(float d, float w)
{
#pragma clang fp contract(off)
  const float m = fmaxf(fminf(d * w, 1.0f), 0.0f);
  return (uint32_t)(m * 16777216.0f);
}

// The four taps of a record on one pair: texel (kFoamDepositNoTexel where the tap has no units) and units
struct FoamDepositTaps
{
  uint32_t q[4], u[4];
};

__device__ __forceinline__ FoamDepositTaps foam_deposit_taps(const FoamDepositPair& c, int n, const FoamDepositRecord& v)
{
#pragma clang fp contract(off)
  const float d = c.amount + c.per_speed * v.speed;
  const LinearTaps k = linear_repeat_taps(n, v.px / c.plane, v.pz / c.plane);  // & (n - 1): inside the map
  const int o[4] = {k.o00, k.o10, k.o01, k.o11};
  const float w[4] = {k.w00, k.w10, k.w01, k.w11};
  FoamDepositTaps t;
#pragma unroll
  for (int j = 0; j < 4; j++)
  {
    t.u[j] = v.live ? foam_deposit_units(d, w[j]) : 0u;
    t.q[j] = t.u[j] > 0u ? (uint32_t)o[j] : kFoamDepositNoTexel;
  }
  return t;
}

// grid: at most kFoamDepositMaxGrid, item loop; every workgroup writes its row of s.taps
template <bool MERGE>
__global__ __launch_bounds__(kFoamDepositThreads) void k_foam_deposit_add(FoamDepositCall s)
{
  __shared__ uint32_t row[kMaxSurfaceCascades];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < kMaxSurfaceCascades)
    row[tid] = 0u;
  __syncthreads();
  const int64_t n = foam_deposit_records(s);
  const int64_t items = (n + kFoamDepositItem - 1) / kFoamDepositItem;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const FoamDepositRecord v = foam_deposit_record(s, item * kFoamDepositItem + tid, n);
    for (int i = 0; i < s.pairs; i++)
    {
      const FoamDepositPair& c = s.c[i];
      if (!c.acc)
        continue;
      const FoamDepositTaps t = foam_deposit_taps(c, s.n, v);
      uint32_t count = 0;  // wave-uniform
#pragma unroll
      for (int j = 0; j < 4; j++)
      {
        const uint32_t q = t.q[j];
        uint32_t sum = t.u[j];
        bool issue = sum > 0u;
        count += (uint32_t)__popcll(__ballot(issue));
        if constexpr (MERGE)
        {
          const uint32_t before = __shfl_up(q, 1);
          const bool head = lane == 0 || before != q;  // the first lane of a run of equal texels
          if (__any(issue && !head))
          {
            uint32_t open = head ? 0u : 1u;  // the lane's scan still reaches further back
#pragma unroll
            for (int d = 1; d < 64; d <<= 1)
            {
              const uint32_t a = __shfl_up(sum, d), o = __shfl_up(open, d);
              if (lane >= d && open)
              {
                sum += a;
                open = o;
              }
            }
          }
          const uint32_t next_head = __shfl_down(head ? 1u : 0u, 1);
          issue = issue && (lane == 63 || next_head);
        }
        if (issue)
          (void)__hip_atomic_fetch_add(c.acc + q, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (lane == 0 && count)
        atomicAdd(&row[i], count);  // LDS, integer
    }
  }
  __syncthreads();
  if (tid < kMaxSurfaceCascades)
    s.taps[(size_t)blockIdx.x * kMaxSurfaceCascades + tid] = row[tid];
}

// grid: at most kFoamDepositMaxGrid, item loop; every workgroup writes its row of s.owned
template <bool MERGE>
__global__ __launch_bounds__(kFoamDepositThreads) void k_foam_deposit_apply(FoamDepositCall s)
{
#pragma clang fp contract(off)
  __shared__ uint32_t row[kMaxSurfaceCascades][2];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 2 * kMaxSurfaceCascades)
    row[tid >> 1][tid & 1] = 0u;
  __syncthreads();
  const int64_t n = foam_deposit_records(s);
  const int64_t items = (n + kFoamDepositItem - 1) / kFoamDepositItem;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const FoamDepositRecord v = foam_deposit_record(s, item * kFoamDepositItem + tid, n);
    for (int i = 0; i < s.pairs; i++)
    {
      const FoamDepositPair& c = s.c[i];
      if (!c.acc)
        continue;
      const FoamDepositTaps t = foam_deposit_taps(c, s.n, v);
      uint32_t touched = 0, saturated = 0;  // wave-uniform
#pragma unroll
      for (int j = 0; j < 4; j++)
      {
        const uint32_t q = t.q[j];
        bool probe = t.u[j] > 0u;
        if constexpr (MERGE)
        {
          const uint32_t before = __shfl_up(q, 1);
          probe = probe && (lane == 0 || before != q);  // one probe per run of equal texels
        }
        bool own = false, full = false;
        if (probe && __hip_atomic_load(c.acc + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull)
        {
          const unsigned long long a = __hip_atomic_exchange(c.acc + q, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (a != 0ull)
          {
            const uint32_t units = a < (unsigned long long)kFoamDepositOne ? (uint32_t)a : kFoamDepositOne;
            const float sum = c.foam[q] + (float)units * 0x1p-24f;
            c.foam[q] = fminf(sum, 1.0f);
            own = true;
            full = sum >= 1.0f;
          }
        }
        touched += (uint32_t)__popcll(__ballot(own));
        saturated += (uint32_t)__popcll(__ballot(full));
      }
      if (lane == 0 && touched)
      {
        atomicAdd(&row[i][0], touched);
        if (saturated)
          atomicAdd(&row[i][1], saturated);
      }
    }
  }
  __syncthreads();
  if (tid < 2 * kMaxSurfaceCascades)
    s.owned[(size_t)blockIdx.x * 2 * kMaxSurfaceCascades + tid] = row[tid >> 1][tid & 1];
}

// grid: 1. Column k < 16 of the taps rows and column k < 32 of the owned rows, a wave each in turn, into the
// table; the slots of pairs the call does not have are 0.
__global__ __launch_bounds__(kFoamDepositFoldThreads) void k_foam_deposit_fold(FoamDepositCall s)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0)
  {
    s.table[0] = foam_deposit_records(s);
    s.table[1] = s.count_device ? *s.count_device : s.max_records;
  }
  for (int col = wave; col < 3 * kMaxSurfaceCascades; col += kFoamDepositFoldThreads / 64)
  {
    const int pair = col / 3, what = col - 3 * pair;  // taps, touched, saturated
    unsigned long long v = 0;
    if (pair < s.pairs)
    {
      if (what == 0)
        for (int r = lane; r < s.grid_add; r += 64)
          v += s.taps[(size_t)r * kMaxSurfaceCascades + pair];
      else
        for (int r = lane; r < s.grid_apply; r += 64)
          v += s.owned[((size_t)r * kMaxSurfaceCascades + pair) * 2 + (what - 1)];
    }
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1)
      v += __shfl_xor(v, stride);
    if (lane == 0)
      s.table[2 + col] = (int64_t)v;
  }
}

}  // namespace oceanfft
