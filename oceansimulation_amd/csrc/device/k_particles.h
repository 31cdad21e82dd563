// device/k_particles.h — spray particles (ocean_particles_step): one step of a persistent pool of 8-float
// particles (px, py, pz, age, ux, uy, uz, id). Per particle, in unfused fp32 (include/oceanfft.h has the
// contract): semi-implicit Euler under gravity and linear drag toward a wind, the water height w under the
// moved particle by the query's fixed point (surface_base_point<false>, device/surface_sample.h, unchanged),
//     landed = !(py' > w);   expired = !landed && !(age' < lifetime);   survives = neither
// then the survivors compacted in order into the next list, the landed in order into the caller's impact
// list, and the records of an ocean_spray_emit call appended after the survivors. No atomics and no "last
// block" counter, so a step replays bit for bit: three launches, the kernel boundaries are the ordering (as
// device/k_spray.h).
// Stage 1 (k_particles_move): an item is kParticleItem = 256 consecutive particles, one per thread; the item
// loop runs to `alive`, read from the table. A thread loads its record with two 16-B loads, integrates, runs
// the fixed point and stores the moved record in place (it owns the record, so the second buffer stays free
// for the compaction); a landed particle's slot 1 leaves as w, which is its impact record. The two fates are
// taken by wave ballot; the ballots go to scratch, so stage 3 never repeats the query, and their popcounts
// cross through LDS into two uint32 per item.
// Stage 2 (k_particles_scan): one workgroup of 1024 threads (others return): k_spray_scan's chunked carry
// walk over both per-item counts at once, int64 offsets; then the count table from the carries and the
// emitter's `written`, the old table[0] moving into table[1].
// Stage 3 (k_particles_scatter): stage 1's items. A particle's rank is the item's offset plus the earlier
// waves' counts (LDS) plus mbcnt of the stored ballot; whole 32-B records go to the next list or, below the
// capacity, to landed_out. The same launch appends: a grid-stride loop over `appended` emitter records
// converts and stores them after the survivors.
// Bytes per particle: stage 1 reads 32 B and writes 32 B beside the query's taps (4 x 3 dwords per cascade
// and vertex stage, up to iterations + 1 stages) and writes 2 bits of ballots; stage 3 reads the 2 bits and
// 32 B and writes 32 B (an expired particle: the 2 bits alone); an appended record is 32 B read and 32 B
// written. Stages 1 to 3 move 24 B per item of counts and offsets. Stage 1 is latency-bound on the tap
// chains, like k_spray_fill; stage 3 is the only pure stream.
// -Rpass-analysis=kernel-resource-usage must report no scratch memory for the three kernels (DESIGN.md has
// the VGPR counts).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kParticleThreads = 256;        // stages 1 and 3
constexpr int kParticleScanThreads = 1024;   // stage 2: its chunk, one item per thread
constexpr int kParticleWaves = kParticleThreads / 64;
static_assert(kParticleItem == kParticleThreads, "an item is one particle per thread");

// the lanes below this one whose bit is set in a wave ballot
__device__ __forceinline__ uint32_t particle_rank(unsigned long long b)
{
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// grid: launch_particles_step's, from the capacity; item loop to table[0]
__global__ __launch_bounds__(kParticleThreads) void k_particles_move(ParticleCall c, SurfaceParams p)
{
#pragma clang fp contract(off)
  __shared__ uint32_t lds[kParticleWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t alive = c.table[0];
  const int64_t items = (alive + kParticleItem - 1) / kParticleItem;
  float4* rows = reinterpret_cast<float4*>(c.cur);
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int64_t idx = item * kParticleItem + tid;
    bool landed = false, survives = false;
    if (idx < alive)
    {
      const float4 a = rows[2 * idx], b = rows[2 * idx + 1];
      const float ax = c.drag * (c.wind[0] - b.x);
      const float ay = c.drag * (c.wind[1] - b.y) - c.gravity;
      const float az = c.drag * (c.wind[2] - b.z);
      const float ux = b.x + ax * c.dt, uy = b.y + ay * c.dt, uz = b.z + az * c.dt;
      const float px = a.x + ux * c.dt, py = a.y + uy * c.dt, pz = a.z + uz * c.dt;
      const float age = a.w + c.dt;
      float bx = px, bz = pz, vx, w, vz;  // a cold start at q = (px', pz')
      surface_base_point<false>(p, px, pz, c.iterations, c.tolerance, bx, bz, vx, w, vz);
      landed = !(py > w);  // a NaN lands
      survives = !landed && age < c.lifetime;
      rows[2 * idx] = make_float4(px, landed ? w : py, pz, age);
      rows[2 * idx + 1] = make_float4(ux, uy, uz, b.w);
    }
    const unsigned long long bs = __ballot(survives), bl = __ballot(landed);
    if (lane == 0)
    {
      unsigned long long* out = c.ballots + ((size_t)item * kParticleWaves + wave) * 2;
      out[0] = bs;
      out[1] = bl;
      lds[wave][0] = (uint32_t)__popcll(bs);
      lds[wave][1] = (uint32_t)__popcll(bl);
    }
    __syncthreads();
    if (tid < 2)
    {
      uint32_t v = lds[0][tid];
#pragma unroll
      for (int w = 1; w < kParticleWaves; w++)
        v += lds[w][tid];
      c.partial[2 * item + tid] = v;
    }
    __syncthreads();
  }
}

// one workgroup (others return): the exclusive prefixes of partial in item order, then the count table
__global__ __launch_bounds__(kParticleScanThreads) void k_particles_scan(ParticleCall c)
{
  constexpr int W = kParticleScanThreads / 64;
  __shared__ uint32_t sums[2][W][2];
  if (blockIdx.x != 0)
    return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t alive = c.table[0];
  const int items = (int)((alive + kParticleItem - 1) / kParticleItem);  // <= 2^20
  const uint2* __restrict__ partial = reinterpret_cast<const uint2*>(c.partial);
  unsigned long long carry_s = 0, carry_l = 0;  // the items before this chunk: the same in every thread
  uint2 next = tid < items ? partial[tid] : make_uint2(0u, 0u);
  int buf = 0;
  for (int base = 0; base < items; base += kParticleScanThreads, buf ^= 1)
  {
    const int i = base + tid;
    const uint2 own = next;
    next = i + kParticleScanThreads < items ? partial[i + kParticleScanThreads] : make_uint2(0u, 0u);
    uint32_t inc_s = own.x, inc_l = own.y;  // inclusive over the wave: a chunk holds at most 1024 * 256 particles
#pragma unroll
    for (int delta = 1; delta < 64; delta <<= 1)
    {
      const uint32_t os = __shfl_up(inc_s, delta), ol = __shfl_up(inc_l, delta);
      if (lane >= delta)
      {
        inc_s += os;
        inc_l += ol;
      }
    }
    if (lane == 63)
    {
      sums[buf][wave][0] = inc_s;
      sums[buf][wave][1] = inc_l;
    }
    __syncthreads();
    uint32_t below_s = 0, below_l = 0, total_s = 0, total_l = 0;
#pragma unroll
    for (int w = 0; w < W; w++)
    {
      const uint32_t ts = sums[buf][w][0], tl = sums[buf][w][1];
      below_s += w < wave ? ts : 0u;
      below_l += w < wave ? tl : 0u;
      total_s += ts;
      total_l += tl;
    }
    if (i < items)
    {
      c.offset[2 * (size_t)i] = (int64_t)(carry_s + below_s + (inc_s - own.x));
      c.offset[2 * (size_t)i + 1] = (int64_t)(carry_l + below_l + (inc_l - own.y));
    }
    carry_s += total_s;
    carry_l += total_l;
  }
  __syncthreads();  // every thread has read table[0]
  if (tid == 0)
  {
    const int64_t survivors = (int64_t)carry_s, landed = (int64_t)carry_l;
    int64_t emitted = c.emit ? c.emit_counts[0] : 0;
    if (emitted < 0)
      emitted = 0;
    const int64_t room = c.capacity - survivors;
    const int64_t appended = emitted < room ? emitted : room;
    c.table[0] = survivors + appended;
    c.table[1] = alive;
    c.table[2] = survivors;
    c.table[3] = landed;
    c.table[4] = landed < c.landed_capacity ? landed : c.landed_capacity;
    c.table[5] = alive - survivors - landed;
    c.table[6] = appended;
    c.table[7] = emitted - appended;
  }
}

// grid: stage 1's; item loop to table[1], then the append
__global__ __launch_bounds__(kParticleThreads) void k_particles_scatter(ParticleCall c)
{
#pragma clang fp contract(off)
  __shared__ uint32_t lds[kParticleWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t before = c.table[1], survivors = c.table[2], appended = c.table[6];
  const int64_t items = (before + kParticleItem - 1) / kParticleItem;
  const float4* __restrict__ src = reinterpret_cast<const float4*>(c.cur);
  float4* __restrict__ dst = reinterpret_cast<float4*>(c.next);
  float4* __restrict__ hit = reinterpret_cast<float4*>(c.landed_out);
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x)
  {
    const unsigned long long* b = c.ballots + (size_t)item * kParticleWaves * 2;
    if (tid < 2 * kParticleWaves)
      lds[tid >> 1][tid & 1] = (uint32_t)__popcll(b[tid]);
    const unsigned long long bs = b[2 * wave], bl = b[2 * wave + 1];
    __syncthreads();
    uint32_t rank_s = particle_rank(bs), rank_l = particle_rank(bl);
#pragma unroll
    for (int w = 0; w < kParticleWaves; w++)
    {
      rank_s += w < wave ? lds[w][0] : 0u;
      rank_l += w < wave ? lds[w][1] : 0u;
    }
    const bool survives = (bs >> lane) & 1ull, landed = (bl >> lane) & 1ull;
    if (survives || landed)  // only particles below table[1] have a bit
    {
      const int64_t idx = item * kParticleItem + tid;
      const float4 r0 = src[2 * idx], r1 = src[2 * idx + 1];
      if (survives)
      {
        const int64_t rec = c.offset[2 * item] + rank_s;  // < survivors <= capacity
        dst[2 * rec] = r0;
        dst[2 * rec + 1] = r1;
      }
      else
      {
        const int64_t rec = c.offset[2 * item + 1] + rank_l;
        if (rec < c.landed_capacity)
        {
          hit[2 * rec] = r0;
          hit[2 * rec + 1] = r1;
        }
      }
    }
    __syncthreads();
  }
  // the emitter's records after the survivors: survivors + appended <= capacity (k_particles_scan)
  const float4* __restrict__ emit = reinterpret_cast<const float4*>(c.emit);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + tid; e < appended; e += (int64_t)gridDim.x * blockDim.x)
  {
    const float4 r0 = emit[2 * e], r1 = emit[2 * e + 1];
    dst[2 * (survivors + e)] = make_float4(r0.x, r0.y, r0.z, 0.0f);
    dst[2 * (survivors + e) + 1] = make_float4(c.gain * r1.x, c.gain * r1.y + c.lift * r0.w, c.gain * r1.z, r1.w);
  }
}

// the table of a list that no step has made: `alive` records, every other count 0
__global__ void k_particles_reset(int64_t* table, int64_t alive)
{
  if (blockIdx.x == 0 && threadIdx.x < kParticleCounts)
    table[threadIdx.x] = threadIdx.x == 0 ? alive : 0;
}

}  // namespace oceanfft
