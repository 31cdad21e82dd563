// device/k_hulls.h — net wave force and torque on batches of floating bodies (ocean_hulls_loads,
// include/oceanfft.h): pose -> world point -> the query's fixed point on the vertex stage -> the water
// particle's velocity -> buoyancy + drag -> the fold over the body's points, in one pass.
//
// A work item is a tile of up to 64 consecutive points of one body (HullTile, built on the host at
// ocean_hulls_create), one wave per item, a lane per point; consecutive bodies of at most 32 points
// share a wave, each in an aligned power-of-two segment of its lanes, and fold within their segments. The fold is the contract's fold64: the xor
// butterfly with strides 32 -> 1, every lane adding its partner's value, so after the last step every lane
// holds a[0] of `for h in 32 .. 1: a = a[:h] + a[h:]` (fp32 addition is commutative, so which of a pair
// is "own" does not matter). Lanes past the tile's count carry +0.0f, the contract's padding. The
// exchanges stay in registers (xor_lane_pair, device/lane_xchg.h, shared with the minima and maxima of
// device/k_bounds.h): v_permlane32_swap / v_permlane16_swap for lane bits 5 and 4, bank-masked DPP row
// shifts for bits 3 and 2, quad_perm for bits 1 and 0. They read the registers of lanes whatever EXEC says, so they run outside every lane-dependent branch, with the
// whole wave active: the item loop and its bound are wave-uniform (one wave per workgroup, items dealt by
// blockIdx).
//
// The query loop is lane-divergent (a lane stops once its residual is within the tolerance): the wave runs
// until its last lane is done, as in k_surface_query. Only the vertex stage is evaluated; the hull loads
// use neither the normal nor the Jacobian.
//
// A one-tile body's fold is its loads. A body of T > 1 tiles writes T partials to the hull set's scratch,
// and k_hulls_fold (one workgroup per such body) folds them by the same rule: sum(a) for more than 64
// values is sum of the fold64s of consecutive runs of 64, so T <= 64 partials are one more fold64 and
// T <= 4096 (262144 points, the largest body) two more. No atomics, no dependence on the grid size: the
// same bits on every run.
#pragma once

#include <hip/hip_runtime.h>

#include "device/lane_xchg.h"
#include "device/surface_sample.h"
#include "device/wave_tile.h"

namespace oceanfft
{

constexpr int kHullTile = kHullTilePoints;  // one wave per work item, a lane per point
static_assert(kHullTile == 64, "the fold is a wave64 butterfly");
constexpr int kHullFoldThreads = 256;  // k_hulls_fold: four waves share a body's runs of 64 partials

// v + the value of lane (lane ^ STRIDE), in every lane
template <int STRIDE>
__device__ __forceinline__ float fold_step(float v)
{
#pragma clang fp contract(off)
  float a, b;
  xor_lane_pair<STRIDE>(v, a, b);
  return a + b;
}

// fold64 of the wave's 64 values, in every lane
__device__ __forceinline__ float wave_fold64(float v)
{
  v = fold_step<32>(v);
  v = fold_step<16>(v);
  v = fold_step<8>(v);
  v = fold_step<4>(v);
  v = fold_step<2>(v);
  return fold_step<1>(v);
}

// The same within aligned segments of `seg` lanes (a power of two, wave-uniform; 64: the whole wave): the
// steps of stride >= seg are left out. For a segment padded with +0.0f those steps add +0.0f, which changes
// at most the sign of a zero, so each segment's lanes hold the fold64 of the segment's values.
__device__ __forceinline__ float wave_fold_segments(float v, int seg)
{
  if (seg > 32)
    v = fold_step<32>(v);
  if (seg > 16)
    v = fold_step<16>(v);
  if (seg > 8)
    v = fold_step<8>(v);
  if (seg > 4)
    v = fold_step<4>(v);
  if (seg > 2)
    v = fold_step<2>(v);
  if (seg > 1)
    v = fold_step<1>(v);
  return v;
}

// HullTile, HullFold and HullCall: ocean_internal.h (the host builds the tables); HullLane: device/wave_tile.h
__device__ __forceinline__ HullLane hull_tile_lane(const HullCall& h, const HullTile& tile, int lane)
{
  return hull_tile_lane(h.bodies, tile, lane);
}

// One point's load (the contract's a_i) from its row L = (l0, l1) of the points and its body's pose P (R, c, v, w: the
// first 18 floats of a poses row), and its point_out rows when point_out is not null. P may be device memory (k_hulls_loads) or
// a pose kept in registers (k_hulls_step, device/k_hulls_step.h): the same expressions, the same bits.
template <bool ATLAS, bool VELOCITY>
__device__ __forceinline__ void hull_point_load(const SurfaceParams& p, const SurfaceRates& r, const HullCall& h,
                                                const float4 l0, const float4 l1, const float* P, int64_t row,
                                                float4* point_out, float (&a)[8])
{
#pragma clang fp contract(off)
  const float dx = (P[0] * l0.x + P[1] * l0.y) + P[2] * l0.z;
  const float dy = (P[3] * l0.x + P[4] * l0.y) + P[5] * l0.z;
  const float dz = (P[6] * l0.x + P[7] * l0.y) + P[8] * l0.z;
  const float xx = P[9] + dx, xy = P[10] + dy, xz = P[11] + dz;
  // ocean_surface_query at q = (xx, xz), vertex stage only
  float bx = xx, bz = xz;
  float vx, vy, vz;
  surface_base_point<ATLAS>(p, xx, xz, h.iterations, h.tolerance, bx, bz, vx, vy, vz);
  const float res = surface_residual(xx, xz, vx, vz);
  const float t = (vy - xy) / (l1.x + l1.x) + 0.5f;
  const float s = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;  // NaN -> 0
  float ux = 0.0f, uy = 0.0f, uz = 0.0f;
  if constexpr (VELOCITY)
  {
    float px = bx, py = 0.0f, pz = bz;
    surface_particle_velocity(p, r, px, py, pz, ux, uy, uz);
  }
  const float wx = P[15], wy = P[16], wz = P[17];
  const float vpx = P[12] + (wy * dz - wz * dy);
  const float vpy = P[13] + (wz * dx - wx * dz);
  const float vpz = P[14] + (wx * dy - wy * dx);
  const float rx = ux - vpx, ry = uy - vpy, rz = uz - vpz;
  const float m = sqrtf((rx * rx + ry * ry) + rz * rz);
  const float k = s * (l1.y + l1.z * m);
  const float vs = l0.w * s;
  const float fx = k * rx, fy = h.rho_g * vs + k * ry, fz = k * rz;
  a[0] = fx;
  a[1] = fy;
  a[2] = fz;
  a[3] = vs;
  a[4] = dy * fz - dz * fy;
  a[5] = dz * fx - dx * fz;
  a[6] = dx * fy - dy * fx;
  a[7] = s > 0.0f ? 1.0f : 0.0f;
  if (point_out)
  {
    point_out[2 * row] = make_float4(bx, vy, bz, res);
    point_out[2 * row + 1] = make_float4(fx, fy, fz, s);
  }
}

template <bool ATLAS, bool VELOCITY>
__global__ __launch_bounds__(kHullTile) void k_hulls_loads(SurfaceParams p, SurfaceRates r, HullCall h)
{
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  for (int item = blockIdx.x; item < h.items; item += gridDim.x)
  {
    const HullTile tile = h.tiles[item];
    const HullLane l = hull_tile_lane(h, tile, lane);
    float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (l.active)
      hull_point_load<ATLAS, VELOCITY>(p, r, h, h.points[2 * (size_t)l.point], h.points[2 * (size_t)l.point + 1],
                                       h.poses + (size_t)l.body * 20, l.row, h.point_out, a);
    const int seg = tile.seg > 0 ? tile.seg : kHullTile;  // wave-uniform
#pragma unroll
    for (int c = 0; c < 8; c++)
      a[c] = wave_fold_segments(a[c], seg);
    if ((lane & (seg - 1)) == 0 && l.active_segment)
    {
      float4* dst = tile.slot < 0 ? h.loads + 2 * (size_t)l.body : h.partial + 2 * (size_t)tile.slot;
      dst[0] = make_float4(a[0], a[1], a[2], a[3]);
      dst[1] = make_float4(a[4], a[5], a[6], a[7]);
    }
  }
}

// The partials of one body of more than one tile -> its loads, in a[] of wave 0 (the other waves' a[] is left
// alone). The whole workgroup calls it: wave w folds the runs w, w + 4, ... of 64 partials, run j's fold
// lands in slot j of the LDS, and when there is more than one run wave 0 folds those (at most 64).
__device__ __forceinline__ void hull_fold_partials(const HullFold& f, const float4* __restrict__ partial,
                                                   float (*runs)[8], int lane, int wave, float (&out)[8])
{
#pragma clang fp contract(off)
  const int nruns = (f.tiles + 63) >> 6;  // <= 64
  // the bound depends on the wave alone: every lane of a wave runs the same steps (whole-wave exchanges)
  for (int j = wave; j < nruns; j += kHullFoldThreads / 64)
  {
    const int t = j * 64 + lane;
    float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (t < f.tiles)
    {
      const float4 lo = partial[2 * (size_t)(f.slot + t)], hi = partial[2 * (size_t)(f.slot + t) + 1];
      a[0] = lo.x, a[1] = lo.y, a[2] = lo.z, a[3] = lo.w;
      a[4] = hi.x, a[5] = hi.y, a[6] = hi.z, a[7] = hi.w;
    }
#pragma unroll
    for (int c = 0; c < 8; c++)
      a[c] = wave_fold64(a[c]);
    if (lane < 8)
    {
      float v = a[0];
#pragma unroll
      for (int c = 1; c < 8; c++)
        v = lane == c ? a[c] : v;
      runs[j][lane] = v;
    }
  }
  __syncthreads();
  if (wave == 0)
  {
#pragma unroll
    for (int c = 0; c < 8; c++)
      out[c] = lane < nruns ? runs[lane][c] : 0.0f;
    if (nruns > 1)  // uniform over the workgroup
    {
#pragma unroll
      for (int c = 0; c < 8; c++)
        out[c] = wave_fold64(out[c]);
    }
  }
}

// The bodies of more than one tile: one workgroup per body (hull_fold_partials), its lane 0 writes the loads.
__global__ __launch_bounds__(kHullFoldThreads) void k_hulls_fold(const HullFold* __restrict__ folds, int count,
                                                                const float4* __restrict__ partial,
                                                                float4* __restrict__ loads)
{
#pragma clang fp contract(off)
  __shared__ float runs[64][8];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int item = blockIdx.x; item < count; item += gridDim.x)
  {
    const HullFold f = folds[item];
    float a[8];
    hull_fold_partials(f, partial, runs, lane, wave, a);
    if (wave == 0 && lane == 0)
    {
      loads[2 * (size_t)f.body] = make_float4(a[0], a[1], a[2], a[3]);
      loads[2 * (size_t)f.body + 1] = make_float4(a[4], a[5], a[6], a[7]);
    }
    __syncthreads();  // the LDS is rewritten by the next body
  }
}

}  // namespace oceanfft
