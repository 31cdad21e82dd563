// device/k_hulls_step.h — hull dynamics (ocean_hulls_step, include/oceanfft.h): the bodies of a hull set
// stepped on the device from their wave loads. Per substep: the loads of device/k_hulls.h at the current pose
// (hull_point_load and the same folds: the same bits as ocean_hulls_loads), then a semi-implicit Euler step of
// the velocities, the centre, and the rotation by the Cayley map with one Gram-Schmidt pass (hull_integrate,
// the header's contract expression by expression, unfused fp32).
//
// The water is frozen during a call and the bodies do not interact, so a body of one tile (at most 64
// points) belongs to one wave, or one segment of a wave, from the first substep to the last. k_hulls_step
// keeps such a body's pose in the registers of its segment's lanes and loops over the substeps: the leader
// lane of the segment integrates after the fold, inside `if (leader)`, and the new pose reaches the segment's
// lanes by lane reads (ds_bpermute from the leader lane), which, like the folds, run outside every
// lane-dependent branch with the whole wave active. The item loop and the substep loop have wave-uniform
// bounds (one wave per workgroup, items dealt by blockIdx). A set with no larger body is one launch per call.
//
// A set that holds a body of more than one tile takes two launches per substep: k_hulls_step with one substep
// per launch, in which the one-tile bodies integrate as above and the tiles of the larger bodies write their
// partials, then k_hulls_step_fold, in which lane 0 of a larger body's workgroup integrates after the last
// fold.
//
// Updating the poses in place is safe: only the owner of a body writes its pose. A one-tile body's pose is
// read and written by the lanes of its own segment alone, which read it before the substep loop and write it
// after. The tiles of a multi-tile body read its pose in k_hulls_step, the launch before the k_hulls_step_fold
// that writes it, and the next substep's k_hulls_step follows that on the stream. No work item reads another
// body's pose.
//
// loads and point_out are written in the call's last substep only (HullStep::last and the last substep of
// the launch), so they hold what ocean_hulls_loads returns for the pose at the start of that substep.
#pragma once

#include <hip/hip_runtime.h>

#include "device/k_hulls.h"

namespace oceanfft
{

// One substep of one body from its loads a[] (the fold of hull_point_load's terms): P[0..17] = R, c, v, w
// is replaced by the stepped pose. include/oceanfft.h, "Hull dynamics", states every expression in this order.
__device__ __forceinline__ void hull_integrate(float (&P)[18], const float (&a)[8], const HullStep& st, int body)
{
#pragma clang fp contract(off)
  const float4 m = st.props[2 * (size_t)body], d = st.props[2 * (size_t)body + 1];
  const float h = st.h;
  float fx = a[0], fy = a[1], fz = a[2], tx = a[4], ty = a[5], tz = a[6];
  if (st.ext)
  {
    const float4 e0 = st.ext[2 * (size_t)body], e1 = st.ext[2 * (size_t)body + 1];
    fx = fx + e0.x, fy = fy + e0.y, fz = fz + e0.z;
    tx = tx + e1.x, ty = ty + e1.y, tz = tz + e1.z;
  }
  float vx = P[12], vy = P[13], vz = P[14], wx = P[15], wy = P[16], wz = P[17];
  if (d.z == 0.0f)  // dynamic
  {
    const float kl = 1.0f + h * d.x, ka = 1.0f + h * d.y;
    vx = (vx + h * (fx / m.x + st.gx)) / kl;
    vy = (vy + h * (fy / m.x + st.gy)) / kl;
    vz = (vz + h * (fz / m.x + st.gz)) / kl;
    // the body frame: the columns of R
    const float bx = (P[0] * wx + P[3] * wy) + P[6] * wz;
    const float by = (P[1] * wx + P[4] * wy) + P[7] * wz;
    const float bz = (P[2] * wx + P[5] * wy) + P[8] * wz;
    const float sx = (P[0] * tx + P[3] * ty) + P[6] * tz;
    const float sy = (P[1] * tx + P[4] * ty) + P[7] * tz;
    const float sz = (P[2] * tx + P[5] * ty) + P[8] * tz;
    const float lx = m.y * bx, ly = m.z * by, lz = m.w * bz;
    const float gx = by * lz - bz * ly, gy = bz * lx - bx * lz, gz = bx * ly - by * lx;
    const float ox = (bx + h * ((sx - gx) / m.y)) / ka;
    const float oy = (by + h * ((sy - gy) / m.z)) / ka;
    const float oz = (bz + h * ((sz - gz) / m.w)) / ka;
    wx = (P[0] * ox + P[1] * oy) + P[2] * oz;
    wy = (P[3] * ox + P[4] * oy) + P[5] * oz;
    wz = (P[6] * ox + P[7] * oy) + P[8] * oz;
  }
  const float cx = P[9] + h * vx, cy = P[10] + h * vy, cz = P[11] + h * vz;
  // the Cayley map of a = (h / 2) w
  const float hh = 0.5f * h;
  const float ax = hh * wx, ay = hh * wy, az = hh * wz;
  const float n = (ax * ax + ay * ay) + az * az;
  const float p = 1.0f - n, q = 1.0f + n;
  const float xy = 2.0f * (ax * ay), xz = 2.0f * (ax * az), yz = 2.0f * (ay * az);
  const float ux = 2.0f * ax, uy = 2.0f * ay, uz = 2.0f * az;
  const float q00 = (p + 2.0f * (ax * ax)) / q, q01 = (xy - uz) / q, q02 = (xz + uy) / q;
  const float q10 = (xy + uz) / q, q11 = (p + 2.0f * (ay * ay)) / q, q12 = (yz - ux) / q;
  const float q20 = (xz - uy) / q, q21 = (yz + ux) / q, q22 = (p + 2.0f * (az * az)) / q;
  float r[9];
#pragma unroll
  for (int j = 0; j < 3; j++)
  {
    r[j] = (q00 * P[j] + q01 * P[3 + j]) + q02 * P[6 + j];
    r[3 + j] = (q10 * P[j] + q11 * P[3 + j]) + q12 * P[6 + j];
    r[6 + j] = (q20 * P[j] + q21 * P[3 + j]) + q22 * P[6 + j];
  }
  // one Gram-Schmidt pass over the rows
  const float l0 = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  const float e0x = r[0] / l0, e0y = r[1] / l0, e0z = r[2] / l0;
  const float dd = (e0x * r[3] + e0y * r[4]) + e0z * r[5];
  const float u1x = r[3] - dd * e0x, u1y = r[4] - dd * e0y, u1z = r[5] - dd * e0z;
  const float l1 = sqrtf((u1x * u1x + u1y * u1y) + u1z * u1z);
  const float e1x = u1x / l1, e1y = u1y / l1, e1z = u1z / l1;
  P[0] = e0x, P[1] = e0y, P[2] = e0z;
  P[3] = e1x, P[4] = e1y, P[5] = e1z;
  P[6] = e0y * e1z - e0z * e1y;
  P[7] = e0z * e1x - e0x * e1z;
  P[8] = e0x * e1y - e0y * e1x;
  P[9] = cx, P[10] = cy, P[11] = cz;
  P[12] = vx, P[13] = vy, P[14] = vz;
  P[15] = wx, P[16] = wy, P[17] = wz;
}

__device__ __forceinline__ void hull_load_pose(const float* src, float (&P)[18])
{
#pragma unroll
  for (int k = 0; k < 18; k++)
    P[k] = src[k];
}

__device__ __forceinline__ void hull_store_pose(float* dst, const float (&P)[18])
{
#pragma unroll
  for (int k = 0; k < 18; k++)
    dst[k] = P[k];
  dst[18] = 0.0f;
  dst[19] = 0.0f;
}

// st.substeps substeps of the bodies of one tile; the tiles of larger bodies (tile.slot >= 0, only with
// st.substeps == 1) write their partials for k_hulls_step_fold.
template <bool ATLAS, bool VELOCITY>
__global__ __launch_bounds__(kHullTile) void k_hulls_step(SurfaceParams p, SurfaceRates r, HullCall h, HullStep st)
{
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  for (int item = blockIdx.x; item < h.items; item += gridDim.x)
  {
    const HullTile tile = h.tiles[item];
    const HullLane l = hull_tile_lane(h, tile, lane);
    const int seg = tile.seg > 0 ? tile.seg : kHullTile;  // wave-uniform
    const bool owner = tile.slot < 0;                     // wave-uniform: the tile's bodies have no other tile
    const bool leader = (lane & (seg - 1)) == 0 && l.active_segment;
    float P[18];
    float4 l0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), l1 = l0;
    if (l.active_segment)
      hull_load_pose(st.poses + (size_t)l.body * 20, P);
    else
    {
#pragma unroll
      for (int k = 0; k < 18; k++)
        P[k] = 0.0f;
    }
    if (l.active)
    {
      l0 = h.points[2 * (size_t)l.point];
      l1 = h.points[2 * (size_t)l.point + 1];
    }
    for (int s = 0; s < st.substeps; s++)
    {
      const bool out = st.last != 0 && s == st.substeps - 1;  // wave-uniform
      float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (l.active)
        hull_point_load<ATLAS, VELOCITY>(p, r, h, l0, l1, P, l.row, out ? h.point_out : nullptr, a);
#pragma unroll
      for (int c = 0; c < 8; c++)
        a[c] = wave_fold_segments(a[c], seg);
      if (leader)
      {
        float4* dst = owner ? (out && h.loads ? h.loads + 2 * (size_t)l.body : nullptr)
                            : h.partial + 2 * (size_t)tile.slot;
        if (dst)
        {
          dst[0] = make_float4(a[0], a[1], a[2], a[3]);
          dst[1] = make_float4(a[4], a[5], a[6], a[7]);
        }
        if (owner)
          hull_integrate(P, a, st, l.body);
      }
      if (owner && s + 1 < st.substeps)  // wave-uniform: the leader's pose to its segment's lanes
      {
        const int src = lane & ~(seg - 1);
#pragma unroll
        for (int k = 0; k < 18; k++)
          P[k] = __shfl(P[k], src);
      }
    }
    if (leader && owner)
      hull_store_pose(st.poses + (size_t)l.body * 20, P);
  }
}

// The bodies of more than one tile: k_hulls_fold's fold of the partials, then lane 0 integrates the body.
// loads is null except in the call's last substep.
__global__ __launch_bounds__(kHullFoldThreads) void k_hulls_step_fold(const HullFold* __restrict__ folds, int count,
                                                                     const float4* __restrict__ partial,
                                                                     float4* __restrict__ loads, HullStep st)
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
      if (loads)
      {
        loads[2 * (size_t)f.body] = make_float4(a[0], a[1], a[2], a[3]);
        loads[2 * (size_t)f.body + 1] = make_float4(a[4], a[5], a[6], a[7]);
      }
      float P[18];
      hull_load_pose(st.poses + (size_t)f.body * 20, P);
      hull_integrate(P, a, st, f.body);
      hull_store_pose(st.poses + (size_t)f.body * 20, P);
    }
    __syncthreads();  // the LDS is rewritten by the next body
  }
}

}  // namespace oceanfft
