// device/k_moorings.h — mooring lines (ocean_moorings_step, include/oceanfft.h): lumped-mass cable chains
// stepped on the device, and the wrench they put on the bodies of a hull set.
//
// A work item is one wave and a lane is one node. The items are k_hulls.h's (HullTile / HullBody with "body"
// read as line and "point" as node, hull_tile_lane of device/wave_tile.h): a line of 33 .. 64 nodes has a wave
// of its own, consecutive lines of at most 32 nodes share a wave in aligned power-of-two segments. A line's
// positions, velocities and the running sum of its fairlead force stay in its lanes' registers from the first
// substep to the last: one launch per call whatever `substeps` is, no global or LDS round trip in between.
//
// Per substep a node needs its neighbours: segment j (between nodes j and j + 1, kept by lane j) reads node
// j + 1's position and velocity, and node i reads segment i - 1's pull. Both are lane shifts inside the segment
// (segment_shift, device/lane_xchg.h), six values down and three up. They read the registers of lanes whatever
// EXEC says, so, by the rule at the top of k_hulls.h, they run outside every lane-dependent branch with the
// whole wave active: the item loop and the substep loop have wave-uniform bounds (one wave per workgroup, items
// dealt by blockIdx). The water query's fixed-point loop is lane-divergent (water_point_kinematics,
// device/k_kinematics.h): the shifts come before it and the folds after the last substep. The largest tension
// is the max fold of k_bounds.h (bounds_fold_step) over the segment's lanes, the wet and bed counts a wave
// ballot masked to the segment. No atomics: the same bits on every run, for every grid size.
//
// The fairleads are frozen during a call (the poses are read once), so lines do not interact and the bodies'
// wrenches are a second, small launch: k_moorings_wrench, one lane per body, walks the body's lines in
// ascending index (a CSR built at create) and sums their mean fairlead forces and the torques d x Fm.
#pragma once

#include <hip/hip_runtime.h>

#include "device/k_kinematics.h"
#include "device/wave_tile.h"

namespace oceanfft
{

static_assert(kMooringMaxNodes == 64, "one lane per node, one wave per line");

// max of the values of a segment's lanes (all >= 0; lanes past the line carry 0), in every lane: the steps of
// wave_fold_segments (k_hulls.h) with k_bounds.h's max
__device__ __forceinline__ float wave_max_segments(float v, int seg)
{
  if (seg > 32)
    v = bounds_fold_step<32, true>(v);
  if (seg > 16)
    v = bounds_fold_step<16, true>(v);
  if (seg > 8)
    v = bounds_fold_step<8, true>(v);
  if (seg > 4)
    v = bounds_fold_step<4, true>(v);
  if (seg > 2)
    v = bounds_fold_step<2, true>(v);
  if (seg > 1)
    v = bounds_fold_step<1, true>(v);
  return v;
}

// The fairlead of a line from its body's pose (P: R, c, v, w): the arm d = R Lf, the world position and its
// velocity, ocean_hulls_loads' expressions (hull_point_load, device/k_hulls.h). body < 0: d = 0, the position Lf.
struct Fairlead
{
  float dx, dy, dz, x, y, z, vx, vy, vz;
};

__device__ __forceinline__ Fairlead mooring_fairlead(const MooringLine& ln, const float* poses)
{
#pragma clang fp contract(off)
  Fairlead f{0.0f, 0.0f, 0.0f, ln.f.x, ln.f.y, ln.f.z, 0.0f, 0.0f, 0.0f};
  if (ln.body >= 0)
  {
    const float* P = poses + (size_t)ln.body * 20;
    f.dx = (P[0] * ln.f.x + P[1] * ln.f.y) + P[2] * ln.f.z;
    f.dy = (P[3] * ln.f.x + P[4] * ln.f.y) + P[5] * ln.f.z;
    f.dz = (P[6] * ln.f.x + P[7] * ln.f.y) + P[8] * ln.f.z;
    f.x = P[9] + f.dx, f.y = P[10] + f.dy, f.z = P[11] + f.dz;
    const float wx = P[15], wy = P[16], wz = P[17];
    f.vx = P[12] + (wy * f.dz - wz * f.dy);
    f.vy = P[13] + (wz * f.dx - wx * f.dz);
    f.vz = P[14] + (wx * f.dy - wy * f.dx);
  }
  return f;
}

// ocean_moorings_reset: every line's nodes on the straight segment from its anchor to its fairlead, at rest.
__global__ __launch_bounds__(kMooringMaxNodes) void k_moorings_reset(MooringCall m)
{
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  for (int item = blockIdx.x; item < m.items; item += gridDim.x)
  {
    const HullTile tile = m.tiles[item];
    const HullLane l = hull_tile_lane(m.table, tile, lane);
    if (!l.active)
      continue;
    const int seg = tile.seg > 0 ? tile.seg : kMooringMaxNodes;
    const int i = lane & (seg - 1);
    const MooringLine ln = m.lines[l.body];
    const Fairlead f = mooring_fairlead(ln, m.poses);
    const float t = (float)i / (float)(ln.nodes - 1);
    m.nodes[2 * l.row] =
        make_float4(ln.a.x + t * (f.x - ln.a.x), ln.a.y + t * (f.y - ln.a.y), ln.a.z + t * (f.z - ln.a.z), 0.0f);
    m.nodes[2 * l.row + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// m.substeps substeps of the lines of one work item; include/oceanfft.h, "Mooring lines", states every
// expression in this order.
template <bool WATER>
__global__ __launch_bounds__(kMooringMaxNodes) void k_moorings_step(SurfaceParams p, WaterLayers w, MooringCall m)
{
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  for (int item = blockIdx.x; item < m.items; item += gridDim.x)
  {
    const HullTile tile = m.tiles[item];
    const HullLane l = hull_tile_lane(m.table, tile, lane);
    const int seg = tile.seg > 0 ? tile.seg : kMooringMaxNodes;  // wave-uniform
    const int i = lane & (seg - 1);
    MooringLine ln{};
    if (l.active_segment)
      ln = m.lines[l.body];
    const int n = ln.nodes;
    const bool first = l.active && i == 0, last = l.active && i == n - 1;
    const bool interior = l.active && !first && !last;
    const bool segment = l.active && i < n - 1;  // the lane keeps the segment from its node to the next
    const float l0 = ln.a.w, ea = ln.f.w, ca = ln.c.x, mn = ln.c.y, vn = ln.c.z, dl = ln.c.w, dq = ln.dq;
    const float kb = m.bed_k * l0, cb = m.bed_c * l0;
    float x = 0.0f, y = 0.0f, z = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f;
    if (interior)
    {
      const float4 r0 = m.nodes[2 * l.row], r1 = m.nodes[2 * l.row + 1];
      x = r0.x, y = r0.y, z = r0.z;
      vx = r1.x, vy = r1.y, vz = r1.z;
    }
    if (first)
      x = ln.a.x, y = ln.a.y, z = ln.a.z;
    if (last)
    {
      const Fairlead f = mooring_fairlead(ln, m.poses);
      x = f.x, y = f.y, z = f.z;
      vx = f.vx, vy = f.vy, vz = f.vz;
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;  // the running sum of -(T e) of the lane's segment
    float T = 0.0f;
    bool wet = false, bed = false;
    for (int s = 0; s < m.substeps; s++)
    {
      // node i + 1 to lane i: the whole wave is active
      const float nx = segment_shift<1>(x, lane, seg), ny = segment_shift<1>(y, lane, seg);
      const float nz = segment_shift<1>(z, lane, seg);
      const float nvx = segment_shift<1>(vx, lane, seg), nvy = segment_shift<1>(vy, lane, seg);
      const float nvz = segment_shift<1>(vz, lane, seg);
      float ex = 0.0f, ey = 0.0f, ez = 0.0f;
      T = 0.0f;
      if (segment)
      {
        const float dx = nx - x, dy = ny - y, dz = nz - z;
        const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
        ex = len > 0.0f ? dx / len : 0.0f;
        ey = len > 0.0f ? dy / len : 0.0f;
        ez = len > 0.0f ? dz / len : 0.0f;
        const float strain = (len - l0) / l0;
        const float rate = ((((nvx - vx) * ex + (nvy - vy) * ey) + (nvz - vz) * ez)) / l0;
        const float t = ea * strain + ca * rate;
        T = t > 0.0f ? t : 0.0f;  // no compression, NaN -> 0
      }
      const float tx = T * ex, ty = T * ey, tz = T * ez;
      // segment i - 1's pull to lane i: the whole wave is active
      const float qx = segment_shift<-1>(tx, lane, seg), qy = segment_shift<-1>(ty, lane, seg);
      const float qz = segment_shift<-1>(tz, lane, seg);
      sx = sx + (-tx), sy = sy + (-ty), sz = sz + (-tz);
      wet = false, bed = false;
      if (interior)
      {
        float ux = 0.0f, uy = 0.0f, uz = 0.0f;
        if constexpr (WATER)
        {
          const WaterPoint q = water_point_kinematics(p, w, x, y, z, m.iterations, m.tolerance);
          ux = q.ux, uy = q.uy, uz = q.uz;
          wet = q.wet;
        }
        else
          wet = 0.0f - y > 0.0f;
        const float rx = ux - vx, ry = uy - vy, rz = uz - vz;
        const float mag = sqrtf((rx * rx + ry * ry) + rz * rz);
        const float k = wet ? dl + dq * mag : 0.0f;
        float fx = ((tx - qx) + k * rx) + mn * m.gx;
        float fy = ((ty - qy) + k * ry) + mn * m.gy;
        float fz = ((tz - qz) + k * rz) + mn * m.gz;
        if (wet)
          fy = fy + m.rho_g * vn;
        const float pen = m.bed_y - y;
        if (pen > 0.0f)
        {
          fy = fy + kb * pen;
          fx = fx - cb * vx, fy = fy - cb * vy, fz = fz - cb * vz;
          bed = true;
        }
        vx = vx + m.h * (fx / mn), vy = vy + m.h * (fy / mn), vz = vz + m.h * (fz / mn);
        x = x + m.h * vx, y = y + m.h * vy, z = z + m.h * vz;
      }
    }
    // the last substep's tensions and flags, folded over the line: the whole wave is active
    const float tmax = wave_max_segments(T, seg);
    const unsigned long long mask = (seg == kMooringMaxNodes ? ~0ull : (1ull << seg) - 1ull) << (lane & ~(seg - 1));
    const float wets = (float)__popcll(__ballot(wet) & mask), beds = (float)__popcll(__ballot(bed) & mask);
    if (l.active)
    {
      m.nodes[2 * l.row] = make_float4(x, y, z, T);
      m.nodes[2 * l.row + 1] = make_float4(vx, vy, vz, (wet ? 1.0f : 0.0f) + (bed ? 2.0f : 0.0f));
    }
    if (segment && i == n - 2)  // the fairlead segment
    {
      const float4 fm = make_float4(sx / m.fsubsteps, sy / m.fsubsteps, sz / m.fsubsteps, T);
      m.fm[l.body] = fm;
      if (m.line_out)
        m.line_out[2 * (size_t)l.body] = fm;
    }
    if (first && m.line_out)  // the anchor segment
      m.line_out[2 * (size_t)l.body + 1] = make_float4(T, tmax, beds, wets);
  }
}

// wrench_ext: one lane per body sums its lines' mean fairlead forces and their torques about the centre, from
// +0.0f in ascending line index; bodies without a line get zeros.
__global__ __launch_bounds__(256) void k_moorings_wrench(MooringWrench q)
{
#pragma clang fp contract(off)
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < q.bodies; b += gridDim.x * blockDim.x)
  {
    const int lo = q.start[b], hi = q.start[b + 1];
    float fx = 0.0f, fy = 0.0f, fz = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f;
    for (int j = lo; j < hi; j++)
    {
      const int li = q.order[j];
      const float4 fm = q.fm[li];
      const Fairlead f = mooring_fairlead(q.lines[li], q.poses);
      fx = fx + fm.x, fy = fy + fm.y, fz = fz + fm.z;
      tx = tx + (f.dy * fm.z - f.dz * fm.y);
      ty = ty + (f.dz * fm.x - f.dx * fm.z);
      tz = tz + (f.dx * fm.y - f.dy * fm.x);
    }
    q.out[2 * (size_t)b] = make_float4(fx, fy, fz, (float)(hi - lo));
    q.out[2 * (size_t)b + 1] = make_float4(tx, ty, tz, 0.0f);
  }
}

}  // namespace oceanfft
