// device/k_mips.h — the mip pyramid of a generator's maps (ocean_generator_build_mips): the box filter of
// glGenerateMipmap, per channel in fp32,
//     L[l+1](x, y) = 0.25f * ((L[l](2x, 2y) + L[l](2x+1, 2y)) + (L[l](2x, 2y+1) + L[l](2x+1, 2y+1))),
// each level from the rounded level below it. One launch writes six levels: a workgroup of 256 threads
// takes a 64 x 64 tile of the source level of one cascade, all three maps (9 floats per texel). A lane
// holds one column of 16 rows (device/mip_index.h), so a load instruction of a wave reads one contiguous
// 64-texel row span. Halvings 1-4 add the horizontal neighbour through a DPP row shift (lane + 1, 2, 4,
// 8, always inside the lane's row of 16) and the vertical one in registers: no LDS, no barrier. The
// 4 x 4 values per channel that remain cross the four waves through 720 B of LDS for halvings 5 and 6.
// The sum order above is kept at every halving, so the bits do not depend on the fusion.
// Clipping: a source level smaller than the tile (N = 16, 32; the 2 x 2, 4 x 4, 64 x 64 sources of the
// later launches) is one tile whose out-of-range loads are replaced by 0 and whose out-of-range stores
// are skipped; an in-range texel of any level depends on in-range texels only. Every lane stays active
// through the cross-lane reads (the predicates guard loads and stores, never the arithmetic).
#pragma once

#include <hip/hip_runtime.h>

#include "device/lane_xchg.h"
#include "device/mip_index.h"

namespace oceanfft
{

struct MipBuild
{
  const float* src[3];   // cascade 0's source level of heightMap, displacementMap, jacobian
  size_t src_stride[3];  // floats between cascades
  float* dst[3];         // cascade 0's chains (device/mip_index.h)
  size_t dst_stride;     // floats between cascades
  int n;                 // side of level 0
  int level;             // the source level: 0, 6, 12
  int top;               // log2 n
};

// Halving J of a lane's column: rows (2r, 2r + 1) and the partner lane's -> row r.
template <int C, int J>
__device__ __forceinline__ void mip_halve(float (&v)[kMipRowsPerWave][C])
{
#pragma clang fp contract(off)
  constexpr int SH = 1 << (J - 1);
#pragma unroll
  for (int r = 0; r < (kMipRowsPerWave >> J); r++)
#pragma unroll
    for (int c = 0; c < C; c++)
    {
      const float a = v[2 * r][c], b = v[2 * r + 1][c];
      const float upper = a + dpp_update<0x100 + SH, 0xF>(a, a);  // (2x, 2y) + (2x+1, 2y)
      const float lower = b + dpp_update<0x100 + SH, 0xF>(b, b);  // (2x, 2y+1) + (2x+1, 2y+1)
      v[r][c] = 0.25f * (upper + lower);
    }
}

template <int C, int J>
__device__ __forceinline__ void mip_store(const float (&v)[kMipRowsPerWave][C], float* __restrict__ chain,
                                          const MipBuild& m, int tx, int ty, int tid)
{
  const int l = m.level + J, side = (m.n >> m.level) >> J;
  if (l > m.top || !mip_lane_holds(tid, J))
    return;
  const int x = mip_dst_x(tx, tid, J);
  float* __restrict__ img = chain + mip_level_offset(m.n, l) * C;
#pragma unroll
  for (int r = 0; r < (kMipRowsPerWave >> J); r++)
  {
    const int y = mip_dst_y(ty, tid, J, r);
    if (x < side && y < side)
    {
      float* q = img + ((size_t)y * side + x) * C;
      if constexpr (C == 4)
        *reinterpret_cast<float4*>(q) = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
      else
        *q = v[r][0];
    }
  }
}

// One map of C floats per texel: halvings 1-4 of the tile, the 4 x 4 remainder into lds[c][16].
template <int C>
__device__ __forceinline__ void mip_tile_map(const float* __restrict__ src, float* __restrict__ chain,
                                             const MipBuild& m, int tx, int ty, int tid, float (*lds)[16])
{
  const int s = m.n >> m.level;
  float v[kMipRowsPerWave][C];
  const int x = mip_src_x(tx, tid);
#pragma unroll
  for (int k = 0; k < kMipRowsPerWave; k++)
  {
    const int y = mip_src_y(ty, tid, k);
    const bool in = x < s && y < s;
    if constexpr (C == 4)
    {
      const float4 q = in ? *reinterpret_cast<const float4*>(src + ((size_t)y * s + x) * 4) : make_float4(0, 0, 0, 0);
      v[k][0] = q.x;
      v[k][1] = q.y;
      v[k][2] = q.z;
      v[k][3] = q.w;
    }
    else
      v[k][0] = in ? src[(size_t)y * s + x] : 0.0f;
  }
  mip_halve<C, 1>(v);
  mip_store<C, 1>(v, chain, m, tx, ty, tid);
  mip_halve<C, 2>(v);
  mip_store<C, 2>(v, chain, m, tx, ty, tid);
  mip_halve<C, 3>(v);
  mip_store<C, 3>(v, chain, m, tx, ty, tid);
  mip_halve<C, 4>(v);
  mip_store<C, 4>(v, chain, m, tx, ty, tid);
  if (mip_lane_holds(tid, kMipLaneLevels))
#pragma unroll
    for (int c = 0; c < C; c++)
      lds[c][mip_lds_slot(tid)] = v[0][c];
}

// grid: (tiles, tiles, cascades) of the source level
__global__ __launch_bounds__(256) void k_mips(MipBuild m)
{
#pragma clang fp contract(off)
  __shared__ float l4[9][16];  // channel (heightMap 0-3, displacementMap 4-7, jacobian 8) x level-4 texel (y * 4 + x)
  __shared__ float l5[9][4];
  const int tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y, cas = blockIdx.z;
  mip_tile_map<4>(m.src[0] + cas * m.src_stride[0], m.dst[0] + cas * m.dst_stride, m, tx, ty, tid, l4);
  mip_tile_map<4>(m.src[1] + cas * m.src_stride[1], m.dst[1] + cas * m.dst_stride, m, tx, ty, tid, l4 + 4);
  mip_tile_map<1>(m.src[2] + cas * m.src_stride[2], m.dst[2] + cas * m.dst_stride, m, tx, ty, tid, l4 + 8);
  __syncthreads();
  // halvings 5 (2 x 2 per tile and channel) and 6 (1): thread -> (channel, texel)
  const int ch = tid >> 2, q = tid & 3, qx = q & 1, qy = q >> 1;
  // the chain, the floats per texel and the lane of channel ch
  const int map = ch < 4 ? 0 : (ch < 8 ? 1 : 2), cpt = ch < 8 ? 4 : 1, sub = ch < 8 ? (ch & 3) : 0;
  if (ch < 9)
  {
    const float* a = l4[ch];
    const int o = 8 * qy + 2 * qx;
    const float val = 0.25f * ((a[o] + a[o + 1]) + (a[o + 4] + a[o + 5]));
    l5[ch][q] = val;
    const int l = m.level + 5, side = (m.n >> m.level) >> 5;
    const int x = tx * 2 + qx, y = ty * 2 + qy;
    if (l <= m.top && x < side && y < side)
      (m.dst[map] + cas * m.dst_stride)[(mip_level_offset(m.n, l) + (size_t)y * side + x) * cpt + sub] = val;
  }
  __syncthreads();
  if (ch < 9 && q == 0)
  {
    const float* a = l5[ch];
    const float val = 0.25f * ((a[0] + a[1]) + (a[2] + a[3]));
    const int l = m.level + 6, side = (m.n >> m.level) >> 6;
    if (l <= m.top && tx < side && ty < side)
      (m.dst[map] + cas * m.dst_stride)[(mip_level_offset(m.n, l) + (size_t)ty * side + tx) * cpt + sub] = val;
  }
}

}  // namespace oceanfft
