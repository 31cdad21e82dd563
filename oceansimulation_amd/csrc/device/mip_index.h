// device/mip_index.h — the index arithmetic of the mip pyramid (k_mips.h, the LOD surface stages, the
// C ABI's getters) as plain constexpr functions: no HIP types, so tools/mips_index_check.cpp walks the
// same code on the host for every N and asserts that no load, store or lane partner leaves its level.
//
// Storage. A map's levels 1 .. top (top = log2 N) are one "chain": level l is a row-major image of side
// N >> l at mip_level_offset(N, l) texels, (N^2 - 1) / 3 texels in all, padded to a multiple of 4 so
// that every level of every chain starts on 16 B. A cascade holds three chains back to back: heightMap
// (float4 texels), displacementMap (float4), jacobian (float) = 9 * mip_chain_texels(N) floats.
//
// The downsampler's tile. One workgroup of 256 threads takes a 64 x 64 tile of a source level of side
// S: lane q of wave w holds the column x = q of the tile's rows 16 w .. 16 w + 15, so each of its 16
// load instructions covers one 64-texel row span (1 KB of an RGBA32F map). After j halvings (j = 1 .. 4)
// the lanes whose low j bits are 0 hold 16 >> j rows of column q >> j of the tile's level-j image; the
// horizontal partner of halving j is lane q + (1 << (j - 1)), inside the lane's row of 16. The 4 x 4
// values left after four halvings go through the LDS for the last two.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define OCEAN_MIP_HD __host__ __device__
#else
#define OCEAN_MIP_HD
#endif

namespace oceanfft
{

constexpr int kMipTile = 64;         // source texels per tile side
constexpr int kMipFused = 6;         // levels one launch writes
constexpr int kMipLaneLevels = 4;    // of which in registers + across lanes
constexpr int kMipRowsPerWave = 16;  // source rows a lane holds

// texels of levels 1 .. log2 n of one map, padded to 16 B for the R32F chain
OCEAN_MIP_HD constexpr size_t mip_chain_texels(int n) { return ((((size_t)n * n - 1) / 3) + 3) & ~(size_t)3; }

// texel offset of level l >= 1 in its chain: the sum of (n >> k)^2 for k = 1 .. l - 1
OCEAN_MIP_HD constexpr size_t mip_level_offset(int n, int l)
{
  return ((size_t)n * n - (size_t)(n >> (l - 1)) * (size_t)(n >> (l - 1))) / 3;
}

// launches of one build: source levels 0, 6, 12
OCEAN_MIP_HD constexpr int mip_launches(int top) { return (top + kMipFused - 1) / kMipFused; }

// tiles per side of a source level of side s
OCEAN_MIP_HD constexpr int mip_tiles(int s) { return s >= kMipTile ? s / kMipTile : 1; }

// source texel of load k (0 .. 15) of thread tid in tile (tx, ty)
OCEAN_MIP_HD constexpr int mip_src_x(int tx, int tid) { return tx * kMipTile + (tid & 63); }
OCEAN_MIP_HD constexpr int mip_src_y(int ty, int tid, int k) { return ty * kMipTile + (tid >> 6) * kMipRowsPerWave + k; }

// After halving j (1 .. 4): does the lane hold values, which lane was its partner, and where do its
// rows r = 0 .. (16 >> j) - 1 go in the level-j image of the source (side s >> j)
OCEAN_MIP_HD constexpr bool mip_lane_holds(int tid, int j) { return ((tid & 63) & ((1 << j) - 1)) == 0; }
OCEAN_MIP_HD constexpr int mip_partner_lane(int tid, int j) { return (tid & 63) + (1 << (j - 1)); }
OCEAN_MIP_HD constexpr int mip_dst_x(int tx, int tid, int j) { return tx * (kMipTile >> j) + ((tid & 63) >> j); }
OCEAN_MIP_HD constexpr int mip_dst_y(int ty, int tid, int j, int r)
{
  return ty * (kMipTile >> j) + (tid >> 6) * (kMipRowsPerWave >> j) + r;
}

// The 4 x 4 level-4 values of a tile in the LDS: the slot of the value the holding lane of wave w has
OCEAN_MIP_HD constexpr int mip_lds_slot(int tid) { return (tid >> 6) * 4 + ((tid & 63) >> 4); }

}  // namespace oceanfft
