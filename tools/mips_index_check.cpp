// mips_index_check — walks the index arithmetic of the mip downsampler (csrc/device/mip_index.h, the
// functions k_mips itself calls) on the host: for every N = 16 .. 16384, every launch of a build, every
// tile and thread, each load the kernel's predicate lets through lies inside the source level, each store
// inside its destination level and inside the cascade's chain, distinct levels do not overlap, every
// texel of every level is written exactly once, and each horizontal partner lane is in the reader's row
// of 16 and held a value at the previous halving. No GPU, no Python:
//   g++ -O2 -std=c++17 -Ioceansimulation_amd/csrc tools/mips_index_check.cpp -o mips_index_check && ./mips_index_check
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device/mip_index.h"

using namespace oceanfft;

#define CHECK(cond)                                                                                  \
  do                                                                                                 \
  {                                                                                                  \
    if (!(cond))                                                                                     \
    {                                                                                                \
      std::fprintf(stderr, "FAILED %s (line %d): n=%d level=%d tile=(%d,%d) tid=%d\n", #cond, __LINE__, n, level, \
                   tx, ty, tid);                                                                     \
      std::exit(1);                                                                                  \
    }                                                                                                \
  } while (0)

int main()
{
  for (int top = 4; top <= 14; top++)
  {
    const int n = 1 << top;
    const size_t chain = mip_chain_texels(n);
    std::vector<unsigned char> written(chain, 0);  // texels of levels >= 1, by chain offset
    // the levels tile the chain without gaps or overlap
    {
      int level = 0, tx = 0, ty = 0, tid = 0;
      size_t end = 0;
      for (int l = 1; l <= top; l++)
      {
        CHECK(mip_level_offset(n, l) == end);
        CHECK(mip_level_offset(n, l) % 4 == 0);
        end += (size_t)(n >> l) * (n >> l);
      }
      CHECK(end <= chain && chain - end < 4 && chain % 4 == 0);
    }
    int launches = 0;
    for (int level = 0; level < top; level += kMipFused, launches++)
    {
      const int s = n >> level, tiles = mip_tiles(s);
      // a launch reads a level an earlier launch completed
      for (int ty = 0; ty < tiles; ty++)
        for (int tx = 0; tx < tiles; tx++)
        {
          for (int tid = 0; tid < 256; tid++)
          {
            // loads: the kernel's predicate is x < s && y < s; what passes must be a texel of the source
            const int x = mip_src_x(tx, tid);
            CHECK(x >= 0);
            for (int k = 0; k < kMipRowsPerWave; k++)
            {
              const int y = mip_src_y(ty, tid, k);
              CHECK(y >= 0);
              if (x < s && y < s)
              {
                const size_t idx = (size_t)y * s + x;
                CHECK(idx < (size_t)s * s);
                if (level > 0)
                  CHECK(written[mip_level_offset(n, level) + idx] == 1);
              }
            }
            // halvings 1 .. 4: partner lanes and stores
            for (int j = 1; j <= kMipLaneLevels; j++)
            {
              if (!mip_lane_holds(tid, j))
                continue;
              const int lane = tid & 63, partner = mip_partner_lane(tid, j);
              CHECK(partner < 64 && (partner >> 4) == (lane >> 4));  // a DPP row shift stays in the row of 16
              CHECK(j == 1 || mip_lane_holds((tid & ~63) | partner, j - 1));
              const int l = level + j, side = s >> j;
              if (l > top)
                continue;
              const int dx = mip_dst_x(tx, tid, j);
              for (int r = 0; r < (kMipRowsPerWave >> j); r++)
              {
                const int dy = mip_dst_y(ty, tid, j, r);
                CHECK(dx >= 0 && dy >= 0);
                if (dx < side && dy < side)
                {
                  const size_t off = mip_level_offset(n, l) + (size_t)dy * side + dx;
                  CHECK(off < mip_level_offset(n, l) + (size_t)side * side && off < chain);
                  CHECK(written[off] == 0);
                  written[off] = 1;
                }
              }
            }
            if (mip_lane_holds(tid, kMipLaneLevels))
              CHECK(mip_lds_slot(tid) >= 0 && mip_lds_slot(tid) < 16);
          }
          // halvings 5 and 6 through the LDS: thread (channel, q) -> texel (2 tx + qx, 2 ty + qy), then (tx, ty)
          int tid = 0;
          for (int q = 0; q < 4; q++)
          {
            const int l = level + 5, side = s >> 5, dx = tx * 2 + (q & 1), dy = ty * 2 + (q >> 1);
            if (l <= top && dx < side && dy < side)
            {
              const size_t off = mip_level_offset(n, l) + (size_t)dy * side + dx;
              CHECK(off < chain && written[off] == 0);
              written[off] = 1;
            }
          }
          {
            const int l = level + 6, side = s >> 6;
            if (l <= top && tx < side && ty < side)
            {
              const size_t off = mip_level_offset(n, l) + (size_t)ty * side + tx;
              CHECK(off < chain && written[off] == 0);
              written[off] = 1;
            }
          }
        }
    }
    {
      int level = 0, tx = 0, ty = 0, tid = 0;
      CHECK(launches == mip_launches(top));
      CHECK(launches == (top <= 6 ? 1 : (top <= 12 ? 2 : 3)));
      size_t count = 0;
      for (size_t i = 0; i < chain; i++)
        count += written[i];
      CHECK(count == ((size_t)n * n - 1) / 3);  // every texel of every level exactly once
    }
    std::printf("N = %5d: %d launch%s, chain %zu texels, all indices in bounds\n", n, launches,
                launches == 1 ? "" : "es", chain);
  }
  return 0;
}
