// launch_mips.hip — the mip pyramid of the maps (device/k_mips.h): ceil(log2 N / 6) launches per build,
// each over every cascade; the kernel boundary is the ordering between a launch and the level it reads.
#include "device/k_mips.h"
#include "ocean_internal.h"

namespace oceanfft
{

size_t mip_cascade_floats(int n) { return 9 * mip_chain_texels(n); }

hipError_t launch_build_mips(int n, int cascades, const float4* maps, const float* jac, float* mips, hipStream_t stream)
{
  int top = 0;
  while ((1 << top) < n)
    top++;
  const size_t nn = (size_t)n * n, chain = mip_chain_texels(n);
  MipBuild m{};
  m.n = n;
  m.top = top;
  m.dst[0] = mips;
  m.dst[1] = mips + 4 * chain;
  m.dst[2] = mips + 8 * chain;
  m.dst_stride = mip_cascade_floats(n);
  for (int level = 0; level < top; level += kMipFused)
  {
    m.level = level;
    if (level == 0)
    {
      // the maps: [cascade][heightMap, displacementMap][n * n] float4 and [cascade][n * n] float
      m.src[0] = reinterpret_cast<const float*>(maps);
      m.src[1] = reinterpret_cast<const float*>(maps + nn);
      m.src[2] = jac;
      m.src_stride[0] = m.src_stride[1] = 8 * nn;
      m.src_stride[2] = nn;
    }
    else
    {
      const size_t off = mip_level_offset(n, level);
      m.src[0] = m.dst[0] + 4 * off;
      m.src[1] = m.dst[1] + 4 * off;
      m.src[2] = m.dst[2] + off;
      m.src_stride[0] = m.src_stride[1] = m.src_stride[2] = m.dst_stride;
    }
    const unsigned tiles = (unsigned)mip_tiles(n >> level);
    hipLaunchKernelGGL(k_mips, dim3(tiles, tiles, (unsigned)cascades), dim3(256), 0, stream, m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

}  // namespace oceanfft
