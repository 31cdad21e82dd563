// device/k_kinematics.h — the packed images of the depth layers (ocean_generator_calculate_kinematics,
// include/oceanfft.h): per cascade and rest depth d, the water velocity and the pressure head under every
// texel, and their sampler (ocean_water_kinematics).
//
// Linear wave theory attenuates every wavenumber on its own, so the factor is applied in k space, before
// the transform: the layers are the frame's own packing (pack_height / pack_displacement of H and of
// Hd = dH/dt, device/k_rates.h) with each complex lane multiplied by a real factor
//     A_h = cosh(k (h - dc)) / cosh(k h)     horizontal velocity and pressure
//     A_v = sinh(k (h - dc)) / sinh(k h)     vertical velocity,                     dc = min(d, h),
// both 1 at the surface. A real multiple keeps a lane's (field, partner) structure, so the Nyquist-row
// defect of the reference's spectrum (device/k_rates.h) is attenuated at its own wavenumber and layer 0 is
// the rate maps' and the height map's lanes bit for bit. In exponentials of non-positive arguments (no
// overflow at any k h):
//     e1 = exp(-k dc), e2 = exp(-2k (h - dc)), e3 = exp(-2k h)
//     A_h = e1 (1 + e2) / (1 + e3),   A_v = e1 expm1(-2k (h - dc)) / expm1(-2k h)   (0 when h == 0).
// At d == 0 the two arguments of each quotient are the same bits and e1 = exp(-0) = 1, so with the
// correctly rounded division both factors are exactly 1.0f. exp is the hardware exponential (its error,
// <= 1e-6 of a factor that is itself <= 1, is below the transform's); expm1 keeps A_v's relative accuracy
// for the longest waves in shallow water, where 2 k h is a few hundredths.
//
// Memory: 16 B read (h0) and 32 * layers B written per point; k_rates_pack's two shapes (BLOCK: CW x
// 1024 / CW texel blocks, four texels per thread, whole-line stores; linear: 256 consecutive texels of the
// blocked image, N = 16, 32), by the same walk (pack_item_texel, device/evolve.h) and the same shape rule
// (pack_shape, launch_common.h). H and Hd are evolved once per texel from one sincos_phase
// (evolve_with_rate, device/evolve.h: evolve()'s and evolve_rate()'s bits); the layers are
// the innermost loop and each layer's two texels are stored as soon as they are formed, so only the four
// packed texels of a point stay live, not its layers (62 VGPRs, no scratch, 8 waves per SIMD).
// Measured (tools/kinematics_bench.py, profiles/kinematics_bench.log; the whole call minus its EncodeIFFT
// alone, beside a plain copy of the same bytes): 8 x 4096^2 with 1 / 4 layers 1.35 / 3.82 ms, 0.60 / 0.63 of
// 8 TB/s at 48 / 144 B per point, 0.97 x the copy both times; 1 x 4096^2 0.155 / 0.537 ms, 0.95 / 1.06 x the
// copy. HBM binds, not the three exponentials, two expm1 and two divisions per texel and layer. At 3 x 256^2
// (0.005 / 0.016 ms) the launch is too short to stream: there the arithmetic shows, 1.5 / 3.8 x the copy.
#pragma once

#include <hip/hip_runtime.h>

#include "device/evolve.h"
#include "device/surface_sample.h"

namespace oceanfft
{

constexpr int kKinematicsTile = 256;  // threads per workgroup; a BLOCK item is 1024 texels, a linear one 256

// (A_h, A_v) of wavenumber k at rest depth d in water of depth h (the header of this file)
__device__ __forceinline__ float2 depth_attenuation(float k, float d, float h)
{
#pragma clang fp contract(off)
  const float dc = fminf(d, h);
  const float k2 = 2.0f * k;
  const float x2 = -(k2 * (h - dc)), x3 = -(k2 * h);
  const float e1 = __expf(-(k * dc)), e2 = __expf(x2), e3 = __expf(x3);
  const float ah = e1 * ((1.0f + e2) / (1.0f + e3));
  const float av = h == 0.0f ? 0.0f : e1 * (expm1f(x2) / expm1f(x3));
  return make_float2(ah, av);
}

// out: [cascade][layer][image 0, image 1][n * n], row-major, still in k space (the batched EncodeIFFT
// follows). items = cascades * n * n / (BLOCK ? 1024 : 256); lcw = log2 CW (device/k_rates.h).
template <bool BLOCK>
__global__ __launch_bounds__(kKinematicsTile) void k_kinematics_pack(FrameParams fp, KinematicsDepths kd, int logn,
                                                                     int logb, int lcw,
                                                                     const float4* __restrict__ h0,
                                                                     float4* __restrict__ out, int items)
{
  constexpr int J = BLOCK ? 4 : 1;
  const int n = 1 << logn;
  const float dim = (float)n;
  const int litems = 2 * logn - (BLOCK ? 10 : 8);  // log2 of the items per cascade
  const size_t nn = (size_t)n * n;
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int c = item >> litems;
    const unsigned local = (unsigned)(item - (c << litems));
    const float4* hc = h0 + (size_t)c * nn;
    int x[J], y[J];
    float4 a[J];
#pragma unroll
    for (int j = 0; j < J; j++)  // every load issued before the first use
      a[j] = hc[pack_item_texel<BLOCK>(local, j, n, logn, logb, lcw, x[j], y[j])];
    const CascadeFrame f = fp.c[c];
    float4* oc = out + (size_t)c * kd.layers * 2 * nn;
#pragma unroll
    for (int j = 0; j < J; j++)
    {
      const KVec q = make_kvec(x[j], y[j], dim, f.dk);
      float2 h, hd;
      evolve_with_rate(a[j], q.k, f, h, hd);
      const CPair rh = pack_height(hd, q), rd = pack_displacement(hd, q), ph = pack_height(h, q);
      float4* o = oc + ((size_t)y[j] << logn) + x[j];
      for (int l = 0; l < kd.layers; l++)
      {
        const float2 at = depth_attenuation(q.k, kd.d[l], f.h);
        o[0] = make_float4(at.y * rh.re.x, at.y * rh.im.x, at.x * rh.re.y, at.x * rh.im.y);
        o[nn] = make_float4(at.x * rd.re.x, at.x * rd.im.x, at.x * ph.re.x, at.x * ph.im.x);
        o += 2 * nn;
      }
    }
  }
}

// What ocean_water_kinematics returns for one world position (include/oceanfft.h): the fixed point is the
// query's (surface_base_point on the maps); the chain then runs once more from the base point with the
// layers' taps beside the maps', layer l and, where the blend factor is not 0, layer l + 1. The fixed-point
// loop is lane-divergent. One definition for k_water_kinematics and the mooring lines' nodes
// (device/k_moorings.h): the same expressions, the same bits.
struct WaterPoint
{
  float bx, eta, bz, res;
  float ux, uy, uz, head;
  float d, f;
  int l;
  bool wet;
};

__device__ __forceinline__ WaterPoint water_point_kinematics(const SurfaceParams& p, const WaterLayers& w, float qx,
                                                             float qy, float qz, int iterations, float tolerance)
{
#pragma clang fp contract(off)
  const size_t nn = (size_t)p.n * p.n;
  float bx = qx, bz = qz;  // the base point p
  float vx, eta, vz;
  surface_base_point<false>(p, qx, qz, iterations, tolerance, bx, bz, vx, eta, vz);
  const float res = surface_residual(qx, qz, vx, vz);
  const float s = eta - qy;
  const bool wet = s > 0.0f;
  const float d = wet ? s : 0.0f;  // max(s, 0), NaN -> 0
  int l = 0;
  float f = 0.0f;
  if (d > w.d[0])
  {
    l = w.layers - 1;
    if (!(d >= w.d[l]))
    {
      l = 0;
      while (w.d[l + 1] <= d)  // ends: d < d[layers - 1]
        l++;
      f = (d - w.d[l]) / (w.d[l + 1] - w.d[l]);
    }
  }
  float px = bx, pz = bz, ux = 0.0f, uy = 0.0f, uz = 0.0f, head = 0.0f;
  for (int c = 0; c < p.count; c++)
  {
    const float u = px / p.c[c].plane, v = pz / p.c[c].plane;
    const LinearTaps k = linear_repeat_taps(p.n, u, v);
    const float sc = p.c[c].scale;
    const float* a0 = reinterpret_cast<const float*>(w.map[c] + (size_t)(2 * l) * nn);
    const float* a1 = reinterpret_cast<const float*>(w.map[c] + (size_t)(2 * l + 1) * nn);
    float v0w = linear_channel<4>(a0, k, 3), v0x = linear_channel<4>(a0, k, 0);
    float v1x = linear_channel<4>(a1, k, 0), v1z = linear_channel<4>(a1, k, 2);
    if (f != 0.0f)
    {
      const float* b0 = a0 + 8 * nn;
      const float* b1 = a1 + 8 * nn;
      v0w = v0w + f * (linear_channel<4>(b0, k, 3) - v0w);
      v0x = v0x + f * (linear_channel<4>(b0, k, 0) - v0x);
      v1x = v1x + f * (linear_channel<4>(b1, k, 0) - v1x);
      v1z = v1z + f * (linear_channel<4>(b1, k, 2) - v1z);
    }
    ux += sc * v0w;
    uy += v0x;
    uz += sc * v1x;
    head += v1z;
    const float* hm = reinterpret_cast<const float*>(p.c[c].height);
    const float* dm = reinterpret_cast<const float*>(p.c[c].disp);
    px += sc * linear_channel<4>(hm, k, 3);
    pz += sc * linear_channel<4>(dm, k, 0);
  }
  return WaterPoint{bx, eta, bz, res, ux, uy, uz, head, d, f, l, wet};
}

// ocean_water_kinematics (include/oceanfft.h): one lane per world position. `inline` for its linkage: this
// header is also included by launch_moorings.hip, which does not launch the kernel and must not define it again
// (clang notes that CUDA would ignore the keyword on a kernel; it does give the host stub vague linkage).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ __launch_bounds__(256) void k_water_kinematics(SurfaceParams p, WaterLayers w, const float* __restrict__ xyz,
                                                          int64_t count, int iterations, float tolerance,
                                                          float4* __restrict__ out)
{
#pragma clang fp contract(off)
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < count;
       idx += (int64_t)gridDim.x * blockDim.x)
  {
    const WaterPoint q =
        water_point_kinematics(p, w, xyz[3 * idx], xyz[3 * idx + 1], xyz[3 * idx + 2], iterations, tolerance);
    out[3 * idx] = make_float4(q.bx, q.eta, q.bz, q.res);
    out[3 * idx + 1] = make_float4(q.ux, q.uy, q.uz, q.head);
    out[3 * idx + 2] = make_float4(q.d, (float)q.l, q.f, q.wet ? 1.0f : 0.0f);
  }
}
#pragma clang diagnostic pop

}  // namespace oceanfft
