// device/k_camera_spray.h — the spray pass of ocean_camera_render_layers (include/oceanfft.h): particle
// records splatted into the picture the water pass (device/k_camera.h, k_camera_render<LOD, true>) left,
// with a per-pixel depth test against the water each pixel's ray found.
// k_camera_splat: one lane per record, grid-stride; the record count is read on the device. A record is
// projected by the inverse of the ray formula onto a pixel (ci, cj) and a square sprite of at most
// 17 x 17 pixels around it; every covered pixel whose water is farther (or whose ray found none) gets
//     key[q] = min(key[q], (uint64)bits(z) << 32 | r);   hits[q] += 1
// z > 0, so the bits of z order as the floats do and an equal depth resolves to the lower record index. Both
// are integer atomics without a return value (global_atomic_umin_x2, global_atomic_add): min and + commute
// and associate exactly, so the words do not depend on the order the records arrive in and a call replays
// bit for bit. Runs of neighbouring lanes on the same pixel are folded within the wave first (see the kernel).
// The water pass has set the words (key ~0, hits 0) for every pixel it owns: no memset.
// k_camera_composite: one lane per pixel, grid-stride: the nearest record's depth fogs the spray colour, the
// hit count sets its opacity, and the pixel goes to image, image8 and aux2.
// Everything is unfused fp32 and follows the header's contract operation by operation
// (tests/camera_layers_ref.py restates it in numpy); expf is the one operation numpy cannot restate bit for
// bit.
#pragma once

#include <hip/hip_runtime.h>

#include "device/k_camera.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kCameraSprayThreads = 256;

// aux2 of a call with both layers off: (0, 0, 0, index 0xFFFFFFFF) per pixel. grid: any; grid-stride
__global__ __launch_bounds__(kCameraSprayThreads) void k_camera_aux2_none(int64_t n, float4* __restrict__ aux2)
{
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x)
    aux2[idx] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
}

// grid: any; a lane per record, grid-stride over n = min(*count_device, max_records). The loops are wave-uniform
// (every lane runs every round and every sprite offset up to the wave's largest half, predicated), so lanes
// can merge before the atomics: an ordered list (an emitter's, by texel) seen from far away puts neighbouring
// records, that is neighbouring lanes, on the same pixel. Where a lane's pixel equals the lane's before it, a
// segmented scan over the runs of equal pixels folds min and count into the last lane of each run, which
// issues one pair for the run. min and + are exact, so the words are what the unmerged atomics give.
__global__ __launch_bounds__(kCameraSprayThreads) void k_camera_splat(CameraParams cam, CameraSpray s)
{
#pragma clang fp contract(off)
  int64_t n = s.max_records;
  if (s.count_device)
  {
    const int64_t c = *s.count_device;
    n = c < n ? c : n;
  }
  const float aspect = (float)cam.width / (float)cam.height;
  const float tx = aspect * cam.tan_half;                       // x = tx at the right edge
  const float pixel = (2.0f * cam.tan_half) / (float)cam.height;  // a pixel's world size at depth 1
  const float half_w = 0.5f * (float)cam.width, half_h = 0.5f * (float)cam.height;
  const int lane = threadIdx.x & 63;
  for (int64_t first = (int64_t)blockIdx.x * blockDim.x; first < n; first += (int64_t)gridDim.x * blockDim.x)
  {
    const int64_t r = first + threadIdx.x;
    int half = -1, i0 = 0, j0 = 0;  // half < 0: no record, or culled
    float z = 0.0f;
    if (r < n)
    {
      const float* rec = s.records + 8 * r;
      const float ex = rec[0] - cam.pos[0], ey = rec[1] - cam.pos[1], ez = rec[2] - cam.pos[2];
      z = dot3(ex, ey, ez, cam.fwd[0], cam.fwd[1], cam.fwd[2]);
      const float x = dot3(ex, ey, ez, cam.right[0], cam.right[1], cam.right[2]);
      const float y = dot3(ex, ey, ez, cam.up[0], cam.up[1], cam.up[2]);
      if (z >= cam.near_plane && z <= cam.far_plane)
      {
        const float ci = floorf(((x / (z * tx)) + 1.0f) * half_w);
        const float cj = floorf((1.0f - (y / (z * cam.tan_half))) * half_h);
        const float hf = ray_min(floorf(s.radius / (z * pixel)), (float)s.max_half);
        const int h = hf == hf ? (int)hf : 0;  // 0 .. max_half <= 8
        if (ci >= (float)-h && ci <= (float)(cam.width - 1 + h) && cj >= (float)-h && cj <= (float)(cam.height - 1 + h))
        {
          half = h;
          i0 = (int)ci;  // within [-8, 16391]
          j0 = (int)cj;
        }
      }
    }
    const unsigned long long own = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)r;
    int reach = s.max_half;  // the wave's largest half
    while (reach >= 0 && !__any(half >= reach))
      reach--;
    for (int db = -reach; db <= reach; db++)
      for (int da = -reach; da <= reach; da++)
      {
        const int a = i0 + da, b = j0 + db;
        const bool in = (da < 0 ? -da : da) <= half && (db < 0 ? -db : db) <= half && a >= 0 && a < cam.width &&
                        b >= 0 && b < cam.height;
        uint32_t q = 0xFFFFFFFFu;  // < width * height <= 2^28 when the lane has a pixel
        bool pass = false;
        if (in)
        {
          q = (uint32_t)b * (uint32_t)cam.width + (uint32_t)a;
          const float4 w = s.aux[q];
          pass = w.w != 0.0f || z < w.y;
        }
        if (!__any(pass))
          continue;
        if (!pass)
          q = 0xFFFFFFFFu;
        unsigned long long key = pass ? own : ~0ull;
        uint32_t count = pass ? 1u : 0u;
        const uint32_t before = __shfl_up(q, 1);
        const bool head = lane == 0 || before != q;  // the first lane of a run of equal pixels
        if (__any(pass && !head))
        {
          uint32_t open = head ? 0u : 1u;  // the lane's scan still reaches further back
#pragma unroll
          for (int d = 1; d < 64; d <<= 1)
          {
            const unsigned long long k = __shfl_up(key, d);
            const uint32_t c = __shfl_up(count, d), o = __shfl_up(open, d);
            if (lane >= d && open)
            {
              key = k < key ? k : key;
              count += c;
              open = o;
            }
          }
        }
        const uint32_t next_head = __shfl_down(head ? 1u : 0u, 1);
        if (count > 0u && (lane == 63 || next_head))
        {
          (void)__hip_atomic_fetch_min(s.key + q, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          (void)__hip_atomic_fetch_add(s.hits + q, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
  }
}

// grid: any; a lane per pixel, row-major, grid-stride. s.base may be `image` itself: a lane reads its own
// pixel before it writes it.
__global__ __launch_bounds__(kCameraSprayThreads) void k_camera_composite(CameraParams cam, ShadingParams sh,
                                                                          CameraSpray s, float4* image,
                                                                          uint32_t* image8, float4* aux2)
{
#pragma clang fp contract(off)
  const int64_t n = (int64_t)cam.width * cam.height;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x)
  {
    const unsigned long long key = s.key[idx];
    const uint32_t c = s.hits[idx];
    const float4 base = s.base[idx];
    float cr = base.x, cg = base.y, cb = base.z, zs = 0.0f;
    uint32_t rid = 0xFFFFFFFFu;
    if (c > 0u)
    {
      zs = __uint_as_float((uint32_t)(key >> 32));
      rid = (uint32_t)key;
      const float a = ray_min((float)c * s.opacity, 1.0f);
      const float fs = ray_max(1.0f - expf(-((zs - sh.fog_begin) * sh.fog_density)), 0.0f);
      const CameraRay ray = camera_ray(cam, (int)(idx % cam.width), (int)(idx / cam.width));
      float kr, kg, kb;
      camera_sky(sh, ray.dx, ray.dy, ray.dz, kr, kg, kb);
      const float sr = (s.color[0] * sh.light[0]) * (1.0f - fs) + kr * fs;
      const float sg = (s.color[1] * sh.light[1]) * (1.0f - fs) + kg * fs;
      const float sb = (s.color[2] * sh.light[2]) * (1.0f - fs) + kb * fs;
      cr = cr * (1.0f - a) + sr * a;
      cg = cg * (1.0f - a) + sg * a;
      cb = cb * (1.0f - a) + sb * a;
    }
    if (image)
      image[idx] = make_float4(cr, cg, cb, 1.0f);
    if (image8)
      image8[idx] = camera_byte(cr) | (camera_byte(cg) << 8) | (camera_byte(cb) << 16) | 0xFF000000u;
    if (aux2)
      aux2[idx] = make_float4(s.foam[idx], zs, __uint_as_float(c), __uint_as_float(rid));
  }
}

}  // namespace oceanfft
