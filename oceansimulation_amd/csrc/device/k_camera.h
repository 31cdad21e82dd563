// device/k_camera.h — ocean_camera_render and ocean_camera_rays (include/oceanfft.h): the picture a pinhole
// camera sees of the water. One lane per pixel, one fused pass: camera ray -> ocean_surface_raycast's march
// (device/ray_march.h, unchanged) -> fragment stage at the hit (on the mip pyramid by the
// pixel's footprint when lod_scale > 0) -> the reference's water colour (resources/waveShader.glsl:146-160)
// -> its fog (:221-233) -> its sky (:41-63) -> image. No hit record goes through memory: per pixel 16 B
// (image), 16 B (aux) and 4 B (image8) are written, whichever of them the caller asked for.
// ocean_camera_render_layers' water pass is the same kernel with FOAM = true: the persistent foam shaded
// between the water colour and the fog, and the per-pixel words its spray pass (device/k_camera_spray.h)
// starts from.
//
// A work item is a 16 x 16 pixel tile; wave w of the workgroup owns an 8 x 8 sub-tile of it, so the 64 rays
// of a wave leave through neighbouring pixels: their march lengths are similar (a wave runs until its last
// lane is done) and their evaluations touch neighbouring texels. Ragged edge tiles are masked.
// The shading runs after the march, on registers the march has released; the camera, the shading constants
// and the march parameters are kernel arguments (scalar registers).
// Everything is unfused fp32 and follows the header's contract operation by operation
// (tests/camera_ref.py restates it in numpy); expf is the one operation numpy cannot restate bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "device/ray_march.h"
#include "device/surface_lod.h"
#include "device/surface_sample.h"
#include "ocean_internal.h"

namespace oceanfft
{

constexpr int kCameraThreads = 256;  // a 16 x 16 pixel tile
constexpr int kCameraTile = 16;

struct CameraRay
{
  float dx, dy, dz, len;
};

// The ray through the centre of pixel (i, j), row 0 on top; len is |(x, y, 1)|, so depth z = t / len
__device__ __forceinline__ CameraRay camera_ray(const CameraParams& cam, int i, int j)
{
#pragma clang fp contract(off)
  const float aspect = (float)cam.width / (float)cam.height;
  const float x = (((2.0f * ((float)i + 0.5f)) / (float)cam.width) - 1.0f) * (aspect * cam.tan_half);
  const float y = (1.0f - ((2.0f * ((float)j + 0.5f)) / (float)cam.height)) * cam.tan_half;
  const float len = sqrtf((x * x + y * y) + 1.0f);
  return CameraRay{((x * cam.right[0] + y * cam.up[0]) + cam.fwd[0]) / len,
                   ((x * cam.right[1] + y * cam.up[1]) + cam.fwd[1]) / len,
                   ((x * cam.right[2] + y * cam.up[2]) + cam.fwd[2]) / len, len};
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}

// SampleSkybox (waveShader.glsl:41-63) in direction v (any length)
__device__ __forceinline__ void camera_sky(const ShadingParams& sh, float vx, float vy, float vz, float& r, float& g,
                                           float& b)
{
#pragma clang fp contract(off)
  const float vl = sqrtf((vx * vx + vy * vy) + vz * vz);
  const float ux = vx / vl, uy = vy / vl, uz = vz / vl;
  const float s = dot3(sh.L[0], sh.L[1], sh.L[2], ux, uy, uz);
  const float e = ray_min(ray_max((s - sh.cfade) / (sh.cthr - sh.cfade), 0.0f), 1.0f);
  float w = (e * e) * (3.0f - 2.0f * e);
  w = w * (w * w);
  float m = 0.8f - uy / 0.8f;
  m = m * m;
  const float a = 1.0f - w, c = 2.0f * w;
  r = a * (sh.sky[0] * (1.0f - m) + sh.light[0] * m) + c * sh.light[0];
  g = a * (sh.sky[1] * (1.0f - m) + sh.light[1] * m) + c * sh.light[1];
  b = a * (sh.sky[2] * (1.0f - m) + sh.light[2] * m) + c * sh.light[2];
}

__device__ __forceinline__ uint32_t camera_byte(float c)
{
#pragma clang fp contract(off)
  return !(c > 0.0f) ? 0u : (uint32_t)(ray_min(c, 1.0f) * 255.0f + 0.5f);
}

// The ray formula alone: one lane per pixel, row-major, grid-stride
__global__ __launch_bounds__(kCameraThreads) void k_camera_rays(CameraParams cam, float4* __restrict__ rays)
{
#pragma clang fp contract(off)
  const int64_t n = (int64_t)cam.width * cam.height;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x)
  {
    const CameraRay r = camera_ray(cam, (int)(idx % cam.width), (int)(idx / cam.width));
    rays[2 * idx] = make_float4(cam.pos[0], cam.pos[1], cam.pos[2], cam.near_plane * r.len);
    rays[2 * idx + 1] = make_float4(r.dx, r.dy, r.dz, cam.far_plane * r.len);
  }
}

// The two arguments only the FOAM variants have: nothing in their place otherwise, so the FOAM = false
// instantiations read the arguments, and are the code, they were before the variants existed.
struct CameraNoArg
{
};
template <bool FOAM>
using CameraFoamArg = std::conditional_t<FOAM, SurfaceFoam, CameraNoArg>;
template <bool FOAM>
using CameraWaterArg = std::conditional_t<FOAM, CameraWaterLayers, CameraNoArg>;

// grid: items = ceil(width / 16) * ceil(height / 16) tiles, item loop. The camera and the shading constants
// on top of the march's arguments ask for 106 SGPRs, one wave per SIMD less than the march alone runs at
// (8 waves need <= 96 on gfx950): capped, the surplus spills to lanes of one VGPR (no scratch).
// FOAM (ocean_camera_render_layers' water pass): the foam stage between the water colour and the fog (when
// lw.foam_opacity > 0: the foam maps in an argument of their own, as k_surface_foam), the pixel's aux2 row
// when no spray pass follows, and when one does the pixel's foam, key and hit words for it (lw.key non-null):
// the kernel owns each pixel exactly once, so the spray pass needs no memset.
template <bool LOD, bool FOAM>
__global__ __launch_bounds__(kCameraThreads) __attribute__((amdgpu_num_sgpr(96))) void k_camera_render(
    SurfaceParams p, RaycastParams rc, CameraParams cam, ShadingParams sh, float4* __restrict__ image,
    float4* __restrict__ aux, uint32_t* __restrict__ image8, CameraFoamArg<FOAM> fm, CameraWaterArg<FOAM> lw)
{
#pragma clang fp contract(off)
  float ylo, yhi;
  ray_slab(p, rc, ylo, yhi);
  const int tiles_x = (cam.width + kCameraTile - 1) / kCameraTile, tiles_y = (cam.height + kCameraTile - 1) / kCameraTile;
  const int items = tiles_x * tiles_y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = 8 * (wave & 1) + (lane & 7), py = 8 * (wave >> 1) + (lane >> 3);
  const int top = 31 - __clz(p.n);
  for (int item = blockIdx.x; item < items; item += gridDim.x)
  {
    const int i = (item % tiles_x) * kCameraTile + px, j = (item / tiles_x) * kCameraTile + py;
    if (i >= cam.width || j >= cam.height)
      continue;
    const int64_t idx = (int64_t)j * cam.width + i;
    const CameraRay ray = camera_ray(cam, i, j);
    float cr, cg, cb;  // the pixel
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    float fog = 1.0f;  // the share of sky(d): all of it unless the ray hits
    float wr = 0.0f, wg = 0.0f, wb = 0.0f;
    [[maybe_unused]] float foam = 0.0f;
    RayMarch m;
    if (ray_march(p, rc, ylo, yhi, cam.pos[0], cam.pos[1], cam.pos[2], cam.near_plane * ray.len, ray.dx, ray.dy, ray.dz,
                  cam.far_plane * ray.len, m))
    {
      const float z = m.t / ray.len;
      float4 f;
      if constexpr (LOD)
        f = surface_fragment_stage_lod(p, top, cam.lod_scale * (z * ((2.0f * cam.tan_half) / (float)cam.height)), m.vx,
                                       m.vz);
      else
        f = surface_fragment_stage<false>(p, m.vx, m.vz);
      a = make_float4(m.t, z, f.w, (float)m.status);
      if (m.status == 0)
      {
        // waveShader.glsl:146-160 at P = V, then the fog factor of :230-231
        const float ex = cam.pos[0] - m.vx, ey = cam.pos[1] - m.vy, ez = cam.pos[2] - m.vz;
        const float el = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float ix = -(ex / el), iy = -(ey / el), iz = -(ez / el);
        const float k = 2.0f * dot3(f.x, f.y, f.z, ix, iy, iz);
        const float rx = ix - k * f.x, ry = iy - k * f.y, rz = iz - k * f.z;
        const float diffuse = ray_max(dot3(f.x, f.y, f.z, sh.L[0], sh.L[1], sh.L[2]), 0.0f) * 0.3f;
        float sp = ray_max(dot3(rx, ry, rz, sh.L[0], sh.L[1], sh.L[2]), 0.0f);
        for (int q = 0; q < 5; q++)
          sp = sp * sp;
        const float specular = sp * 0.5f;
        const float scatter = ray_max(m.vy * 0.1f, 0.0f);
        const float light = (diffuse + 0.5f) + specular;
        float sr, sg, sb;
        camera_sky(sh, rx, ry, rz, sr, sg, sb);
        wr = ((light * sh.wave[0]) * sr) + scatter * sh.scatter[0];
        wg = ((light * sh.wave[1]) * sg) + scatter * sh.scatter[1];
        wb = ((light * sh.wave[2]) * sb) + scatter * sh.scatter[2];
        if constexpr (FOAM)
          if (lw.foam_opacity > 0.0f)
          {
            foam = surface_foam_stage(p, fm, m.vx, m.vz);
            float w = ray_min(ray_max((foam - lw.foam_lo) / (lw.foam_hi - lw.foam_lo), 0.0f), 1.0f);
            w = (w * w) * (3.0f - 2.0f * w);
            w = w * lw.foam_opacity;
            const float lit = diffuse + 0.5f;
            wr = wr * (1.0f - w) + (lit * lw.foam_color[0]) * w;
            wg = wg * (1.0f - w) + (lit * lw.foam_color[1]) * w;
            wb = wb * (1.0f - w) + (lit * lw.foam_color[2]) * w;
          }
        fog = ray_max(1.0f - expf(-((z - sh.fog_begin) * sh.fog_density)), 0.0f);
      }
    }
    camera_sky(sh, ray.dx, ray.dy, ray.dz, cr, cg, cb);
    if (a.w == 0.0f)
    {
      cr = wr * (1.0f - fog) + cr * fog;
      cg = wg * (1.0f - fog) + cg * fog;
      cb = wb * (1.0f - fog) + cb * fog;
    }
    if (image)
      image[idx] = make_float4(cr, cg, cb, 1.0f);
    if (aux)
      aux[idx] = a;
    if (image8)
      image8[idx] = camera_byte(cr) | (camera_byte(cg) << 8) | (camera_byte(cb) << 16) | 0xFF000000u;
    if constexpr (FOAM)
    {
      if (lw.aux2)
        lw.aux2[idx] = make_float4(foam, 0.0f, __uint_as_float(0u), __uint_as_float(0xFFFFFFFFu));
      if (lw.key)
      {
        lw.key[idx] = ~0ull;
        lw.hits[idx] = 0u;
        lw.foam[idx] = foam;
      }
    }
  }
}

}  // namespace oceanfft
