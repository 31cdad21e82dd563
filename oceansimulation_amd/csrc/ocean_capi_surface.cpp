// ocean_capi_surface.cpp — the part of the C ABI (include/oceanfft.h) that consumes a generator's maps:
// the map getters, ocean_surface_sample / _query / _sample_plane, the mip pyramids and the *_lod requests,
// the rate maps and ocean_surface_velocity, the depth layers and ocean_water_kinematics, the bounds and ocean_surface_raycast, the persistent foam with
// ocean_surface_sample_foam and ocean_foam_deposit, the camera images (ocean_camera_render, ocean_camera_render_layers), the hull sets, the mooring
// lines, the wake windows, the spray emitters and the spray particles.
// The plans and generators themselves are in ocean_capi.cpp, their exchanges in ocean_capi_exchange.cpp;
// ocean_capi_internal.h has what the three share.
//
// Every request checks its arguments in the order its contract lists them, and every message starts with
// the entry point's name (`who`); the checks more than one entry point makes are written once, below.
#include "oceanfft.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device/mip_index.h"
#include "ocean_capi_internal.h"
#include "ocean_internal.h"

namespace
{

// A generator's buffer that is allocated on first use
template <typename T>
int alloc_once(T*& ptr, size_t bytes, const std::string& who)
{
  const hipError_t e = alloc_if_null(ptr, bytes);
  return e == hipSuccess ? OCEAN_OK : alloc_fail(e, who);
}

// A generator's buffer that is allocated on first use and zeroed on `stream` (ocean_foam_deposit's)
template <typename T>
int alloc_zeroed_once(T*& ptr, size_t bytes, hipStream_t stream, const std::string& who)
{
  if (ptr)
    return OCEAN_OK;
  T* fresh = nullptr;
  hipError_t e = alloc_if_null(fresh, bytes);
  if (e == hipSuccess && (e = hipMemsetAsync(fresh, 0, bytes, stream)) != hipSuccess)
  {
    (void)hipStreamSynchronize(stream);  // the memset of the buffer about to be freed may be in flight
    (void)hipFree(fresh);
  }
  if (e != hipSuccess)
    return alloc_fail(e, who);
  ptr = fresh;
  return OCEAN_OK;
}

// A generator that holds whole maps and, with `frame`, has calculated a frame
int whole_maps(const ocean_generator* g, bool frame, const std::string& who)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, who + ": null generator");
  if (g->slab || g->ranks != 1)
    return fail(OCEAN_ERR_INVALID, who + ": slab generators hold row slabs, not whole maps");
  if (frame && g->frame.cascades != g->cascades)
    return fail(OCEAN_ERR_INVALID, who + ": no frame calculated yet (ocean_generator_calculate)");
  return OCEAN_OK;
}

int check_points(int64_t points, const float* positions, const float* out, const std::string& who)
{
  if (points < 0 || (points > 0 && (!positions || !out)))
    return fail(OCEAN_ERR_INVALID, who + ": null positions/output or negative count");
  return OCEAN_OK;
}

// The parameters of the query's fixed point
int check_fixed_point(int iterations, float tolerance, const std::string& who)
{
  if (iterations < 0 || iterations > 64)
    return fail(OCEAN_ERR_INVALID, who + ": iterations outside 0..64");
  if (!(tolerance >= 0.0f) || !std::isfinite(tolerance))
    return fail(OCEAN_ERR_INVALID, who + ": tolerance must be finite and >= 0");
  return OCEAN_OK;
}

// The scalar rules of a march (ocean_surface_raycast, ocean_camera_render)
int check_march(float step, int max_steps, int refine, int iterations, float tolerance, float slope, float pad,
                const std::string& who)
{
  if (!std::isfinite(step) || !(step > 0.0f))
    return fail(OCEAN_ERR_INVALID, who + ": step must be finite and > 0");
  if (max_steps < 1 || max_steps > 65535)
    return fail(OCEAN_ERR_INVALID, who + ": max_steps outside 1..65535");
  if (refine < 0 || refine > 32)
    return fail(OCEAN_ERR_INVALID, who + ": refine outside 0..32");
  TRY(check_fixed_point(iterations, tolerance, who));
  if (!(pad >= 0.0f) || !std::isfinite(pad))
    return fail(OCEAN_ERR_INVALID, who + ": pad must be finite and >= 0");
  if (!(slope >= 0.0f))
    return fail(OCEAN_ERR_INVALID, who + ": slope must be >= 0 (+inf: fixed steps)");
  return OCEAN_OK;
}

// A plane-mesh request: its SurfacePlane and vertex count
int plane_request(const float camera[5], int res, const float* out, const std::string& who, SurfacePlane& plane,
                  int64_t& points)
{
  if (!camera || !out || res < 1 || res > 46340)
    return fail(OCEAN_ERR_INVALID, who + ": null camera/output or resolution outside 1..46340");
  if (camera[3] == 0.0f && camera[4] == 0.0f)
    return fail(OCEAN_ERR_INVALID, who + ": camera forward has no horizontal component");
  plane = SurfacePlane{res, camera[0], camera[1], camera[2], camera[3], camera[4]};
  points = (int64_t)(res + 1) * (res + 1);
  return OCEAN_OK;
}

int check_dt(float dt, const std::string& who)
{
  if (!(dt >= 0.0f) || !std::isfinite(dt))
    return fail(OCEAN_ERR_INVALID, who + ": dt must be finite and >= 0");
  return OCEAN_OK;
}

// A request's generators run on the plan of the object it uses (`what`: the hull set, the emitter, the pool)
int same_plan(const ocean_generator* first, const ocean_fft* fft, const char* what, const std::string& who)
{
  if (first->fft != fft)
    return fail(OCEAN_ERR_INVALID, who + ": the first generator is on another plan than the " + what);
  return OCEAN_OK;
}

// Every pair of a request (its surface_params passed) holds whole maps with a frame calculated
int frames_calculated(ocean_generator* const* gens, int count, const std::string& who)
{
  for (int i = 0; i < count; i++)
  {
    if (gens[i]->slab)
      return fail(OCEAN_ERR_INVALID,
                  who + ": generator " + std::to_string(i) + " is a slab generator: row slabs, not whole maps");
    if (gens[i]->frame.cascades != gens[i]->cascades)
      return fail(OCEAN_ERR_INVALID, who + ": generator " + std::to_string(i) +
                                         " has no frame calculated yet (ocean_generator_calculate)");
  }
  return OCEAN_OK;
}

// A few words of device memory to the host, complete on return
int read_back(void* out, const void* device, size_t bytes, const ocean_fft* fft, const char* who)
{
  HIP_TRY(hipMemcpyAsync(out, device, bytes, hipMemcpyDeviceToHost, fft->stream), who);
  HIP_TRY(hipStreamSynchronize(fft->stream), who);
  return OCEAN_OK;
}

// The march of a ray cast or a render (its rules: check_march)
void set_march(RaycastParams& r, const ocean_march& m)
{
  r.step = m.step;
  r.max_steps = m.max_steps;
  r.refine = m.refine;
  r.iterations = m.iterations;
  r.tolerance = m.tolerance;
  r.slope = m.slope;
  r.pad = m.pad;
}

// The refusal of an entry point that returns a pointer: the message is set, the result is null
std::nullptr_t fail_null(const std::string& msg)
{
  fail(OCEAN_ERR_INVALID, msg);
  return nullptr;
}

// Generator i of a request lacks the data `builder` makes (none / stale: the two wordings up to its name)
int not_fresh(const std::string& who, int i, bool have, const char* none, const char* stale, const char* builder)
{
  return fail(OCEAN_ERR_INVALID, who + ": generator " + std::to_string(i) + (have ? stale : none) + " " + builder + ")");
}

}  // namespace

extern "C" {

float* ocean_generator_height_map(ocean_generator* g, int c)
{
  if (!g || c < 0 || c >= g->cascades)
    return nullptr;
  return reinterpret_cast<float*>(g->maps + (size_t)g->fft->n * g->geom.w * (2 * c));
}

float* ocean_generator_displacement_map(ocean_generator* g, int c)
{
  if (!g || c < 0 || c >= g->cascades)
    return nullptr;
  return reinterpret_cast<float*>(g->maps + (size_t)g->fft->n * g->geom.w * (2 * c + 1));
}

float* ocean_generator_jacobian_map(ocean_generator* g, int c)
{
  if (!g || c < 0 || c >= g->cascades)
    return nullptr;
  return g->jac + (size_t)g->fft->n * g->geom.w * c;
}

static int surface_params(ocean_generator* const* gens, const int* cascades, int count, SurfaceParams& p,
                          ocean_fft*& fft, const char* who)
{
  if (!gens || !cascades || count < 1 || count > kMaxSurfaceCascades)
    return fail(OCEAN_ERR_INVALID, std::string(who) + ": need 1..16 (generator, cascade) pairs");
  p = SurfaceParams{};
  p.count = count;
  fft = nullptr;
  for (int i = 0; i < count; i++)
  {
    ocean_generator* g = gens[i];
    if (!g || cascades[i] < 0 || cascades[i] >= g->cascades)
      return fail(OCEAN_ERR_INVALID, std::string(who) + ": null generator or cascade out of range");
    if (g->ranks != 1)
      return fail(OCEAN_ERR_INVALID, std::string(who) + ": slab generators hold row slabs, not whole maps");
    if (!fft)
      fft = g->fft;
    else if (g->fft->n != fft->n)
      return fail(OCEAN_ERR_INVALID, std::string(who) + ": all cascades must share one map size");
    const int c = cascades[i];
    p.c[i].height = reinterpret_cast<const float4*>(ocean_generator_height_map(g, c));
    p.c[i].disp = reinterpret_cast<const float4*>(ocean_generator_displacement_map(g, c));
    p.c[i].jac = ocean_generator_jacobian_map(g, c);
    p.c[i].plane = g->settings[c].planeSize;
    p.c[i].scale = g->settings[c].displacement;
  }
  p.n = fft->n;
  p.atlas = nullptr;
  return OCEAN_OK;
}

// The surface atlas of a request that uses one (surface_use_atlas / surface_query_use_atlas), owned by the
// plan whose stream runs the request: requests on one plan are stream-ordered, so one buffer serves them all.
static int surface_atlas(ocean_fft* fft, SurfaceParams& p, bool use, const char* who)
{
  if (!use)
    return OCEAN_OK;
  const size_t texels = surface_atlas_texels(p);
  if (fft->surf_atlas_texels < texels)
  {
    if (fft->surf_atlas)
    {
      HIP_TRY(hipStreamSynchronize(fft->stream), who);  // an earlier request may still read the old one
      HIP_TRY(hipFree(fft->surf_atlas), who);
      fft->surf_atlas = nullptr;
      fft->surf_atlas_texels = 0;
    }
    HIP_TRY(hipMalloc(&fft->surf_atlas, texels * sizeof(float4)), who);
    fft->surf_atlas_texels = texels;
  }
  p.atlas = fft->surf_atlas;
  return OCEAN_OK;
}

int ocean_surface_sample(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                         int64_t points, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_sample"));
  TRY(check_points(points, xz, out, "ocean_surface_sample"));
  TRY(surface_atlas(fft, p, surface_use_atlas(p, points), "ocean_surface_sample"));
  HIP_TRY(launch_surface(p, SurfacePlane{}, reinterpret_cast<const float2*>(xz), points, reinterpret_cast<float4*>(out),
                         fft->stream, fft->cus),
          "ocean_surface_sample");
  return OCEAN_OK;
}

int ocean_surface_query(ocean_generator* const* gens, const int* cascades, int count, const float* xz, int64_t points,
                        int iterations, float tolerance, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_query"));
  TRY(check_fixed_point(iterations, tolerance, "ocean_surface_query"));
  TRY(check_points(points, xz, out, "ocean_surface_query"));
  TRY(surface_atlas(fft, p, surface_query_use_atlas(p, points, iterations), "ocean_surface_query"));
  HIP_TRY(launch_surface_query(p, reinterpret_cast<const float2*>(xz), points, iterations, tolerance,
                               reinterpret_cast<float4*>(out), fft->stream, fft->cus),
          "ocean_surface_query");
  return OCEAN_OK;
}

int ocean_surface_sample_plane(ocean_generator* const* gens, const int* cascades, int count, const float camera[5],
                               int res, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  SurfacePlane plane;
  int64_t pts;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_sample_plane"));
  TRY(plane_request(camera, res, out, "ocean_surface_sample_plane", plane, pts));
  TRY(surface_atlas(fft, p, surface_use_atlas(p, pts), "ocean_surface_sample_plane"));
  HIP_TRY(launch_surface(p, plane, nullptr, pts, reinterpret_cast<float4*>(out), fft->stream, fft->cus),
          "ocean_surface_sample_plane");
  return OCEAN_OK;
}

// ---- mip pyramid and footprint-aware sampling ----
int ocean_generator_mip_levels(const ocean_generator* g) { return g ? g->fft->logn + 1 : 0; }

int ocean_generator_build_mips(ocean_generator* g)
{
  TRY(whole_maps(g, false, "ocean_generator_build_mips"));
  ocean_fft* f = g->fft;
  TRY(alloc_once(g->mips, (size_t)g->cascades * mip_cascade_floats(f->n) * sizeof(float), "ocean_generator_build_mips"));
  g->mips_fresh = false;
  HIP_TRY(launch_build_mips(f->n, g->cascades, g->maps, g->jac, g->mips, f->stream), "ocean_generator_build_mips");
  g->mips_fresh = true;
  return OCEAN_OK;
}

// Level `level` of map `map` (0 heightMap, 1 displacementMap, 2 jacobian) of cascade c
static float* generator_mip(ocean_generator* g, int c, int level, int map, const char* who)
{
  if (!g || c < 0 || c >= g->cascades)
    return fail_null(std::string(who) + ": null generator or cascade out of range");
  if (level < 0 || level > g->fft->logn)
    return fail_null(std::string(who) + ": level outside 0..log2(N)");
  if (level == 0)
    return map == 0 ? ocean_generator_height_map(g, c)
                    : (map == 1 ? ocean_generator_displacement_map(g, c) : ocean_generator_jacobian_map(g, c));
  if (!g->mips)
    return fail_null(std::string(who) + ": the pyramid was never built (ocean_generator_build_mips)");
  const int n = g->fft->n;
  const size_t chain = mip_chain_texels(n), off = mip_level_offset(n, level);
  float* base = g->mips + (size_t)c * mip_cascade_floats(n);
  return map == 2 ? base + 8 * chain + off : base + (size_t)map * 4 * chain + 4 * off;
}

float* ocean_generator_height_mip(ocean_generator* g, int c, int level)
{
  return generator_mip(g, c, level, 0, "ocean_generator_height_mip");
}

float* ocean_generator_displacement_mip(ocean_generator* g, int c, int level)
{
  return generator_mip(g, c, level, 1, "ocean_generator_displacement_mip");
}

float* ocean_generator_jacobian_mip(ocean_generator* g, int c, int level)
{
  return generator_mip(g, c, level, 2, "ocean_generator_jacobian_mip");
}

// surface_params of a LOD call: also the chains, which must be built and not older than the maps
static int surface_params_lod(ocean_generator* const* gens, const int* cascades, int count, SurfaceParams& p,
                              ocean_fft*& fft, const char* who)
{
  TRY(surface_params(gens, cascades, count, p, fft, who));
  for (int i = 0; i < count; i++)
  {
    ocean_generator* g = gens[i];
    if (!g->mips || !g->mips_fresh)
      return not_fresh(who, i, g->mips, " has no mip pyramid (call",
                       " has a stale mip pyramid (its maps were rewritten since", "ocean_generator_build_mips");
    const size_t chain = mip_chain_texels(fft->n);
    const float* base = g->mips + (size_t)cascades[i] * mip_cascade_floats(fft->n);
    p.c[i].height_mip = reinterpret_cast<const float4*>(base);
    p.c[i].disp_mip = reinterpret_cast<const float4*>(base + 4 * chain);
    p.c[i].jac_mip = base + 8 * chain;
  }
  return OCEAN_OK;
}

int ocean_surface_sample_lod(ocean_generator* const* gens, const int* cascades, int count, const float* xzf,
                             int64_t points, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params_lod(gens, cascades, count, p, fft, "ocean_surface_sample_lod"));
  TRY(check_points(points, xzf, out, "ocean_surface_sample_lod"));
  HIP_TRY(launch_surface_lod(p, SurfacePlane{}, xzf, points, reinterpret_cast<float4*>(out), fft->stream, fft->cus),
          "ocean_surface_sample_lod");
  return OCEAN_OK;
}

int ocean_surface_sample_plane_lod(ocean_generator* const* gens, const int* cascades, int count, const float camera[5],
                                   int res, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  SurfacePlane plane;
  int64_t pts;
  TRY(surface_params_lod(gens, cascades, count, p, fft, "ocean_surface_sample_plane_lod"));
  TRY(plane_request(camera, res, out, "ocean_surface_sample_plane_lod", plane, pts));
  HIP_TRY(launch_surface_lod(p, plane, nullptr, pts, reinterpret_cast<float4*>(out), fft->stream, fft->cus),
          "ocean_surface_sample_plane_lod");
  return OCEAN_OK;
}

// ---- time derivative of the maps and the velocity of water particles ----
int ocean_generator_calculate_rates(ocean_generator* g)
{
  TRY(whole_maps(g, true, "ocean_generator_calculate_rates"));
  ocean_fft* f = g->fft;
  const size_t nn = (size_t)f->n * f->n;
  TRY(alloc_once(g->rates, (size_t)g->cascades * 2 * nn * sizeof(float4), "ocean_generator_calculate_rates"));
  g->rates_fresh = false;
  // after fused re-seed frames the h0 image is still to be written: on the generator's stream, so with
  // frame overlap the next column pass waits for it (h0_dirty, set by the write); the memo keeps its inputs
  TRY(materialise_h0(g));
  HIP_TRY(launch_rates_pack(f->logn, g->frame, g->h0_block, g->h0, g->rates, f->stream, f->cus),
          "ocean_generator_calculate_rates");
  TRY(ocean_fft_encode_ifft_batch(f, reinterpret_cast<float*>(g->rates), 2 * g->cascades));
  g->rates_fresh = true;
  return OCEAN_OK;
}

// Image `image` (0 height-rate, 1 displacement-rate) of cascade c
static float* generator_rate_map(ocean_generator* g, int c, int image, const char* who)
{
  if (!g || c < 0 || c >= g->cascades)
    return fail_null(std::string(who) + ": null generator or cascade out of range");
  if (!g->rates)
    return fail_null(std::string(who) + ": the rates were never calculated (ocean_generator_calculate_rates)");
  return reinterpret_cast<float*>(g->rates + (size_t)g->fft->n * g->fft->n * (2 * c + image));
}

float* ocean_generator_height_rate_map(ocean_generator* g, int c)
{
  return generator_rate_map(g, c, 0, "ocean_generator_height_rate_map");
}

float* ocean_generator_displacement_rate_map(ocean_generator* g, int c)
{
  return generator_rate_map(g, c, 1, "ocean_generator_displacement_rate_map");
}

// The rate maps of a request's cascades, which must be calculated and not older than the maps
static int surface_rates(ocean_generator* const* gens, const int* cascades, int count, const ocean_fft* fft,
                         SurfaceRates& r, const char* who)
{
  r = SurfaceRates{};
  for (int i = 0; i < count; i++)
  {
    ocean_generator* g = gens[i];
    if (!g->rates || !g->rates_fresh)
      return not_fresh(who, i, g->rates, " has no rates (call", " has stale rates (a frame was calculated since",
                       "ocean_generator_calculate_rates");
    const size_t nn = (size_t)fft->n * fft->n;
    r.height[i] = g->rates + nn * (2 * cascades[i]);
    r.disp[i] = g->rates + nn * (2 * cascades[i] + 1);
  }
  return OCEAN_OK;
}

int ocean_surface_velocity(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                           int64_t points, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  SurfaceRates r;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_velocity"));
  TRY(surface_rates(gens, cascades, count, fft, r, "ocean_surface_velocity"));
  TRY(check_points(points, xz, out, "ocean_surface_velocity"));
  HIP_TRY(launch_surface_velocity(p, r, reinterpret_cast<const float2*>(xz), points, reinterpret_cast<float4*>(out),
                                  fft->stream, fft->cus),
          "ocean_surface_velocity");
  return OCEAN_OK;
}

// ---- depth layers: water velocity and pressure head below the surface ----
int ocean_generator_set_depth_layers(ocean_generator* g, const float* depths, int layers)
{
  // the list's own rules first: they need no generator
  if (!depths || layers < 1 || layers > kMaxDepthLayers)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_depth_layers: need 1..8 depths");
  for (int l = 0; l < layers; l++)
    if (!std::isfinite(depths[l]) || !(depths[l] >= 0.0f) || (l > 0 && !(depths[l] > depths[l - 1])))
      return fail(OCEAN_ERR_INVALID,
                  "ocean_generator_set_depth_layers: depths must be finite, >= 0 and strictly ascending");
  TRY(whole_maps(g, false, "ocean_generator_set_depth_layers"));
  if (g->kin && layers != g->depths.layers)
  {
    // an earlier calculate_kinematics or ocean_water_kinematics may still use the old storage
    HIP_TRY(hipStreamSynchronize(g->fft->stream), "ocean_generator_set_depth_layers");
    HIP_TRY(hipFree(g->kin), "ocean_generator_set_depth_layers");
    g->kin = nullptr;
  }
  g->depths = KinematicsDepths{};
  g->depths.layers = layers;
  for (int l = 0; l < layers; l++)
    g->depths.d[l] = depths[l];
  g->kin_fresh = false;
  return OCEAN_OK;
}

int ocean_generator_depth_layers(const ocean_generator* g, float out[8])
{
  if (!g)
    return 0;
  for (int l = 0; out && l < g->depths.layers; l++)
    out[l] = g->depths.d[l];
  return g->depths.layers;
}

int ocean_generator_calculate_kinematics(ocean_generator* g)
{
  TRY(whole_maps(g, true, "ocean_generator_calculate_kinematics"));
  if (g->depths.layers < 1)
    return fail(OCEAN_ERR_INVALID,
                "ocean_generator_calculate_kinematics: no depth layers set (ocean_generator_set_depth_layers)");
  ocean_fft* f = g->fft;
  const size_t nn = (size_t)f->n * f->n;
  const int images = 2 * g->depths.layers * g->cascades;
  TRY(alloc_once(g->kin, (size_t)images * nn * sizeof(float4), "ocean_generator_calculate_kinematics"));
  g->kin_fresh = false;
  TRY(materialise_h0(g));  // as ocean_generator_calculate_rates
  HIP_TRY(launch_kinematics_pack(f->logn, g->frame, g->depths, g->h0_block, g->h0, g->kin, f->stream, f->cus),
          "ocean_generator_calculate_kinematics");
  TRY(ocean_fft_encode_ifft_batch(f, reinterpret_cast<float*>(g->kin), images));
  g->kin_fresh = true;
  return OCEAN_OK;
}

float* ocean_generator_kinematics_map(ocean_generator* g, int c, int layer, int image)
{
  const char* who = "ocean_generator_kinematics_map";
  if (!g || c < 0 || c >= g->cascades)
    return fail_null(std::string(who) + ": null generator or cascade out of range");
  if (!g->kin)
    return fail_null(std::string(who) +
                     ": the depth layers were never calculated (ocean_generator_calculate_kinematics)");
  if (layer < 0 || layer >= g->depths.layers || image < 0 || image > 1)
    return fail_null(std::string(who) + ": layer or image out of range");
  const size_t nn = (size_t)g->fft->n * g->fft->n;
  return reinterpret_cast<float*>(g->kin + nn * (((size_t)c * g->depths.layers + layer) * 2 + image));
}

// The layer maps of the pairs surface_params accepted, beside SurfaceParams' maps: every generator's layers
// calculated, fresh and of gens[0]'s depth list
static int water_layers(ocean_generator* const* gens, const int* cascades, int count, const ocean_fft* fft,
                        WaterLayers& w, const char* who)
{
  w = WaterLayers{};
  const KinematicsDepths& first = gens[0]->depths;
  const size_t nn = (size_t)fft->n * fft->n;
  for (int i = 0; i < count; i++)
  {
    ocean_generator* g = gens[i];
    if (!g->kin || !g->kin_fresh)
      return not_fresh(who, i, g->kin, " has no depth layers (call",
                       " has stale depth layers (a frame was calculated or the depths were set since",
                       "ocean_generator_calculate_kinematics");
    if (g->depths.layers != first.layers ||
        std::memcmp(g->depths.d, first.d, sizeof(float) * (size_t)first.layers) != 0)
      return fail(OCEAN_ERR_INVALID, std::string(who) + ": generator " + std::to_string(i) +
                                         " has other depth layers than generator 0 (ocean_generator_set_depth_layers)");
    w.map[i] = g->kin + nn * ((size_t)cascades[i] * first.layers * 2);
  }
  w.layers = first.layers;
  for (int l = 0; l < first.layers; l++)
    w.d[l] = first.d[l];
  return OCEAN_OK;
}

int ocean_water_kinematics(ocean_generator* const* gens, const int* cascades, int count, const float* xyz,
                           int64_t points, int iterations, float tolerance, float* out)
{
  const char* who = "ocean_water_kinematics";
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, who));
  TRY(check_fixed_point(iterations, tolerance, who));
  WaterLayers w;
  TRY(water_layers(gens, cascades, count, fft, w, who));
  TRY(check_points(points, xyz, out, who));
  HIP_TRY(launch_water_kinematics(p, w, xyz, points, iterations, tolerance, reinterpret_cast<float4*>(out),
                                  fft->stream, fft->cus),
          who);
  return OCEAN_OK;
}

// ---- bounds of the maps and ray casting against the displaced surface ----
int ocean_generator_build_bounds(ocean_generator* g)
{
  TRY(whole_maps(g, true, "ocean_generator_build_bounds"));
  ocean_fft* f = g->fft;
  TRY(alloc_once(g->bounds, bounds_floats(f->n, g->cascades) * sizeof(float), "ocean_generator_build_bounds"));
  g->bounds_fresh = false;
  HIP_TRY(launch_build_bounds(f->n, g->cascades, g->maps, g->jac, g->bounds, f->stream, f->cus),
          "ocean_generator_build_bounds");
  g->bounds_fresh = true;
  return OCEAN_OK;
}

// The table of a generator whose bounds are built and not older than its maps, else null with a message
static const float* generator_bounds(ocean_generator* g, const char* who)
{
  if (!g)
    return fail_null(std::string(who) + ": null generator");
  if (!g->bounds || !g->bounds_fresh)
    return fail_null(std::string(who) + (g->bounds ? ": the bounds are stale (the maps were rewritten since"
                                                   : ": the bounds were never built (call") +
                     " ocean_generator_build_bounds)");
  return g->bounds;
}

const float* ocean_generator_bounds_device(ocean_generator* g)
{
  return generator_bounds(g, "ocean_generator_bounds_device");
}

int ocean_generator_bounds(ocean_generator* g, int cascade, float out[18])
{
  const float* table = generator_bounds(g, "ocean_generator_bounds");
  if (!table)
    return OCEAN_ERR_INVALID;
  if (cascade < 0 || cascade >= g->cascades || !out)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_bounds: cascade out of range or null output");
  return read_back(out, table + (size_t)cascade * 18, 18 * sizeof(float), g->fft, "ocean_generator_bounds");
}

// The bounds rows of a request's cascades, which must be built and not older than the maps
static int surface_bounds_rows(ocean_generator* const* gens, const int* cascades, int count, RaycastParams& r,
                               const char* who)
{
  for (int i = 0; i < count; i++)
  {
    ocean_generator* g = gens[i];
    if (!g->bounds || !g->bounds_fresh)
      return not_fresh(who, i, g->bounds, " has no bounds (call", " has stale bounds (its maps were rewritten since",
                       "ocean_generator_build_bounds");
    r.bounds[i] = g->bounds + (size_t)cascades[i] * 18;
  }
  return OCEAN_OK;
}

int ocean_surface_raycast(ocean_generator* const* gens, const int* cascades, int count, const float* rays,
                          int64_t n_rays, float step, int max_steps, int refine, int iterations, float tolerance,
                          float slope, float pad, float* out)
{
  // the scalar rules first: they need no generator
  if (!gens || !cascades)
    return fail(OCEAN_ERR_INVALID, "ocean_surface_raycast: null gens / cascades");
  TRY(check_march(step, max_steps, refine, iterations, tolerance, slope, pad, "ocean_surface_raycast"));
  if (n_rays < 0 || (n_rays > 0 && (!rays || !out)))
    return fail(OCEAN_ERR_INVALID, "ocean_surface_raycast: null rays/output or negative count");
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_raycast"));
  RaycastParams r{};
  TRY(surface_bounds_rows(gens, cascades, count, r, "ocean_surface_raycast"));
  set_march(r, ocean_march{step, max_steps, refine, iterations, tolerance, slope, pad});
  HIP_TRY(launch_surface_raycast(p, r, reinterpret_cast<const float4*>(rays), n_rays, reinterpret_cast<float4*>(out),
                                 fft->stream, fft->cus),
          "ocean_surface_raycast");
  return OCEAN_OK;
}

// ---- camera images: ray-cast pixels shaded with the reference's water, sky and fog ----
void ocean_default_camera(ocean_camera* c)
{
  if (!c)
    return;
  const double deg = 3.14159265358979323846 / 180.0;
  const double p = -5.0 * deg, y = -135.0 * deg;  // src/Renderer.cpp:16
  const double f[3] = {std::cos(p) * std::sin(y), std::sin(p), -std::cos(p) * std::cos(y)};
  const double r[3] = {std::cos(y), 0.0, std::sin(y)};
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  *c = ocean_camera{};
  c->position[1] = 5.0f;
  for (int k = 0; k < 3; k++)
  {
    c->right[k] = (float)r[k];
    c->up[k] = (float)u[k];
    c->forward[k] = (float)f[k];
  }
  c->tan_half_fov_y = (float)std::tan(22.5 * deg);  // a 45 degree vertical field of view: this library's choice
  c->near_plane = 1.0f;
  c->far_plane = 1500.0f;
  c->lod_scale = 0.0f;
}

void ocean_default_shading(ocean_shading* s)
{
  if (s)  // src/Renderer.h:22-29, waveShader.glsl:230
    *s = ocean_shading{{0.0f, 0.33f, 0.47f}, {0.5f, 0.8f, 0.9f}, {0.53f, 0.8f, 0.94f}, {1.0f, 1.0f, 1.0f},
                       {0.703f, 0.105f, 0.703f}, 3.0f, 1.0f, 30.0f, 0.0025f};
}

void ocean_default_march(ocean_march* m)
{
  if (m)
    *m = ocean_march{0.25f, 256, 10, 4, 1e-3f, 1.0f, 0.0f};
}

// The camera's own rules and its kernel argument
static int camera_params(const ocean_camera* c, int width, int height, CameraParams& cam, const std::string& who)
{
  if (width < 1 || width > 16384 || height < 1 || height > 16384)
    return fail(OCEAN_ERR_INVALID, who + ": width or height outside 1..16384");
  const float* entries = c->position;  // 15 floats, then lod_scale
  static_assert(sizeof(ocean_camera) == 16 * sizeof(float), "ocean_camera is 16 floats");
  for (int k = 0; k < 15; k++)
    if (!std::isfinite(entries[k]))
      return fail(OCEAN_ERR_INVALID, who + ": non-finite camera entry");
  if (!(c->tan_half_fov_y > 0.0f))
    return fail(OCEAN_ERR_INVALID, who + ": tan_half_fov_y must be > 0");
  if (c->near_plane < 0.0f || c->near_plane >= c->far_plane)
    return fail(OCEAN_ERR_INVALID, who + ": near_plane must be >= 0 and below far_plane");
  if (!(c->lod_scale >= 0.0f) || !std::isfinite(c->lod_scale))
    return fail(OCEAN_ERR_INVALID, who + ": lod_scale must be finite and >= 0");
  cam = CameraParams{};
  for (int k = 0; k < 3; k++)
  {
    cam.pos[k] = c->position[k];
    cam.right[k] = c->right[k];
    cam.up[k] = c->up[k];
    cam.fwd[k] = c->forward[k];
  }
  cam.tan_half = c->tan_half_fov_y;
  cam.near_plane = c->near_plane;
  cam.far_plane = c->far_plane;
  cam.lod_scale = c->lod_scale;
  cam.width = width;
  cam.height = height;
  return OCEAN_OK;
}

int ocean_camera_rays(const ocean_camera* camera, int width, int height, float* rays, void* hip_stream)
{
  const std::string who = "ocean_camera_rays";
  if (!camera)
    return fail(OCEAN_ERR_INVALID, who + ": null camera");
  CameraParams cam;
  TRY(camera_params(camera, width, height, cam, who));
  if (!rays)
    return fail(OCEAN_ERR_INVALID, who + ": null rays");
  HIP_TRY(launch_camera_rays(cam, reinterpret_cast<float4*>(rays), static_cast<hipStream_t>(hip_stream)), who.c_str());
  return OCEAN_OK;
}

// The rules of a render that need no generator, in the contract's order up to the outputs, and the camera's
// and the shading's kernel arguments (ocean_camera_render, ocean_camera_render_layers)
static int camera_scalars(ocean_generator* const* gens, const int* cascades, const ocean_camera* camera,
                          const ocean_shading* shading, const ocean_march* march, int width, int height,
                          CameraParams& cam, ShadingParams& sh, const std::string& who)
{
  if (!gens || !cascades)
    return fail(OCEAN_ERR_INVALID, who + ": null gens / cascades");
  if (!camera)
    return fail(OCEAN_ERR_INVALID, who + ": null camera");
  if (!shading)
    return fail(OCEAN_ERR_INVALID, who + ": null shading");
  if (!march)
    return fail(OCEAN_ERR_INVALID, who + ": null march");
  TRY(camera_params(camera, width, height, cam, who));
  static_assert(sizeof(ocean_shading) == 19 * sizeof(float), "ocean_shading is 19 floats");
  const float* entries = shading->wave_color;
  for (int k = 0; k < 19; k++)
    if (!std::isfinite(entries[k]))
      return fail(OCEAN_ERR_INVALID, who + ": non-finite shading entry");
  const double lx = shading->light_direction[0], ly = shading->light_direction[1], lz = shading->light_direction[2];
  const double ll = std::sqrt(lx * lx + ly * ly + lz * lz);
  if (!(ll > 0.0))
    return fail(OCEAN_ERR_INVALID, who + ": light_direction is zero");
  if (shading->sun_view_angle < 0.0f)
    return fail(OCEAN_ERR_INVALID, who + ": sun_view_angle must be >= 0");
  if (shading->sun_falloff_angle < 0.0f)
    return fail(OCEAN_ERR_INVALID, who + ": sun_falloff_angle must be >= 0");
  if (shading->fog_density < 0.0f)
    return fail(OCEAN_ERR_INVALID, who + ": fog_density must be >= 0");
  TRY(check_march(march->step, march->max_steps, march->refine, march->iterations, march->tolerance, march->slope,
                  march->pad, who));
  sh = ShadingParams{};
  for (int k = 0; k < 3; k++)
  {
    sh.wave[k] = shading->wave_color[k];
    sh.scatter[k] = shading->scatter_color[k];
    sh.sky[k] = shading->sky_color[k];
    sh.light[k] = shading->light_color[k];
    sh.L[k] = (float)((double)shading->light_direction[k] / ll);
  }
  // waveShader.glsl:48-49 (DEGREE_TO_RADIANS 0.0174533), in double, rounded once
  sh.cthr = (float)std::cos((double)shading->sun_view_angle * 0.0174533);
  sh.cfade = (float)std::cos(((double)shading->sun_view_angle + std::max((double)shading->sun_falloff_angle, 0.01)) *
                             0.0174533);
  sh.fog_begin = shading->fog_begin;
  sh.fog_density = shading->fog_density;
  return OCEAN_OK;
}

// The generators' part of a render: the maps (the pyramids with lod_scale > 0), the bounds rows and the march
static int camera_scene(ocean_generator* const* gens, const int* cascades, int count, const CameraParams& cam,
                        const ocean_march* march, SurfaceParams& p, RaycastParams& r, ocean_fft*& fft,
                        const std::string& who)
{
  if (cam.lod_scale > 0.0f)
    TRY(surface_params_lod(gens, cascades, count, p, fft, who.c_str()));
  else
    TRY(surface_params(gens, cascades, count, p, fft, who.c_str()));
  r = RaycastParams{};
  TRY(surface_bounds_rows(gens, cascades, count, r, who.c_str()));
  set_march(r, *march);
  return OCEAN_OK;
}

int ocean_camera_render(ocean_generator* const* gens, const int* cascades, int count, const ocean_camera* camera,
                        const ocean_shading* shading, const ocean_march* march, int width, int height, float* image,
                        float* aux, uint8_t* image8)
{
  const std::string who = "ocean_camera_render";
  CameraParams cam;
  ShadingParams sh;
  TRY(camera_scalars(gens, cascades, camera, shading, march, width, height, cam, sh, who));
  if (!image && !aux && !image8)
    return fail(OCEAN_ERR_INVALID, who + ": all three outputs are null");
  SurfaceParams p;
  RaycastParams r;
  ocean_fft* fft;
  TRY(camera_scene(gens, cascades, count, cam, march, p, r, fft, who));
  HIP_TRY(launch_camera_render(p, r, cam, sh, reinterpret_cast<float4*>(image), reinterpret_cast<float4*>(aux),
                               reinterpret_cast<uint32_t*>(image8), fft->stream, fft->cus),
          who.c_str());
  return OCEAN_OK;
}

// ---- persistent foam: per-cascade accumulation, coverage counts, sampler ----
void ocean_default_foam_settings(ocean_foam_settings* s)
{
  if (s)
    *s = ocean_foam_settings{0.9f, 8.0f, 0.5f, 0.5f};
}

ocean_foam_settings* ocean_generator_foam_settings(ocean_generator* g, int c)
{
  if (!g || c < 0 || c >= g->cascades)
    return fail_null("ocean_generator_foam_settings: null generator or cascade out of range");
  return &g->foam_settings[c];
}

// The foam maps and counts of a whole-grid generator: allocated, and zeroed on its stream, on first use
static int foam_storage(ocean_generator* g, const std::string& who)
{
  if (g->foam)
    return OCEAN_OK;
  ocean_fft* f = g->fft;
  const size_t map_bytes = (size_t)g->cascades * f->n * f->n * sizeof(float);
  const size_t count_bytes = foam_counts_bytes(f->n, g->cascades);
  float* maps = nullptr;
  void* counts = nullptr;
  hipError_t e = alloc_if_null(maps, map_bytes);
  e = alloc_if_null(counts, count_bytes, e);
  if (e == hipSuccess)
    e = hipMemsetAsync(maps, 0, map_bytes, f->stream);
  if (e == hipSuccess)
    e = hipMemsetAsync(counts, 0, count_bytes, f->stream);
  if (e != hipSuccess)
  {
    if (maps || counts)
      (void)hipStreamSynchronize(f->stream);  // a memset of the buffer about to be freed may be in flight
    if (maps)
      (void)hipFree(maps);
    if (counts)
      (void)hipFree(counts);
    return alloc_fail(e, who);
  }
  g->foam = maps;
  g->foam_counts = counts;
  return OCEAN_OK;
}

int ocean_generator_advance_foam(ocean_generator* g, float dt)
{
  const std::string who = "ocean_generator_advance_foam";
  TRY(whole_maps(g, true, who));
  TRY(check_dt(dt, who));
  FoamCascade fc[kMaxCascades];
  for (int c = 0; c < g->cascades; c++)
  {
    const ocean_foam_settings& s = g->foam_settings[c];
    if (!std::isfinite(s.bias) || !std::isfinite(s.level))
      return fail(OCEAN_ERR_INVALID, who + ": cascade " + std::to_string(c) + " has a non-finite bias or level");
    if (!(s.gain >= 0.0f) || !std::isfinite(s.gain) || !(s.decay >= 0.0f) || !std::isfinite(s.decay))
      return fail(OCEAN_ERR_INVALID,
                  who + ": cascade " + std::to_string(c) + " needs gain and decay finite and >= 0");
    fc[c] = FoamCascade{(float)std::exp(-(double)s.decay * (double)dt), s.bias, s.gain, s.level, dt};
  }
  TRY(foam_storage(g, who));
  ocean_fft* f = g->fft;
  HIP_TRY(launch_foam_step(f->n, g->cascades, g->jac, g->foam, g->foam_counts, fc, f->stream, f->cus), who.c_str());
  return OCEAN_OK;
}

int ocean_generator_reset_foam(ocean_generator* g)
{
  const std::string who = "ocean_generator_reset_foam";
  TRY(whole_maps(g, false, who));
  if (!g->foam)
    return foam_storage(g, who);  // zeroed as allocated
  ocean_fft* f = g->fft;
  HIP_TRY(hipMemsetAsync(g->foam, 0, (size_t)g->cascades * f->n * f->n * sizeof(float), f->stream), who.c_str());
  HIP_TRY(hipMemsetAsync(g->foam_counts, 0, foam_counts_bytes(f->n, g->cascades), f->stream), who.c_str());
  if (g->deposit_acc)  // zero between calls already: a reset also clears what a failed deposit may have left
    HIP_TRY(hipMemsetAsync(g->deposit_acc, 0, (size_t)g->cascades * f->n * f->n * sizeof(unsigned long long), f->stream),
            who.c_str());
  return OCEAN_OK;
}

// A generator with foam storage, else null with a message
static ocean_generator* generator_foam(ocean_generator* g, const char* who)
{
  if (!g)
    return fail_null(std::string(who) + ": null generator");
  if (!g->foam)
    return fail_null(std::string(who) + ": the generator has no foam yet (call ocean_generator_advance_foam or "
                                        "ocean_generator_reset_foam)");
  return g;
}

float* ocean_generator_foam_map(ocean_generator* g, int c)
{
  if (!generator_foam(g, "ocean_generator_foam_map"))
    return nullptr;
  if (c < 0 || c >= g->cascades)
    return fail_null("ocean_generator_foam_map: cascade out of range");
  return g->foam + (size_t)g->fft->n * g->fft->n * c;
}

const int64_t* ocean_generator_foam_counts_device(ocean_generator* g)
{
  return generator_foam(g, "ocean_generator_foam_counts_device") ? static_cast<const int64_t*>(g->foam_counts) : nullptr;
}

int ocean_generator_foam_counts(ocean_generator* g, int cascade, int64_t out[3])
{
  if (!generator_foam(g, "ocean_generator_foam_counts"))
    return OCEAN_ERR_INVALID;
  if (cascade < 0 || cascade >= g->cascades || !out)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_foam_counts: cascade out of range or null output");
  return read_back(out, static_cast<const int64_t*>(g->foam_counts) + (size_t)cascade * 3, 3 * sizeof(int64_t), g->fft,
                   "ocean_generator_foam_counts");
}

// The foam maps of a request's cascades: every generator must have foam storage
static int surface_foam(ocean_generator* const* gens, const int* cascades, int count, const ocean_fft* fft,
                        SurfaceFoam& f, const char* who)
{
  f = SurfaceFoam{};
  for (int i = 0; i < count; i++)
  {
    if (!gens[i]->foam)
      return not_fresh(who, i, false, " has no foam (call", "", "ocean_generator_advance_foam or ocean_generator_reset_foam");
    f.foam[i] = gens[i]->foam + (size_t)fft->n * fft->n * cascades[i];
  }
  return OCEAN_OK;
}

int ocean_surface_sample_foam(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                              int64_t points, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  SurfaceFoam f;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_sample_foam"));
  TRY(surface_foam(gens, cascades, count, fft, f, "ocean_surface_sample_foam"));
  TRY(check_points(points, xz, out, "ocean_surface_sample_foam"));
  HIP_TRY(launch_surface_foam(p, f, SurfacePlane{}, reinterpret_cast<const float2*>(xz), points,
                              reinterpret_cast<float4*>(out), fft->stream, fft->cus),
          "ocean_surface_sample_foam");
  return OCEAN_OK;
}

int ocean_surface_sample_plane_foam(ocean_generator* const* gens, const int* cascades, int count,
                                    const float camera[5], int res, float* out)
{
  SurfaceParams p;
  ocean_fft* fft;
  SurfaceFoam f;
  SurfacePlane plane;
  int64_t pts;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_surface_sample_plane_foam"));
  TRY(surface_foam(gens, cascades, count, fft, f, "ocean_surface_sample_plane_foam"));
  TRY(plane_request(camera, res, out, "ocean_surface_sample_plane_foam", plane, pts));
  HIP_TRY(launch_surface_foam(p, f, plane, nullptr, pts, reinterpret_cast<float4*>(out), fft->stream, fft->cus),
          "ocean_surface_sample_plane_foam");
  return OCEAN_OK;
}

// ---- foam deposit: spray impacts splatted into the persistent foam ----
void ocean_default_foam_deposit_settings(ocean_foam_deposit_settings* s)
{
  if (s)
    *s = ocean_foam_deposit_settings{0.05f, 0.01f};
}

static bool g_deposit_merge = true;

int ocean_debug_foam_deposit_merge(int enable)
{
  const bool was = g_deposit_merge;
  g_deposit_merge = enable != 0;
  return was ? 1 : 0;
}

int ocean_foam_deposit(ocean_generator* const* gens, const int* cascades, int count,
                       const ocean_foam_deposit_settings* settings, const float* records,
                       const int64_t* count_device, int64_t max_records)
{
  const std::string who = "ocean_foam_deposit";
  // the rules that need no generator first
  if (!gens || !cascades || count < 1 || count > kMaxSurfaceCascades)
    return fail(OCEAN_ERR_INVALID, who + ": need 1..16 (generator, cascade) pairs");
  if (!settings)
    return fail(OCEAN_ERR_INVALID, who + ": null settings");
  if (max_records < 0 || max_records > ((int64_t)1 << 28) || (max_records > 0 && !records))
    return fail(OCEAN_ERR_INVALID, who + ": max_records outside 0..2^28, or null records with max_records > 0");
  for (int i = 0; i < count; i++)
  {
    const ocean_foam_deposit_settings& s = settings[i];
    if (!(s.amount >= 0.0f) || !std::isfinite(s.amount) || !(s.per_speed >= 0.0f) || !std::isfinite(s.per_speed))
      return fail(OCEAN_ERR_INVALID, who + ": pair " + std::to_string(i) + " needs amount and per_speed finite and >= 0");
  }
  SurfaceParams p;
  ocean_fft* fft;
  SurfaceFoam f;
  TRY(surface_params(gens, cascades, count, p, fft, who.c_str()));
  TRY(frames_calculated(gens, count, who));
  TRY(surface_foam(gens, cascades, count, fft, f, who.c_str()));
  for (int i = 1; i < count; i++)
    for (int j = 0; j < i; j++)
      if (gens[i] == gens[j] && cascades[i] == cascades[j])
        return fail(OCEAN_ERR_INVALID, who + ": pairs " + std::to_string(j) + " and " + std::to_string(i) +
                                           " are the same foam map: a texel has one owner per call");
  // first use: the counts of gens[0] and the accumulators of every generator with an active pair
  ocean_generator* g0 = gens[0];
  TRY(alloc_zeroed_once(g0->deposit_counts, foam_deposit_scratch_bytes(), fft->stream, who));
  const size_t nn = (size_t)fft->n * fft->n;
  FoamDepositCall c{};
  foam_deposit_scratch(g0->deposit_counts, c);
  for (int i = 0; i < count; i++)
  {
    const ocean_foam_deposit_settings& s = settings[i];
    const bool active = s.amount != 0.0f || s.per_speed != 0.0f;
    if (active)
      TRY(alloc_zeroed_once(gens[i]->deposit_acc, (size_t)gens[i]->cascades * nn * sizeof(unsigned long long), fft->stream,
                         who));
    c.c[i] = FoamDepositPair{const_cast<float*>(f.foam[i]), active ? gens[i]->deposit_acc + nn * cascades[i] : nullptr,
                             p.c[i].plane, s.amount, s.per_speed, 0};
  }
  if (max_records == 0)
  {
    HIP_TRY(hipMemsetAsync(c.table, 0, kFoamDepositCounts * sizeof(int64_t), fft->stream), who.c_str());
    return OCEAN_OK;
  }
  c.records = records;
  c.count_device = count_device;
  c.max_records = max_records;
  c.n = fft->n;
  c.pairs = count;
  HIP_TRY(launch_foam_deposit(c, g_deposit_merge, fft->stream, fft->cus), who.c_str());
  return OCEAN_OK;
}

// The first generator of an ocean_foam_deposit call, else null with a message
static ocean_generator* generator_deposited(ocean_generator* g, const char* who)
{
  if (!g)
    return fail_null(std::string(who) + ": null generator");
  if (!g->deposit_counts)
    return fail_null(std::string(who) + ": the generator was the first of no ocean_foam_deposit call yet");
  return g;
}

const int64_t* ocean_foam_deposit_counts_device(ocean_generator* gen0)
{
  return generator_deposited(gen0, "ocean_foam_deposit_counts_device") ? static_cast<const int64_t*>(gen0->deposit_counts)
                                                                       : nullptr;
}

int ocean_foam_deposit_counts(ocean_generator* gen0, int64_t out[50])
{
  if (!generator_deposited(gen0, "ocean_foam_deposit_counts"))
    return OCEAN_ERR_INVALID;
  if (!out)
    return fail(OCEAN_ERR_INVALID, "ocean_foam_deposit_counts: null output");
  return read_back(out, gen0->deposit_counts, kFoamDepositCounts * sizeof(int64_t), gen0->fft,
                   "ocean_foam_deposit_counts");
}

// ---- camera layers: the foam stage in the water pass, spray records splatted over it ----
void ocean_default_camera_layers(ocean_camera_layers* l)
{
  if (l)  // starting points, not measurements
    *l = ocean_camera_layers{{1.0f, 1.0f, 1.0f}, 0.25f, 0.75f, 1.0f, {1.0f, 1.0f, 1.0f}, 0.05f, 2, 0.25f};
}

size_t ocean_camera_layers_scratch_bytes(int width, int height)
{
  if (width < 1 || width > 16384 || height < 1 || height > 16384)
    return 0;
  return camera_layers_scratch_bytes(width, height);
}

int ocean_camera_render_layers(ocean_generator* const* gens, const int* cascades, int count,
                               const ocean_camera* camera, const ocean_shading* shading, const ocean_march* march,
                               const ocean_camera_layers* layers, int width, int height, const float* records,
                               const int64_t* count_device, int64_t max_records, void* scratch, float* image,
                               float* aux, float* aux2, uint8_t* image8)
{
  const std::string who = "ocean_camera_render_layers";
  CameraParams cam;
  ShadingParams sh;
  TRY(camera_scalars(gens, cascades, camera, shading, march, width, height, cam, sh, who));
  if (!layers)
    return fail(OCEAN_ERR_INVALID, who + ": null layers");
  const ocean_camera_layers& l = *layers;
  const float entries[12] = {l.foam_color[0], l.foam_color[1], l.foam_color[2], l.foam_lo, l.foam_hi, l.foam_opacity,
                             l.spray_color[0], l.spray_color[1], l.spray_color[2], l.spray_radius, l.spray_opacity,
                             0.0f};
  for (float v : entries)
    if (!std::isfinite(v))
      return fail(OCEAN_ERR_INVALID, who + ": non-finite layers entry");
  if (l.foam_lo >= l.foam_hi)
    return fail(OCEAN_ERR_INVALID, who + ": foam_lo must be below foam_hi");
  if (l.foam_opacity < 0.0f || l.foam_opacity > 1.0f)
    return fail(OCEAN_ERR_INVALID, who + ": foam_opacity outside 0..1");
  if (l.spray_opacity < 0.0f || l.spray_opacity > 1.0f)
    return fail(OCEAN_ERR_INVALID, who + ": spray_opacity outside 0..1");
  if (l.spray_radius < 0.0f)
    return fail(OCEAN_ERR_INVALID, who + ": spray_radius must be >= 0");
  if (l.spray_max_half < 0 || l.spray_max_half > 8)
    return fail(OCEAN_ERR_INVALID, who + ": spray_max_half outside 0..8");
  if (max_records < 0 || max_records > ((int64_t)1 << 28))
    return fail(OCEAN_ERR_INVALID, who + ": max_records outside 0..2^28");
  const bool spray = records && max_records > 0;
  if (spray && !scratch)
    return fail(OCEAN_ERR_INVALID, who + ": records need scratch (ocean_camera_layers_scratch_bytes)");
  if (!image && !aux && !aux2 && !image8)
    return fail(OCEAN_ERR_INVALID, who + ": all four outputs are null");
  SurfaceParams p;
  RaycastParams r;
  ocean_fft* fft;
  TRY(camera_scene(gens, cascades, count, cam, march, p, r, fft, who));
  SurfaceFoam fm{};
  const bool foam = l.foam_opacity > 0.0f;
  if (foam)
    TRY(surface_foam(gens, cascades, count, fft, fm, who.c_str()));
  float4* const image4 = reinterpret_cast<float4*>(image);
  float4* const aux4 = reinterpret_cast<float4*>(aux);
  float4* const aux24 = reinterpret_cast<float4*>(aux2);
  uint32_t* const bytes = reinterpret_cast<uint32_t*>(image8);
  if (!foam && !spray)
  {
    // ocean_camera_render itself: the same kernel instantiation; aux2 has nothing to say but "no spray"
    if (image || aux || image8)
      HIP_TRY(launch_camera_render(p, r, cam, sh, image4, aux4, bytes, fft->stream, fft->cus), who.c_str());
    if (aux2)
      HIP_TRY(launch_camera_aux2_none(cam, aux24, fft->stream, fft->cus), who.c_str());
    return OCEAN_OK;
  }
  CameraWaterLayers lw{};
  for (int k = 0; k < 3; k++)
    lw.foam_color[k] = l.foam_color[k];
  lw.foam_lo = l.foam_lo;
  lw.foam_hi = l.foam_hi;
  lw.foam_opacity = l.foam_opacity;
  if (!spray)
  {
    lw.aux2 = aux24;
    HIP_TRY(launch_camera_render_foam(p, r, cam, sh, fm, lw, image4, aux4, bytes, fft->stream, fft->cus), who.c_str());
    return OCEAN_OK;
  }
  // the spray pass follows: the water pass leaves its float image and aux where the composite and the splat
  // read them (the caller's, else the scratch's), and the pixel words; image8 and aux2 are the composite's
  CameraSpray s{};
  float4 *scratch_image, *scratch_aux;
  float* foam_words;
  camera_layers_scratch(scratch, width, height, s.key, s.hits, foam_words, scratch_image, scratch_aux);
  s.foam = foam_words;
  s.base = image4 ? image4 : scratch_image;
  float4* const water_aux = aux4 ? aux4 : scratch_aux;
  s.aux = water_aux;
  s.records = records;
  s.count_device = count_device;
  s.max_records = max_records;
  for (int k = 0; k < 3; k++)
    s.color[k] = l.spray_color[k];
  s.radius = l.spray_radius;
  s.opacity = l.spray_opacity;
  s.max_half = l.spray_max_half;
  lw.key = s.key;
  lw.hits = s.hits;
  lw.foam = foam_words;
  HIP_TRY(launch_camera_render_foam(p, r, cam, sh, fm, lw, s.base, water_aux, nullptr, fft->stream, fft->cus),
          who.c_str());
  HIP_TRY(launch_camera_spray(cam, sh, s, image4, bytes, aux24, fft->stream, fft->cus), who.c_str());
  return OCEAN_OK;
}

// ---- hull sets: net wave force and torque on batches of floating bodies ----
// Consecutive bodies of at most 32 points share a wave (tools/hulls_bench.py times both)
static bool g_hulls_pack = true;

int ocean_debug_hulls_packing(int enable)
{
  g_hulls_pack = enable != 0;
  return OCEAN_OK;
}

// The power of two `count` lanes fit in
static int lane_segment(int count)
{
  int seg = 1;
  while (seg < count)
    seg *= 2;
  return seg;
}

// The consecutive entries from b on that share a wave: those with b's segment size, as many as fit (1: b has
// waves of its own). counts: n x 2 int32 with the lane count second (a hull set's ranges, a mooring set's
// attach): the packing of the hull sets' bodies and the mooring sets' lines.
static int packed_run(int b, int n, const int32_t* counts)
{
  const int seg = lane_segment(counts[2 * b + 1]);
  int run = 1;
  while (g_hulls_pack && seg <= kHullTilePoints / 2 && run < kHullTilePoints / seg && b + run < n &&
         lane_segment(counts[2 * (b + run) + 1]) == seg)
    run++;
  return run;
}

struct ocean_hulls
{
  ocean_fft* fft = nullptr;
  int bodies = 0;
  int64_t instance_points = 0;
  int items = 0;    // 64-point tiles
  int n_folds = 0;  // bodies of more than one tile
  float4* points = nullptr;
  HullTile* tiles = nullptr;
  HullBody* body_table = nullptr;
  HullFold* folds = nullptr;
  float4* partial = nullptr;  // one 8-float partial per tile of a body in `folds`
  float4* props = nullptr;    // ocean_hulls_set_bodies: two float4 per body
};

int ocean_hulls_destroy(ocean_hulls* h)
{
  if (!h)
    return OCEAN_OK;
  if (h->fft)
    (void)hipStreamSynchronize(h->fft->stream);
  for (void* p : {(void*)h->points, (void*)h->tiles, (void*)h->body_table, (void*)h->folds, (void*)h->partial,
                  (void*)h->props})
    if (p)
      (void)hipFree(p);
  delete h;
  return OCEAN_OK;
}

int ocean_hulls_create(ocean_hulls** out, ocean_fft* fft, const float* points, int64_t n_points, const int32_t* ranges,
                       int bodies)
{
  if (!out || !fft || !points || !ranges)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: null argument");
  *out = nullptr;
  if (bodies < 1 || bodies > 1048576)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: bodies outside 1..1048576");
  if (n_points < 1)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: no points");
  int64_t n_tiles = 0, instance_points = 0;
  for (int b = 0; b < bodies; b++)
  {
    const int64_t first = ranges[2 * b], count = ranges[2 * b + 1];
    if (count < 1 || count > 262144)
      return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: body " + std::to_string(b) + " has a count outside 1..262144");
    if (first < 0 || first + count > n_points)
      return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: the range of body " + std::to_string(b) + " leaves the points");
    n_tiles += (count + kHullTilePoints - 1) / kHullTilePoints;
    instance_points += count;
  }
  for (int64_t i = 0; i < n_points; i++)
  {
    const float* l = points + 8 * i;
    for (int k = 0; k < 8; k++)
      if (!std::isfinite(l[k]))
        return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: point " + std::to_string(i) + " has a non-finite field");
    if (l[3] < 0.0f || !(l[4] > 0.0f) || l[5] < 0.0f || l[6] < 0.0f)
      return fail(OCEAN_ERR_INVALID, "ocean_hulls_create: point " + std::to_string(i) +
                                         " needs volume >= 0, half_height > 0 and drag coefficients >= 0");
  }
  if (n_tiles > INT32_MAX)
    return fail(OCEAN_ERR_OOM, "ocean_hulls_create: more than 2^31 - 1 tiles of 64 points");

  // the work items, in the order of the bodies: a body's 64-point tiles, or one packed tile for a run of
  // consecutive small bodies with one segment size; point_out rows in the order of the bodies
  std::vector<HullTile> tiles;
  std::vector<HullBody> table((size_t)bodies);
  std::vector<HullFold> folds;
  tiles.reserve((size_t)n_tiles);
  int slot = 0;
  int64_t rows = 0;
  for (int b = 0; b < bodies; b++)
  {
    table[b] = HullBody{rows, ranges[2 * b], ranges[2 * b + 1]};
    rows += ranges[2 * b + 1];
  }
  for (int b = 0; b < bodies; b++)
  {
    const int first = ranges[2 * b], count = ranges[2 * b + 1];
    const int seg = lane_segment(count);
    const int run = packed_run(b, bodies, ranges);
    if (run > 1)
    {
      HullTile t{};
      t.count = run;
      t.body = b;
      t.slot = -1;
      t.seg = seg;
      tiles.push_back(t);
      b += run - 1;
      continue;
    }
    const int64_t offset = table[b].offset;
    const int nt = (count + kHullTilePoints - 1) / kHullTilePoints;
    if (nt > 1)
      folds.push_back(HullFold{b, slot, nt, 0});
    for (int j = 0; j < nt; j++)
      tiles.push_back(HullTile{offset + (int64_t)j * kHullTilePoints, first + j * kHullTilePoints,
                               std::min(kHullTilePoints, count - j * kHullTilePoints), b, nt > 1 ? slot + j : -1});
    if (nt > 1)
      slot += nt;
  }

  auto* h = new ocean_hulls();
  h->fft = fft;
  h->bodies = bodies;
  h->instance_points = instance_points;
  h->items = (int)tiles.size();
  h->n_folds = (int)folds.size();
  hipError_t e = hipMalloc(&h->points, (size_t)n_points * 2 * sizeof(float4));
  if (e == hipSuccess)
    e = hipMalloc(&h->tiles, tiles.size() * sizeof(HullTile));
  if (e == hipSuccess)
    e = hipMalloc(&h->body_table, table.size() * sizeof(HullBody));
  if (e == hipSuccess && !folds.empty())
    e = hipMalloc(&h->folds, folds.size() * sizeof(HullFold));
  if (e == hipSuccess && slot > 0)
    e = hipMalloc(&h->partial, (size_t)slot * 2 * sizeof(float4));
  // synchronous copies from the caller's and these pageable buffers: complete on return
  if (e == hipSuccess)
    e = hipMemcpy(h->points, points, (size_t)n_points * 2 * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->tiles, tiles.data(), tiles.size() * sizeof(HullTile), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->body_table, table.data(), table.size() * sizeof(HullBody), hipMemcpyHostToDevice);
  if (e == hipSuccess && !folds.empty())
    e = hipMemcpy(h->folds, folds.data(), folds.size() * sizeof(HullFold), hipMemcpyHostToDevice);
  if (e != hipSuccess)
  {
    h->fft = nullptr;
    ocean_hulls_destroy(h);
    return alloc_fail(e, "ocean_hulls_create");
  }
  *out = h;
  return OCEAN_OK;
}

int ocean_hulls_bodies(const ocean_hulls* h) { return h ? h->bodies : 0; }

int64_t ocean_hulls_instance_points(const ocean_hulls* h) { return h ? h->instance_points : 0; }

int ocean_hulls_loads(ocean_hulls* h, ocean_generator* const* gens, const int* cascades, int count, const float* poses,
                      float rho_g, int iterations, float tolerance, int water_velocity, float* loads, float* point_out)
{
  if (!h)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_loads: null hull set");
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_hulls_loads"));
  TRY(same_plan(gens[0], h->fft, "hull set", "ocean_hulls_loads"));
  TRY(check_fixed_point(iterations, tolerance, "ocean_hulls_loads"));
  if (!(rho_g >= 0.0f) || !std::isfinite(rho_g))
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_loads: rho_g must be finite and >= 0");
  if (water_velocity != 0 && water_velocity != 1)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_loads: water_velocity must be 0 or 1");
  if (!poses || !loads)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_loads: null poses/loads");
  SurfaceRates r{};
  if (water_velocity)
    TRY(surface_rates(gens, cascades, count, fft, r, "ocean_hulls_loads"));
  const bool atlas = surface_query_use_atlas(p, h->instance_points, iterations);
  TRY(surface_atlas(fft, p, atlas, "ocean_hulls_loads"));
  if (atlas)
    launch_surface_atlas(p, fft->stream, fft->cus);
  HullCall call{};
  call.points = h->points;
  call.tiles = h->tiles;
  call.bodies = h->body_table;
  call.poses = poses;
  call.loads = reinterpret_cast<float4*>(loads);
  call.partial = h->partial;
  call.point_out = reinterpret_cast<float4*>(point_out);
  call.items = h->items;
  call.iterations = iterations;
  call.tolerance = tolerance;
  call.rho_g = rho_g;
  HIP_TRY(launch_hulls_loads(p, r, water_velocity != 0, call, h->folds, h->n_folds, fft->stream, fft->cus),
          "ocean_hulls_loads");
  return OCEAN_OK;
}

// ---- hull dynamics: the bodies stepped from their loads (device/k_hulls_step.h) ----
int ocean_hulls_set_bodies(ocean_hulls* h, const float* props)
{
  if (!h || !props)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_set_bodies: null argument");
  for (int b = 0; b < h->bodies; b++)
  {
    const float* q = props + 8 * (size_t)b;
    const std::string who = "ocean_hulls_set_bodies: body " + std::to_string(b);
    for (int k = 0; k < 8; k++)
      if (!std::isfinite(q[k]))
        return fail(OCEAN_ERR_INVALID, who + " has a non-finite field");
    if (!(q[0] > 0.0f) || !(q[1] > 0.0f) || !(q[2] > 0.0f) || !(q[3] > 0.0f))
      return fail(OCEAN_ERR_INVALID, who + " needs a mass and moments > 0");
    if (q[4] < 0.0f || q[5] < 0.0f)
      return fail(OCEAN_ERR_INVALID, who + " has a negative damping");
    if (q[6] != 0.0f && q[6] != 1.0f)
      return fail(OCEAN_ERR_INVALID, who + " needs kinematic 0 or 1");
  }
  // the one allocation of the dynamics: ocean_hulls_step keeps the sums in registers and needs no buffer of
  // its own for a caller that passes no loads. A later call replaces the properties behind the stream's work.
  const size_t bytes = (size_t)h->bodies * 2 * sizeof(float4);
  hipError_t e = hipSuccess;
  if (!h->props)
    e = hipMalloc(&h->props, bytes);
  else
    e = hipStreamSynchronize(h->fft->stream);
  if (e != hipSuccess)
    return alloc_fail(e, "ocean_hulls_set_bodies");
  HIP_TRY(hipMemcpy(h->props, props, bytes, hipMemcpyHostToDevice), "ocean_hulls_set_bodies");
  return OCEAN_OK;
}

void ocean_default_hull_step_settings(ocean_hull_step_settings* s)
{
  if (s)
    *s = ocean_hull_step_settings{1.0f / 60.0f, 1, {0.0f, -9.8f, 0.0f}, 9810.0f, 8, 0.0f, 0};
}

int ocean_hulls_step(ocean_hulls* h, ocean_generator* const* gens, const int* cascades, int count,
                     const ocean_hull_step_settings* s, float* poses, const float* wrench_ext, float* loads,
                     float* point_out)
{
  if (!h)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: null hull set");
  if (!s || !poses)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: null settings/poses");
  // the settings' own rules first: they need neither the set nor a generator
  if (!(s->dt > 0.0f) || !std::isfinite(s->dt))
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: dt must be finite and > 0");
  if (s->substeps < 1 || s->substeps > 64)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: substeps outside 1..64");
  if (!std::isfinite(s->gravity[0]) || !std::isfinite(s->gravity[1]) || !std::isfinite(s->gravity[2]))
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: gravity must be finite");
  TRY(check_fixed_point(s->iterations, s->tolerance, "ocean_hulls_step"));
  if (!(s->rho_g >= 0.0f) || !std::isfinite(s->rho_g))
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: rho_g must be finite and >= 0");
  if (s->water_velocity != 0 && s->water_velocity != 1)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: water_velocity must be 0 or 1");
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, "ocean_hulls_step"));
  TRY(same_plan(gens[0], h->fft, "hull set", "ocean_hulls_step"));
  if (!h->props)
    return fail(OCEAN_ERR_INVALID, "ocean_hulls_step: the bodies' properties were never set (ocean_hulls_set_bodies)");
  SurfaceRates r{};
  if (s->water_velocity)
    TRY(surface_rates(gens, cascades, count, fft, r, "ocean_hulls_step"));
  const bool atlas = surface_query_use_atlas(p, h->instance_points, s->iterations);
  TRY(surface_atlas(fft, p, atlas, "ocean_hulls_step"));
  if (atlas)
    launch_surface_atlas(p, fft->stream, fft->cus);
  HullCall call{};
  call.points = h->points;
  call.tiles = h->tiles;
  call.bodies = h->body_table;
  call.poses = poses;
  call.loads = reinterpret_cast<float4*>(loads);
  call.partial = h->partial;
  call.point_out = reinterpret_cast<float4*>(point_out);
  call.items = h->items;
  call.iterations = s->iterations;
  call.tolerance = s->tolerance;
  call.rho_g = s->rho_g;
  HullStep st{};
  st.poses = poses;
  st.props = h->props;
  st.ext = reinterpret_cast<const float4*>(wrench_ext);
  st.h = s->dt / (float)s->substeps;
  st.gx = s->gravity[0], st.gy = s->gravity[1], st.gz = s->gravity[2];
  HIP_TRY(launch_hulls_step(p, r, s->water_velocity != 0, call, st, s->substeps, h->folds, h->n_folds, fft->stream,
                            fft->cus),
          "ocean_hulls_step");
  return OCEAN_OK;
}

// ---- mooring lines: cable chains stepped on the device, wrenches for hulls (device/k_moorings.h) ----
struct ocean_moorings
{
  ocean_fft* fft = nullptr;
  int lines = 0, bodies = 0;
  int attached = 0;  // lines with a body
  int64_t total_nodes = 0;
  int items = 0;
  bool placed = false;  // the nodes were reset, or handed to the caller to write
  HullTile* tiles = nullptr;
  HullBody* table = nullptr;
  MooringLine* consts = nullptr;
  int* start = nullptr;  // [bodies + 1]
  int* order = nullptr;  // [attached]
  float4* nodes = nullptr;
  float4* fm = nullptr;
};

int ocean_moorings_destroy(ocean_moorings* m)
{
  if (!m)
    return OCEAN_OK;
  if (m->fft)
    (void)hipStreamSynchronize(m->fft->stream);
  for (void* p : {(void*)m->tiles, (void*)m->table, (void*)m->consts, (void*)m->start, (void*)m->order,
                  (void*)m->nodes, (void*)m->fm})
    if (p)
      (void)hipFree(p);
  delete m;
  return OCEAN_OK;
}

int ocean_moorings_create(ocean_moorings** out, ocean_fft* fft, const float* lines, const int32_t* attach, int n_lines,
                          int bodies)
{
  if (!out || !fft || !lines || !attach)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_create: null argument");
  *out = nullptr;
  if (n_lines < 1 || n_lines > 1048576)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_create: n_lines outside 1..1048576");
  if (bodies < 0 || bodies > 1048576)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_create: bodies outside 0..1048576");
  for (int i = 0; i < n_lines; i++)
  {
    const float* l = lines + 16 * (size_t)i;
    const std::string who = "ocean_moorings_create: line " + std::to_string(i);
    if (attach[2 * i] < -1 || attach[2 * i] >= bodies)
      return fail(OCEAN_ERR_INVALID, who + " has a body outside -1.." + std::to_string(bodies - 1));
    if (attach[2 * i + 1] < 2 || attach[2 * i + 1] > kMooringMaxNodes)
      return fail(OCEAN_ERR_INVALID, who + " has a node count outside 2..64");
    for (int k = 0; k < 16; k++)
      if (!std::isfinite(l[k]))
        return fail(OCEAN_ERR_INVALID, who + " has a non-finite field");
    if (!(l[6] > 0.0f) || !(l[7] > 0.0f) || !(l[9] > 0.0f))
      return fail(OCEAN_ERR_INVALID, who + " needs length, EA and mass_per_m > 0");
    if (l[8] < 0.0f || l[10] < 0.0f || l[11] < 0.0f || l[12] < 0.0f)
      return fail(OCEAN_ERR_INVALID, who + " needs CA, volume_per_m and drag coefficients >= 0");
    if (l[13] != 0.0f || l[14] != 0.0f || l[15] != 0.0f)
      return fail(OCEAN_ERR_INVALID, who + " needs slots 13..15 zero");
  }

  // the lines' constants and node rows, the work items in the order of the lines (ocean_hulls_create's
  // packing), and the CSR of each body's lines in ascending line index
  std::vector<MooringLine> consts((size_t)n_lines);
  std::vector<HullBody> table((size_t)n_lines);
  std::vector<HullTile> tiles;
  std::vector<int> start((size_t)bodies + 1, 0), order;
  int64_t rows = 0;
  for (int i = 0; i < n_lines; i++)
  {
    const float* l = lines + 16 * (size_t)i;
    const int nodes = attach[2 * i + 1];
    const float l0 = l[6] / (float)(nodes - 1);
    MooringLine c{};
    c.a = make_float4(l[0], l[1], l[2], l0);
    c.f = make_float4(l[3], l[4], l[5], l[7]);
    c.c = make_float4(l[8], l[9] * l0, l[10] * l0, l[11] * l0);
    c.dq = l[12] * l0;
    c.body = attach[2 * i];
    c.nodes = nodes;
    consts[i] = c;
    table[i] = HullBody{rows, (int)rows, nodes};
    rows += nodes;
    if (c.body >= 0)
      start[(size_t)c.body + 1]++;
  }
  for (int b = 0; b < bodies; b++)
    start[(size_t)b + 1] += start[b];
  order.resize((size_t)start[bodies]);
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n_lines; i++)
      if (consts[i].body >= 0)
        order[(size_t)fill[consts[i].body]++] = i;
  }
  for (int i = 0; i < n_lines; i++)
  {
    const int run = packed_run(i, n_lines, attach);
    HullTile t{};
    t.body = i;
    t.slot = -1;
    if (run > 1)
    {
      t.count = run;
      t.seg = lane_segment(attach[2 * i + 1]);
      i += run - 1;
    }
    else
    {
      t.offset = table[i].offset;
      t.first = table[i].first;
      t.count = table[i].count;
    }
    tiles.push_back(t);
  }

  auto* m = new ocean_moorings();
  m->fft = fft;
  m->lines = n_lines;
  m->bodies = bodies;
  m->attached = (int)order.size();
  m->total_nodes = rows;
  m->items = (int)tiles.size();
  hipError_t e = hipMalloc(&m->tiles, tiles.size() * sizeof(HullTile));
  if (e == hipSuccess)
    e = hipMalloc(&m->table, table.size() * sizeof(HullBody));
  if (e == hipSuccess)
    e = hipMalloc(&m->consts, consts.size() * sizeof(MooringLine));
  if (e == hipSuccess)
    e = hipMalloc(&m->start, start.size() * sizeof(int));
  if (e == hipSuccess && !order.empty())
    e = hipMalloc(&m->order, order.size() * sizeof(int));
  if (e == hipSuccess)
    e = hipMalloc(&m->nodes, (size_t)rows * 2 * sizeof(float4));
  if (e == hipSuccess)
    e = hipMalloc(&m->fm, (size_t)n_lines * sizeof(float4));
  // synchronous copies from these pageable buffers: complete on return
  if (e == hipSuccess)
    e = hipMemcpy(m->tiles, tiles.data(), tiles.size() * sizeof(HullTile), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(m->table, table.data(), table.size() * sizeof(HullBody), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(m->consts, consts.data(), consts.size() * sizeof(MooringLine), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(m->start, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess && !order.empty())
    e = hipMemcpy(m->order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess)
  {
    m->fft = nullptr;
    ocean_moorings_destroy(m);
    return alloc_fail(e, "ocean_moorings_create");
  }
  *out = m;
  return OCEAN_OK;
}

int ocean_moorings_lines(const ocean_moorings* m) { return m ? m->lines : 0; }

int64_t ocean_moorings_total_nodes(const ocean_moorings* m) { return m ? m->total_nodes : 0; }

float* ocean_moorings_nodes(ocean_moorings* m)
{
  if (!m)
    return nullptr;
  m->placed = true;  // the caller may write them
  return reinterpret_cast<float*>(m->nodes);
}

// What both launches of a set share
static MooringCall mooring_call(const ocean_moorings* m, const float* poses)
{
  MooringCall c{};
  c.tiles = m->tiles;
  c.table = m->table;
  c.lines = m->consts;
  c.poses = poses;
  c.nodes = m->nodes;
  c.fm = m->fm;
  c.items = m->items;
  return c;
}

int ocean_moorings_reset(ocean_moorings* m, const float* poses)
{
  if (!m)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_reset: null mooring set");
  if (!poses && m->attached > 0)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_reset: null poses, and a line has a body");
  HIP_TRY(launch_moorings_reset(mooring_call(m, poses), m->fft->stream, m->fft->cus), "ocean_moorings_reset");
  m->placed = true;
  return OCEAN_OK;
}

void ocean_default_mooring_settings(ocean_mooring_settings* s)
{
  if (s)
    *s = ocean_mooring_settings{1.0f / 60.0f, 8, {0.0f, -9.8f, 0.0f}, 9810.0f, 4, 0.0f, 0, -100.0f, 1e5f, 1e3f};
}

int ocean_moorings_step(ocean_moorings* m, ocean_generator* const* gens, const int* cascades, int count,
                        const ocean_mooring_settings* s, const float* poses, float* wrench_ext, float* line_out)
{
  const char* who = "ocean_moorings_step";
  if (!m)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: null mooring set");
  if (!s)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: null settings");
  // the settings' own rules first: they need neither the set nor a generator
  if (!(s->dt > 0.0f) || !std::isfinite(s->dt))
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: dt must be finite and > 0");
  if (s->substeps < 1 || s->substeps > 256)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: substeps outside 1..256");
  if (!std::isfinite(s->gravity[0]) || !std::isfinite(s->gravity[1]) || !std::isfinite(s->gravity[2]))
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: gravity must be finite");
  if (!(s->rho_g >= 0.0f) || !std::isfinite(s->rho_g))
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: rho_g must be finite and >= 0");
  TRY(check_fixed_point(s->iterations, s->tolerance, who));
  if (s->water != 0 && s->water != 1)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: water must be 0 or 1");
  if (!std::isfinite(s->bed_y))
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: bed_y must be finite");
  if (!(s->bed_k >= 0.0f) || !std::isfinite(s->bed_k) || !(s->bed_c >= 0.0f) || !std::isfinite(s->bed_c))
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: bed_k and bed_c must be finite and >= 0");
  if (!poses && m->attached > 0)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: null poses, and a line has a body");
  if (!wrench_ext && m->bodies > 0)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: null wrench_ext, and the set has bodies");
  if (!m->placed)
    return fail(OCEAN_ERR_INVALID, "ocean_moorings_step: the nodes were never reset nor written "
                                   "(ocean_moorings_reset, ocean_moorings_nodes)");
  SurfaceParams p{};
  WaterLayers w{};
  if (s->water)
  {
    ocean_fft* fft;
    TRY(surface_params(gens, cascades, count, p, fft, who));
    TRY(same_plan(gens[0], m->fft, "mooring set", who));
    TRY(water_layers(gens, cascades, count, fft, w, who));
  }
  MooringCall c = mooring_call(m, poses);
  c.line_out = reinterpret_cast<float4*>(line_out);
  c.substeps = s->substeps;
  c.fsubsteps = (float)s->substeps;
  c.h = s->dt / (float)s->substeps;
  c.gx = s->gravity[0], c.gy = s->gravity[1], c.gz = s->gravity[2];
  c.rho_g = s->rho_g;
  c.bed_y = s->bed_y, c.bed_k = s->bed_k, c.bed_c = s->bed_c;
  c.iterations = s->iterations;
  c.tolerance = s->tolerance;
  MooringWrench q{};
  q.start = m->start;
  q.order = m->order;
  q.lines = m->consts;
  q.fm = m->fm;
  q.poses = poses;
  q.out = reinterpret_cast<float4*>(wrench_ext);
  q.bodies = m->bodies;
  HIP_TRY(launch_moorings_step(p, w, s->water != 0, c, q, m->fft->stream, m->fft->cus), who);
  return OCEAN_OK;
}

// ---- wake windows: hull loads drive local surface waves (device/k_wake.h) ----
struct ocean_wake
{
  ocean_fft* fft = nullptr;  // null: a host-only window (ocean_debug_wake_create_host), no device storage
  int m = 0;
  float dx = 0, origin_x = 0, origin_z = 0, sigma = 0;
  int64_t off_i = 0, off_j = 0;
  float taps[49] = {};
  double sum_abs = 0;  // of all 169 float taps
  float hs = 0;        // the last call's substep; 0: no step since the creation or the last reset
  void* storage = nullptr;  // acc | map | map
  long long* acc = nullptr;
  float* h = nullptr;
  float* h_prev = nullptr;
};

namespace
{

// I0(z) and I1(z) by their power series: every term is positive, z <= 30 here (x / 2, x = 72 / (4 * 0.3))
void bessel_i01(double z, double& i0, double& i1)
{
  const double q = 0.25 * z * z;
  double t0 = 1.0, t1 = 1.0;
  i0 = 1.0, i1 = 1.0;
  for (int k = 1; k < 200; k++)
  {
    t0 *= q / ((double)k * k);
    t1 *= q / ((double)k * (k + 1));
    i0 += t0;
    i1 += t1;
  }
  i1 *= 0.5 * z;
}

// T[a][b] = (1 / 2 pi) int_0^inf q^2 exp(-sigma q^2) J0(q r) dq, r^2 = a^2 + b^2, by its closed form
//   sqrt(pi) / (4 sigma^1.5) exp(-x / 2) ((1 - x) I0(x / 2) + x I1(x / 2)) / (2 pi),   x = r^2 / (4 sigma),
// in double, rounded once to float
void wake_taps(double sigma, float out[49])
{
  const double pi = 3.14159265358979323846;
  const double lead = std::sqrt(pi) / (4.0 * sigma * std::sqrt(sigma)) / (2.0 * pi);
  for (int a = 0; a <= kWakeRadius; a++)
    for (int b = 0; b <= kWakeRadius; b++)
    {
      const double x = (double)(a * a + b * b) / (4.0 * sigma);
      double i0, i1;
      bessel_i01(0.5 * x, i0, i1);
      out[a * 7 + b] = (float)(lead * std::exp(-0.5 * x) * ((1.0 - x) * i0 + x * i1));
    }
}

// The smallest value of the 13 x 13 operator's symbol, the double cosine sum of the float taps, on 257^2
// points of [-pi, pi]^2. A value <= 0 is a mode that does not oscillate but grows.
double wake_symbol_min(const float taps[49])
{
  const double pi = 3.14159265358979323846;
  const int grid = 257;
  std::vector<double> c((size_t)grid * 7);
  for (int p = 0; p < grid; p++)
    for (int a = 0; a < 7; a++)
      c[(size_t)p * 7 + a] = (a ? 2.0 : 1.0) * std::cos((double)a * (-pi + 2.0 * pi * p / (grid - 1)));
  double least = INFINITY;
  for (int p = 0; p < grid; p++)
  {
    double row[7];  // sum over a of c[p][a] T[a][b]
    for (int b = 0; b < 7; b++)
    {
      row[b] = 0.0;
      for (int a = 0; a < 7; a++)
        row[b] += c[(size_t)p * 7 + a] * (double)taps[a * 7 + b];
    }
    for (int q = 0; q < grid; q++)
    {
      double v = 0.0;
      for (int b = 0; b < 7; b++)
        v += row[b] * c[(size_t)q * 7 + b];
      least = std::min(least, v);
    }
  }
  return least;
}

// Everything of a window that needs no device: the argument rules, the taps, the symbol's sign
int wake_host(ocean_wake** out, int size, float dx, float origin_x, float origin_z, float smoothing, const std::string& who)
{
  if (!out)
    return fail(OCEAN_ERR_INVALID, who + ": null output");
  *out = nullptr;
  if (size < 32 || size > 4096 || size % 16 != 0)
    return fail(OCEAN_ERR_INVALID, who + ": size must be a multiple of 16 in 32..4096");
  if (!std::isfinite(dx) || !(dx > 0.0f))
    return fail(OCEAN_ERR_INVALID, who + ": dx must be finite and > 0");
  if (!std::isfinite(origin_x) || !std::isfinite(origin_z))
    return fail(OCEAN_ERR_INVALID, who + ": the origin must be finite");
  if (smoothing == 0.0f)
    smoothing = 0.5f;
  if (!(smoothing >= 0.3f) || !(smoothing <= 0.55f))
    return fail(OCEAN_ERR_INVALID, who + ": smoothing outside 0.3..0.55 (0: the default 0.5)");
  auto* w = new ocean_wake();
  w->m = size;
  w->dx = dx;
  w->origin_x = origin_x;
  w->origin_z = origin_z;
  w->sigma = smoothing;
  wake_taps((double)smoothing, w->taps);
  if (!(wake_symbol_min(w->taps) > 0.0))
  {
    delete w;
    return fail(OCEAN_ERR_INVALID, who + ": smoothing gives an operator whose symbol is not positive");
  }
  for (int a = -kWakeRadius; a <= kWakeRadius; a++)
    for (int b = -kWakeRadius; b <= kWakeRadius; b++)
      w->sum_abs += std::fabs((double)w->taps[std::abs(a) * 7 + std::abs(b)]);
  *out = w;
  return OCEAN_OK;
}

int wake_device(const ocean_wake* w, const std::string& who)
{
  if (!w->fft)
    return fail(OCEAN_ERR_INVALID, who + ": the window has no device storage (ocean_debug_wake_create_host)");
  return OCEAN_OK;
}

// What every launch of a window shares
WakeCall wake_call(const ocean_wake* w)
{
#pragma clang fp contract(off)
  WakeCall c{};
  c.h = w->h;
  c.h_prev = w->h_prev;
  c.acc = w->acc;
  c.m = w->m;
  c.dx = w->dx;
  c.ox = w->origin_x + (float)w->off_i * w->dx;
  c.oz = w->origin_z + (float)w->off_j * w->dx;
  c.hs = w->hs;
  for (int a = 0; a <= kWakeRadius; a++)
    for (int b = 0; b <= a; b++)
      c.taps[a * (a + 1) / 2 + b] = w->taps[a * 7 + b];
  return c;
}

}  // namespace

int ocean_wake_destroy(ocean_wake* w)
{
  if (!w)
    return OCEAN_OK;
  if (w->fft)
    (void)hipStreamSynchronize(w->fft->stream);
  if (w->storage)
    (void)hipFree(w->storage);
  delete w;
  return OCEAN_OK;
}

int ocean_debug_wake_create_host(ocean_wake** out, int size, float dx, float origin_x, float origin_z, float smoothing)
{
  return wake_host(out, size, dx, origin_x, origin_z, smoothing, "ocean_debug_wake_create_host");
}

int ocean_wake_create(ocean_wake** out, ocean_fft* fft, int size, float dx, float origin_x, float origin_z,
                      float smoothing)
{
  const std::string who = "ocean_wake_create";
  if (out)
    *out = nullptr;
  if (!out || !fft)
    return fail(OCEAN_ERR_INVALID, who + ": null argument");
  ocean_wake* w = nullptr;
  TRY(wake_host(&w, size, dx, origin_x, origin_z, smoothing, who));
  const size_t mm = (size_t)size * size;
  hipError_t e = hipMalloc(&w->storage, mm * 16);
  if (e == hipSuccess)
    e = hipMemsetAsync(w->storage, 0, mm * 16, fft->stream);
  if (e != hipSuccess)
  {
    if (w->storage)
    {
      (void)hipStreamSynchronize(fft->stream);
      (void)hipFree(w->storage);
    }
    delete w;
    return alloc_fail(e, who);
  }
  w->fft = fft;
  w->acc = static_cast<long long*>(w->storage);
  w->h = reinterpret_cast<float*>(w->acc + mm);
  w->h_prev = w->h + mm;
  *out = w;
  return OCEAN_OK;
}

int ocean_wake_size(const ocean_wake* w) { return w ? w->m : 0; }

int ocean_wake_kernel(const ocean_wake* w, float out[49])
{
  if (!w || !out)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_kernel: null argument");
  std::memcpy(out, w->taps, sizeof(w->taps));
  return OCEAN_OK;
}

double ocean_wake_max_substep(const ocean_wake* w, float gravity)
{
  if (!w || !(gravity > 0.0f))
    return 0.0;
  return 2.0 * std::sqrt((double)w->dx / ((double)gravity * w->sum_abs));
}

int ocean_wake_origin(const ocean_wake* w, float out[2])
{
  if (!w || !out)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_origin: null argument");
  const WakeCall c = wake_call(w);
  out[0] = c.ox;
  out[1] = c.oz;
  return OCEAN_OK;
}

float* ocean_wake_height(ocean_wake* w) { return w ? w->h : nullptr; }

int ocean_wake_reset(ocean_wake* w)
{
  const char* who = "ocean_wake_reset";
  if (!w)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_reset: null wake");
  TRY(wake_device(w, who));
  float* first = w->h < w->h_prev ? w->h : w->h_prev;  // the two maps are neighbours
  HIP_TRY(hipMemsetAsync(first, 0, (size_t)w->m * w->m * 2 * sizeof(float), w->fft->stream), who);
  w->hs = 0.0f;
  return OCEAN_OK;
}

int ocean_wake_shift(ocean_wake* w, int di, int dj)
{
  const char* who = "ocean_wake_shift";
  if (!w)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_shift: null wake");
  if (di < -1048576 || di > 1048576 || dj < -1048576 || dj > 1048576)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_shift: di or dj outside -1048576..1048576");
  TRY(wake_device(w, who));
  if (di != 0 || dj != 0)
    HIP_TRY(launch_wake_shift(wake_call(w), di, dj, w->fft->stream, w->fft->cus), who);
  w->off_i += di;
  w->off_j += dj;
  return OCEAN_OK;
}

void ocean_default_wake_settings(ocean_wake_settings* s)
{
  if (s)
    *s = ocean_wake_settings{1.0f / 60.0f, 4, 9.8f, 9810.0f, 0.05f, 8.0f, 16};
}

int ocean_wake_step(ocean_wake* w, const ocean_wake_settings* s, const float* records, const int64_t* count_device,
                    int64_t max_records)
{
#pragma clang fp contract(off)
  const char* who = "ocean_wake_step";
  if (!w)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: null wake");
  if (!s)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: null settings");
  if (!(s->dt > 0.0f) || !std::isfinite(s->dt))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: dt must be finite and > 0");
  if (s->substeps < 1 || s->substeps > 64)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: substeps outside 1..64");
  if (!(s->gravity > 0.0f) || !std::isfinite(s->gravity))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: gravity must be finite and > 0");
  if (!(s->rho_g > 0.0f) || !std::isfinite(s->rho_g))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: rho_g must be finite and > 0");
  if (!(s->damp >= 0.0f) || !std::isfinite(s->damp))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: damp must be finite and >= 0");
  if (!(s->edge_damp >= 0.0f) || !std::isfinite(s->edge_damp))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: edge_damp must be finite and >= 0");
  if (s->border < 0 || s->border > w->m / 2)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: border outside 0..size/2");
  if (max_records < 0 || max_records > ((int64_t)1 << 28))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: max_records outside 0..2^28");
  if (!records && max_records > 0)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: null records with max_records > 0");
  const float hs = s->dt / (float)s->substeps;
  if (!((double)hs < ocean_wake_max_substep(w, s->gravity)))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_step: dt / substeps is at or above ocean_wake_max_substep");
  TRY(wake_device(w, who));
  WakeCall c = wake_call(w);
  c.border = s->border;
  c.c = ((hs * hs) * s->gravity) / w->dx;
  c.hb = 0.5f * hs;
  c.inv = 1.0f / ((s->rho_g * w->dx) * w->dx);
  c.damp = s->damp;
  c.edge_damp = s->edge_damp;
  c.records = records;
  c.count_device = count_device;
  c.max_records = max_records;
  const hipError_t e = launch_wake_step(c, s->substeps, w->fft->stream, w->fft->cus);
  w->h = c.h;  // as far as the substeps were issued
  w->h_prev = c.h_prev;
  if (e != hipSuccess)
  {
    // a launch failed part way: the maps hold an unfinished step, and the accumulators are zeroed here so that
    // "all zero between calls" holds for the next call, whatever the splat had added
    (void)hipMemsetAsync(w->acc, 0, (size_t)w->m * w->m * sizeof(long long), w->fft->stream);
    return hip_fail(e, who);
  }
  w->hs = hs;
  return OCEAN_OK;
}

int ocean_wake_sample(ocean_wake* w, const float* xz, int64_t n, float* out)
{
  const char* who = "ocean_wake_sample";
  if (!w)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_sample: null wake");
  if (n < 0 || n > 2147483647LL)
    return fail(OCEAN_ERR_INVALID, "ocean_wake_sample: n outside 0..2^31-1");
  if (n > 0 && (!xz || !out))
    return fail(OCEAN_ERR_INVALID, "ocean_wake_sample: null xz or out with n > 0");
  TRY(wake_device(w, who));
  HIP_TRY(launch_wake_sample(wake_call(w), xz, n, out, w->fft->stream, w->fft->cus), who);
  return OCEAN_OK;
}

// ---- spray emitters: ordered compaction of breaking texels into records ----
void ocean_default_spray_settings(ocean_spray_settings* s)
{
  if (s)
    *s = ocean_spray_settings{0.9f, 8.0f, 0u};
}

struct ocean_spray
{
  ocean_fft* fft = nullptr;
  void* scratch = nullptr;  // spray_scratch_bytes(fft->n), allocated by the first emit
};

int ocean_spray_create(ocean_spray** out, ocean_fft* fft)
{
  if (!out || !fft)
    return fail(OCEAN_ERR_INVALID, "ocean_spray_create: null argument");
  auto* s = new ocean_spray();
  s->fft = fft;
  *out = s;
  return OCEAN_OK;
}

int ocean_spray_destroy(ocean_spray* s)
{
  if (!s)
    return OCEAN_OK;
  if (s->scratch)
  {
    (void)hipStreamSynchronize(s->fft->stream);
    (void)hipFree(s->scratch);
  }
  delete s;
  return OCEAN_OK;
}

int ocean_spray_emit(ocean_spray* spray, ocean_generator* const* gens, const int* cascades, int count,
                     const ocean_spray_settings* settings, const int32_t* tiles, float dt, uint32_t step, int velocity,
                     int64_t capacity, float* out)
{
  const std::string who = "ocean_spray_emit";
  // the rules that need no generator first
  if (!spray)
    return fail(OCEAN_ERR_INVALID, who + ": null emitter");
  if (!gens || !cascades || count < 1 || count > kMaxSurfaceCascades)
    return fail(OCEAN_ERR_INVALID, who + ": need 1..16 (generator, cascade) pairs");
  if (!settings)
    return fail(OCEAN_ERR_INVALID, who + ": null settings");
  if (capacity < 0 || (capacity > 0 && !out))
    return fail(OCEAN_ERR_INVALID, who + ": negative capacity, or null output with capacity > 0");
  TRY(check_dt(dt, who));
  for (int i = 0; i < count; i++)
  {
    if (!std::isfinite(settings[i].threshold))
      return fail(OCEAN_ERR_INVALID, who + ": pair " + std::to_string(i) + " has a non-finite threshold");
    if (!(settings[i].rate >= 0.0f) || !std::isfinite(settings[i].rate))
      return fail(OCEAN_ERR_INVALID, who + ": pair " + std::to_string(i) + " needs a rate finite and >= 0");
  }
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, who.c_str()));
  TRY(same_plan(gens[0], spray->fft, "emitter", who));
  TRY(frames_calculated(gens, count, who));
  SurfaceRates r{};
  if (velocity)
    TRY(surface_rates(gens, cascades, count, fft, r, who.c_str()));
  TRY(alloc_once(spray->scratch, spray_scratch_bytes(fft->n), who));
  SprayCall s{};
  spray_scratch(spray->scratch, fft->n, s);
  s.out = out;
  s.capacity = capacity;
  s.n = fft->n;
  s.logn = fft->logn;
  s.nn = fft->n * fft->n;
  s.tiles = foam_tiles(fft->n);
  s.dt = dt;
  s.step = step;
  SprayTiles t{};
  for (int i = 0; i < count; i++)
  {
    if (tiles)
    {
      t.t[i][0] = tiles[2 * i];
      t.t[i][1] = tiles[2 * i + 1];
    }
    if (settings[i].rate != 0.0f)  // a pair that never emits has no items
      s.c[s.pairs++] = SprayPair{p.c[i].jac, settings[i].threshold, settings[i].rate, settings[i].seed, i};
  }
  HIP_TRY(launch_spray_emit(s, p, r, t, velocity != 0, fft->stream, fft->cus), who.c_str());
  return OCEAN_OK;
}

// An emitter that has emitted, else null with a message
static ocean_spray* spray_emitted(ocean_spray* s, const char* who)
{
  if (!s)
    return fail_null(std::string(who) + ": null emitter");
  if (!s->scratch)
    return fail_null(std::string(who) + ": the emitter has no counts yet (call ocean_spray_emit)");
  return s;
}

const int64_t* ocean_spray_counts_device(ocean_spray* s)
{
  return spray_emitted(s, "ocean_spray_counts_device") ? static_cast<const int64_t*>(s->scratch) : nullptr;
}

int ocean_spray_counts(ocean_spray* s, int64_t out[18])
{
  if (!spray_emitted(s, "ocean_spray_counts"))
    return OCEAN_ERR_INVALID;
  if (!out)
    return fail(OCEAN_ERR_INVALID, "ocean_spray_counts: null output");
  return read_back(out, s->scratch, 18 * sizeof(int64_t), s->fft, "ocean_spray_counts");
}

// ---- spray particles: a persistent pool, stepped, landed on the water, compacted in order ----
void ocean_default_particle_settings(ocean_particle_settings* s)
{
  if (s)
    *s = ocean_particle_settings{9.8f, 0.5f, {0.0f, 0.0f, 0.0f}, 4.0f, 1.0f, 10.0f, 4, 1e-3f};
}

struct ocean_particles
{
  ocean_fft* fft = nullptr;
  int64_t capacity = 0;
  float* list[2] = {nullptr, nullptr};  // capacity x 8 floats each; list[current] is the pool's list
  int current = 0;
  void* scratch = nullptr;  // particle_scratch_bytes(capacity): the count table first
};

int ocean_particles_destroy(ocean_particles* p)
{
  if (!p)
    return OCEAN_OK;
  if (p->scratch)  // a pool that launched anything has all three buffers
    (void)hipStreamSynchronize(p->fft->stream);
  (void)hipFree(p->list[0]);
  (void)hipFree(p->list[1]);
  (void)hipFree(p->scratch);
  delete p;
  return OCEAN_OK;
}

int ocean_particles_create(ocean_particles** out, ocean_fft* fft, int64_t capacity)
{
  const std::string who = "ocean_particles_create";
  if (!out || !fft)
    return fail(OCEAN_ERR_INVALID, who + ": null argument");
  if (capacity < 1 || capacity > ((int64_t)1 << 28))
    return fail(OCEAN_ERR_INVALID, who + ": capacity outside 1..2^28");
  auto* p = new ocean_particles();
  p->fft = fft;
  p->capacity = capacity;
  const size_t bytes = (size_t)capacity * 8 * sizeof(float);
  hipError_t e = alloc_if_null(p->list[0], bytes);
  e = alloc_if_null(p->list[1], bytes, e);
  e = alloc_if_null(p->scratch, particle_scratch_bytes(capacity), e);
  if (e == hipSuccess)
    e = launch_particles_reset(static_cast<int64_t*>(p->scratch), 0, fft->stream);
  if (e != hipSuccess)
  {
    ocean_particles_destroy(p);
    return alloc_fail(e, who);
  }
  *out = p;
  return OCEAN_OK;
}

int ocean_particles_step(ocean_particles* pool, ocean_generator* const* gens, const int* cascades, int count,
                         const ocean_particle_settings* settings, float dt, const float* emit_records,
                         const int64_t* emit_counts_device, int64_t landed_capacity, float* landed_out)
{
  const std::string who = "ocean_particles_step";
  // the rules that need neither the pool's fields nor a generator first
  if (!pool)
    return fail(OCEAN_ERR_INVALID, who + ": null pool");
  if (!gens || !cascades || count < 1 || count > kMaxSurfaceCascades)
    return fail(OCEAN_ERR_INVALID, who + ": need 1..16 (generator, cascade) pairs");
  if (!settings)
    return fail(OCEAN_ERR_INVALID, who + ": null settings");
  TRY(check_dt(dt, who));
  const ocean_particle_settings& s = *settings;
  if (!std::isfinite(s.gravity))
    return fail(OCEAN_ERR_INVALID, who + ": non-finite gravity");
  if (!(s.drag >= 0.0f) || !std::isfinite(s.drag))
    return fail(OCEAN_ERR_INVALID, who + ": drag must be finite and >= 0");
  if (!std::isfinite(s.wind[0]) || !std::isfinite(s.wind[1]) || !std::isfinite(s.wind[2]))
    return fail(OCEAN_ERR_INVALID, who + ": non-finite wind");
  if (!(s.lifetime > 0.0f))
    return fail(OCEAN_ERR_INVALID, who + ": lifetime must be > 0 (+inf: never expires)");
  if (!std::isfinite(s.gain))
    return fail(OCEAN_ERR_INVALID, who + ": non-finite gain");
  if (!std::isfinite(s.lift))
    return fail(OCEAN_ERR_INVALID, who + ": non-finite lift");
  TRY(check_fixed_point(s.iterations, s.tolerance, who));
  if (landed_capacity < 0 || (landed_capacity > 0 && !landed_out))
    return fail(OCEAN_ERR_INVALID, who + ": negative landed_capacity, or null landed_out with landed_capacity > 0");
  if (emit_records && !emit_counts_device)
    return fail(OCEAN_ERR_INVALID, who + ": emit_records without emit_counts_device");
  SurfaceParams p;
  ocean_fft* fft;
  TRY(surface_params(gens, cascades, count, p, fft, who.c_str()));
  TRY(same_plan(gens[0], pool->fft, "pool", who));
  TRY(frames_calculated(gens, count, who));
  ParticleCall c{};
  particle_scratch(pool->scratch, pool->capacity, c);
  c.cur = pool->list[pool->current];
  c.next = pool->list[pool->current ^ 1];
  c.emit = emit_records;
  c.emit_counts = emit_records ? emit_counts_device : nullptr;
  c.landed_out = landed_out;
  c.landed_capacity = landed_capacity;
  c.capacity = pool->capacity;
  c.dt = dt;
  c.gravity = s.gravity;
  c.drag = s.drag;
  c.wind[0] = s.wind[0];
  c.wind[1] = s.wind[1];
  c.wind[2] = s.wind[2];
  c.lifetime = s.lifetime;
  c.gain = s.gain;
  c.lift = s.lift;
  c.iterations = s.iterations;
  c.tolerance = s.tolerance;
  HIP_TRY(launch_particles_step(c, p, fft->stream, fft->cus), who.c_str());
  pool->current ^= 1;
  return OCEAN_OK;
}

int ocean_particles_load(ocean_particles* pool, const float* device_records, int64_t count)
{
  const std::string who = "ocean_particles_load";
  if (!pool)
    return fail(OCEAN_ERR_INVALID, who + ": null pool");
  if (count < 0 || (count > 0 && !device_records))
    return fail(OCEAN_ERR_INVALID, who + ": negative count, or null records with count > 0");
  if (count > pool->capacity)
    return fail(OCEAN_ERR_INVALID, who + ": count above the pool's capacity");
  if (count > 0)
    HIP_TRY(hipMemcpyAsync(pool->list[pool->current], device_records, (size_t)count * 8 * sizeof(float),
                           hipMemcpyDeviceToDevice, pool->fft->stream),
            who.c_str());
  HIP_TRY(launch_particles_reset(static_cast<int64_t*>(pool->scratch), count, pool->fft->stream), who.c_str());
  return OCEAN_OK;
}

int ocean_particles_clear(ocean_particles* pool)
{
  if (!pool)
    return fail(OCEAN_ERR_INVALID, "ocean_particles_clear: null pool");
  HIP_TRY(launch_particles_reset(static_cast<int64_t*>(pool->scratch), 0, pool->fft->stream), "ocean_particles_clear");
  return OCEAN_OK;
}

const float* ocean_particles_records(ocean_particles* pool)
{
  if (!pool)
    return fail_null("ocean_particles_records: null pool");
  return pool->list[pool->current];
}

const int64_t* ocean_particles_counts_device(ocean_particles* pool)
{
  if (!pool)
    return fail_null("ocean_particles_counts_device: null pool");
  return static_cast<const int64_t*>(pool->scratch);
}

int ocean_particles_counts(ocean_particles* pool, int64_t out[8])
{
  if (!pool)
    return fail(OCEAN_ERR_INVALID, "ocean_particles_counts: null pool");
  if (!out)
    return fail(OCEAN_ERR_INVALID, "ocean_particles_counts: null output");
  return read_back(out, pool->scratch, 8 * sizeof(int64_t), pool->fft, "ocean_particles_counts");
}

}  // extern "C"
