// ocean_capi.cpp — implementation of the C ABI in include/oceanfft.h.
//
// Host-side orchestration of the reference's FFTCalculator / Generator (src/FFTCalculator.cpp,
// src/Generator.cpp) over the HIP kernels in ocean_kernels.hip and launch_*.hip: the plans and the
// generators. The exchanges that move a slab frame's blocks between ranks are in ocean_capi_exchange.cpp,
// the entry points that consume a generator's maps (the map getters, the surface requests, mips, rates,
// bounds and hull sets) in ocean_capi_surface.cpp. No CPU fallback exists: without a GPU every entry point
// fails with OCEAN_ERR_NO_DEVICE / OCEAN_ERR_HIP.
#include "oceanfft.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ocean_capi_internal.h"
#include "ocean_internal.h"

static_assert(sizeof(ocean_settings) == sizeof(OceanSettings), "settings layout");

namespace
{
int log2_exact(size_t n)
{
  int l = 0;
  while (((size_t)1 << l) < n)
    l++;
  return ((size_t)1 << l) == n ? l : -1;
}

// Twiddle table exp(+2 pi i e / N), two levels (FFTCalculator's pass table analogue,
// src/FFTCalculator.cpp:14-32): [0, TB) = low part, [TB, TB+TA) = high part. The four-step
// EncodeIFFT (N = 16384) appends the N/16-point table at tw2_at, the pre-stage one (N = 8192) the
// 4096-point table at twm_at.
std::vector<float2> twiddle_tables(int logn, size_t& tw2_at, size_t& twm_at)
{
  std::vector<float2> tab;
  const double two_pi = 6.283185307179586476925286766559;
  auto append_table = [&](int lg) {
    const int lb = lg / 2, tb = 1 << lb, ta = 1 << (lg - lb);
    const double len = (double)(1 << lg);
    for (int e2 = 0; e2 < tb; e2++)
    {
      double a = two_pi * e2 / len;
      tab.push_back(make_float2((float)std::cos(a), (float)std::sin(a)));
    }
    for (int e2 = 0; e2 < ta; e2++)
    {
      double a = two_pi * ((double)e2 * tb) / len;
      tab.push_back(make_float2((float)std::cos(a), (float)std::sin(a)));
    }
  };
  append_table(logn);
  tw2_at = tab.size();
  if (fourstep_table(logn))
    append_table(logn - 4);
  twm_at = tab.size();
  if (ifft_pre_supported(logn))
    append_table(12);
  return tab;
}

// Replaces the plan's work buffer by one of `texels` (`images` whole images; 0: the four-step slab).
// Capped (ocean_debug_fft_work_limit) or without room, the plan keeps what it has and the caller falls
// back to the in-place passes.
void grow_work(ocean_fft* fft, size_t texels, int images)
{
  float4* w = nullptr;
  if (texels * sizeof(float4) > fft->work_limit)
    return;
  if (hipMalloc(&w, texels * sizeof(float4)) != hipSuccess)
  {
    (void)hipGetLastError();
    return;
  }
  if (fft->work)
    (void)hipFree(fft->work);
  fft->work = w;
  fft->work_images = images;
  fft->work_texels = texels;
}
}  // namespace

// Four-step EncodeIFFT work slab width at N = 16384 (tools/microbench/ifft4bench,
// profiles/r02_ifft4bench.log: 2048 columns 5.05 ms, whole image 5.39, in place 7.26)
constexpr int kFourStepSlab = 2048;

extern "C" {

const char* ocean_last_error(void) { return g_err.c_str(); }

const char* ocean_version(void) { return "oceanfft 0.1 (gfx950)"; }

void ocean_default_settings(ocean_settings* s)
{
  // src/Generator.h:14-29
  std::memset(s, 0, sizeof(*s));
  s->seed[0] = 12342;
  s->seed[1] = 8934;
  s->U_10 = 40.0f;
  s->theta_0 = 25.0f;
  s->F = 800000.0f;
  s->g = 9.8f;
  s->swell = 0.5f;
  s->h = 100.0f;
  s->displacement = 0.4f;
  s->time = 0.0f;
  s->planeSize = 40.0f;
  s->scale = 1.0f;
  s->spread = 0.2f;
  s->boundWavelength = 0;
  s->wavelengthMin = 0.0f;
  s->wavelengthMax = 0.0f;
}

int ocean_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

int ocean_fft_create(ocean_fft** out, size_t texture_size, void* hip_stream)
{
  if (!out)
    return fail(OCEAN_ERR_INVALID, "ocean_fft_create: out is null");
  *out = nullptr;
  int logn = log2_exact(texture_size);
  if (logn < 4 || logn > 14)
    return fail(OCEAN_ERR_INVALID, "ocean_fft_create: texture_size must be a power of two in [16, 16384], got " +
                                       std::to_string(texture_size));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(OCEAN_ERR_NO_DEVICE, "ocean_fft_create: no HIP device visible");

  auto* f = new ocean_fft();
  f->n = (int)texture_size;
  f->logn = logn;
  f->stream = (hipStream_t)hip_stream;
  hipError_t e = hipGetDevice(&f->device);
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&f->device_cus, hipDeviceAttributeMultiprocessorCount, f->device);
  f->cus = f->device_cus;
  if (e != hipSuccess)
  {
    delete f;
    return hip_fail(e, "ocean_fft_create: device query");
  }

  size_t tw2_at = 0, twm_at = 0;
  const std::vector<float2> tab = twiddle_tables(logn, tw2_at, twm_at);
  e = hipMalloc(&f->twiddles, tab.size() * sizeof(float2));
  if (e == hipSuccess)
    e = hipMemcpy(f->twiddles, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice);
  if (e != hipSuccess)
  {
    if (f->twiddles)
      (void)hipFree(f->twiddles);
    delete f;
    return hip_fail(e, "ocean_fft_create: twiddle table");
  }
  if (fourstep_table(logn))
    f->tw2 = f->twiddles + tw2_at;
  if (ifft_pre_supported(logn))
    f->twm = f->twiddles + twm_at;
  *out = f;
  return OCEAN_OK;
}

int ocean_fft_destroy(ocean_fft* fft)
{
  if (!fft)
    return OCEAN_OK;
  if (fft->twiddles)
    (void)hipFree(fft->twiddles);
  if (fft->work)
    (void)hipFree(fft->work);
  if (fft->surf_atlas)
    (void)hipFree(fft->surf_atlas);
  delete fft;
  return OCEAN_OK;
}

size_t ocean_fft_texture_resolution(const ocean_fft* fft) { return fft ? (size_t)fft->n : 0; }

int ocean_fft_device_cus(const ocean_fft* fft) { return fft ? fft->device_cus : 0; }

int ocean_fft_set_cu_budget(ocean_fft* fft, int cus)
{
  if (!fft)
    return fail(OCEAN_ERR_INVALID, "ocean_fft_set_cu_budget: null plan");
  if (cus < 0 || cus > fft->device_cus)
    return fail(OCEAN_ERR_INVALID, "ocean_fft_set_cu_budget: budget outside [0, device CUs]");
  fft->cus = cus == 0 ? fft->device_cus : cus;
  return OCEAN_OK;
}

int ocean_debug_fft_work_limit(ocean_fft* fft, size_t bytes)
{
  if (!fft)
    return fail(OCEAN_ERR_INVALID, "ocean_debug_fft_work_limit: null plan");
  fft->work_limit = bytes;
  if (fft->work && fft->work_texels * sizeof(float4) > bytes)
  {
    HIP_TRY(hipStreamSynchronize(fft->stream), "hipStreamSynchronize");  // launches may still read it
    (void)hipFree(fft->work);
    fft->work = nullptr;
    fft->work_images = 0;
    fft->work_texels = 0;
  }
  return OCEAN_OK;
}

int ocean_fft_encode_ifft_batch(ocean_fft* fft, float* images, int n_images)
{
  if (!fft || !images || n_images < 1)
    return fail(OCEAN_ERR_INVALID, "ocean_fft_encode_ifft_batch: null plan/image or n_images < 1");
  auto* img = reinterpret_cast<float4*>(images);
  const bool pre = fft->logn == 13 && fft->twm != nullptr;  // 8192: the radix-2 pre-stage column pass
  if (ifft_colfirst_supported(fft->logn) || pre)
  {
    // column-first through a work image of up to 2 GiB (8 images at N = 4096, 2 at 8192)
    const int chunk = std::max(1, (int)(((size_t)2 << 30) / ((size_t)fft->n * fft->n * sizeof(float4))));
    const int want = n_images < chunk ? n_images : chunk;
    if (fft->work_images < want)
      grow_work(fft, (size_t)want * fft->n * fft->n, want);
    if (fft->work)
    {
      for (int first = 0; first < n_images; first += fft->work_images)
      {
        const int count = n_images - first < fft->work_images ? n_images - first : fft->work_images;
        float4* first_img = img + (size_t)first * fft->n * fft->n;
        if (pre)
          HIP_TRY(launch_ifft_pre(fft->logn, count, first_img, fft->work, fft->twiddles, fft->twm, fft->stream, fft->cus),
                  "pre-stage EncodeIFFT");
        else
          HIP_TRY(launch_ifft_colfirst(fft->logn, count, first_img, fft->work, fft->twiddles, fft->stream, fft->cus),
                  "column-first EncodeIFFT");
      }
      return OCEAN_OK;
    }
  }
  if (ifft_fourstep_supported(fft->logn) && fft->logn == 14)
  {
    // rows in place, then the column transform in four steps through a work slab of N x 2048
    // texels (512 MiB): every access a >= 256-B row piece instead of one-column 16-B pieces
    const size_t want = ifft_fourstep_work_texels(fft->logn, kFourStepSlab);
    if (fft->work_texels < want)
      grow_work(fft, want, 0);
    if (fft->work_texels >= want)
    {
      HIP_TRY(launch_ifft_fourstep(fft->logn, n_images, img, fft->work, kFourStepSlab, fft->twiddles, fft->tw2,
                                   fft->stream, fft->cus),
              "four-step EncodeIFFT");
      return OCEAN_OK;
    }
  }
  HIP_TRY(launch_rows_ifft(fft->logn, n_images, img, fft->twiddles, fft->stream, fft->cus), "row pass");
  HIP_TRY(launch_cols(fft->logn, n_images, img, fft->twiddles, fft->stream, fft->cus), "column pass");
  return OCEAN_OK;
}

int ocean_fft_encode_ifft(ocean_fft* fft, float* image) { return ocean_fft_encode_ifft_batch(fft, image, 1); }

int ocean_fft_synchronize(ocean_fft* fft)
{
  if (!fft)
    return fail(OCEAN_ERR_INVALID, "ocean_fft_synchronize: null plan");
  HIP_TRY(hipStreamSynchronize(fft->stream), "hipStreamSynchronize");
  return OCEAN_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Generator
// ---------------------------------------------------------------------------------------------
namespace
{
hipEvent_t take_event(ocean_generator* g)
{
  if (!g->pool.empty())
  {
    hipEvent_t e = g->pool.back();
    g->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// Runs `launch` bracketed by events when profiling is on.
template <typename F>
hipError_t timed(ocean_generator* g, int kind, F&& launch, hipStream_t stream = nullptr)
{
  if (!g->profiling)
    return launch();
  if (!stream)
    stream = g->fft->stream;
  EventPair p{kind, take_event(g), take_event(g)};
  hipError_t e = hipEventRecord(p.a, stream);
  if (e != hipSuccess)
    return e;
  e = launch();
  if (e != hipSuccess)
    return e;
  e = hipEventRecord(p.b, stream);
  g->pending.push_back(p);
  return e;
}

// One slot of the blocked half path's fields
hipError_t half_fields(ocean_generator* g, int slot)
{
  const size_t t = half_field_texels(g->fft->logn) * g->cascades;
  HalfFields& f = g->fields[slot];
  hipError_t e = alloc_if_null(f.gab, t * sizeof(float4));
  e = alloc_if_null(f.gde, t * sizeof(float4), e);
  e = alloc_if_null(f.gc, t * sizeof(float2), e);
  return alloc_if_null(f.spec, (size_t)g->cascades * 2 * g->fft->n * sizeof(float4), e);
}

hipError_t half_buffers(ocean_generator* g)
{
  // slot 0, and pass 1's H scratch: one slice per resident block (1 per CU)
  return alloc_if_null(g->hs, half_hs_bytes(g->fft->logn, g->fft->device_cus), half_fields(g, 0));
}

// The strip-dealt path's geometry: STRIPS kept strips dealt S = ceil(STRIPS / ranks) per rank.
HalfSlab half_slab_geom(int logn, int rank, int ranks)
{
  const int strips = half_strips(logn);
  HalfSlab h{};
  h.S = (strips + ranks - 1) / ranks;
  h.strip0 = rank * h.S;
  h.nstrips = std::max(0, std::min(h.S, strips - h.strip0));
  h.w = (1 << logn) / ranks;
  return h;
}

// strip width of the h0 image the current frame path reads (the whole-grid half path at <= 2
// cascades of 4096: 2-column strips, one per half-strip item, launch_common.h half_h0_block)
int h0_block(const ocean_generator* g)
{
  switch (frame_path(g))
  {
    case FramePath::FourStep:
      return gen4_h0_block();
    case FramePath::HalfBlocked:
      return half_h0_block(g->fft->logn, g->cascades);
    default:
      return spectrum_block(g->fft->logn);
  }
}

// h0 texels per cascade: the whole grid (ranks == 1), or the largest of a slab's layouts (its column
// slab, its dealt strips, its four-step columns blocked 64 wide), so switching paths needs no reallocation
size_t h0_texels(const ocean_generator* g)
{
  const size_t full = (size_t)g->fft->n * g->geom.w;  // the full path's column slab (whole grid: N^2)
  if (g->ranks == 1)
    return full;
  const size_t strips = (size_t)g->hsl.nstrips * spectrum_block(g->fft->logn) * g->fft->n;
  size_t t = std::max(full, strips);
  if (gen4_supported(g->fft->logn))
    t = std::max(t, g->g4.h0_cstride);
  return t;
}

hipError_t full_buffers(ocean_generator* g)
{
  const size_t slab = (size_t)g->fft->n * g->geom.w * g->cascades;
  hipError_t e = alloc_if_null(g->inter, slab * 2 * sizeof(float4));
  return rows_need_transpose(g->fft->logn) ? alloc_if_null(g->scratch, slab * 2 * sizeof(float4), e) : e;
}

// The buffers of the current frame path (allocated when the path is first used; a path switch keeps the
// other paths' buffers)
hipError_t path_buffers(ocean_generator* g)
{
  switch (frame_path(g))
  {
    case FramePath::Full:
      return full_buffers(g);
    case FramePath::HalfBlocked:
      return half_buffers(g);
    default:
      return hslab_buffers(g);
  }
}
}  // namespace

size_t hslab_xbuf_bytes(const ocean_generator* g)
{
  if (frame_path(g) == FramePath::FourStep)
    return (size_t)g->ranks * g->g4.blk_bytes;
  return (size_t)g->ranks * half_slab_block_bytes(g->fft->logn, g->cascades, g->hsl);
}

// Four-step: step 1's parts and the exchange blocks (ranks == 1: one block, read back by the row pass).
// Strip-dealt: the row-major fields and the H scratch.
hipError_t hslab_buffers(ocean_generator* g)
{
  const int logn = g->fft->logn, C = g->cascades;
  hipError_t e = hipSuccess;
  if (frame_path(g) == FramePath::FourStep)
    e = alloc_if_null(g->parts, gen4_parts_bytes(logn, C, g->g4));
  else
  {
    const size_t rt = half_slab_row_texels(logn, C, g->hsl.w);
    e = alloc_if_null(g->rm_ab, rt * sizeof(float4));
    e = alloc_if_null(g->rm_de, rt * sizeof(float4), e);
    e = alloc_if_null(g->rm_c, rt * sizeof(float2), e);
    e = alloc_if_null(g->hs, half_hs_bytes(logn, g->fft->device_cus), e);
  }
  const size_t xb = hslab_xbuf_bytes(g);
  if (e == hipSuccess && g->xbuf_bytes < xb)
  {
    if (g->xbuf)
      (void)hipFree(g->xbuf);
    g->xbuf = nullptr;
    g->xbuf_bytes = 0;
    e = hipMalloc(&g->xbuf, xb);
    if (e == hipSuccess)
      g->xbuf_bytes = xb;
  }
  if (g->ranks > 1)
    e = alloc_if_null(g->h0row, (size_t)C * g->fft->n * sizeof(float4), e);
  return e;
}

namespace
{
int generator_alloc(ocean_generator** out, ocean_fft* fft, int cascades, int rank, int ranks, bool is_slab)
{
  auto* g = new ocean_generator();
  g->fft = fft;
  g->cascades = cascades;
  g->rank = rank;
  g->ranks = ranks;
  g->geom.w = fft->n / ranks;
  g->geom.x0 = rank * g->geom.w;
  g->settings.resize(cascades);
  for (auto& s : g->settings)
    ocean_default_settings(&s);
  g->foam_settings.resize(cascades);
  for (auto& s : g->foam_settings)
    ocean_default_foam_settings(&s);
  const size_t slab = (size_t)fft->n * g->geom.w;  // texels per cascade image slab
  g->slab = is_slab;
  g->half_kind = half_kind_of(fft->logn, is_slab);
  g->half_on = g->half_kind != HalfKind::None;
  g->hsl = half_slab_geom(fft->logn, rank, ranks);
  if (gen4_supported(fft->logn))
  {
    g->g4 = gen4_geom(fft->logn, cascades, rank, ranks, ranks == 1);
    // one h0 cascade stride for every writer and reader (generate_spectrum_with, k_gen4,
    // ocean_generator_initial_spectrum): the largest of the layouts, as allocated
    g->g4.h0_cstride = h0_texels(g);
  }
  // the strip-dealt column pass reads cascade c's strips at (c * nstrips + s) * N * B, which equals
  // h0_texels(g) * c only for one cascade: slabs are single-grid (ocean_generator_create_slab)
  if (is_slab && cascades != 1)
  {
    delete g;
    return fail(OCEAN_ERR_INVALID, "generator allocation: a slab generator holds exactly one cascade");
  }
  const size_t h0_bytes = h0_texels(g) * cascades * sizeof(float4);
  hipError_t e = alloc_if_null(g->h0, h0_bytes);
  if (e == hipSuccess)
    e = path_buffers(g);
  e = alloc_if_null(g->maps, slab * cascades * 2 * sizeof(float4), e);
  e = alloc_if_null(g->jac, slab * cascades * sizeof(float), e);
  // Textures start zeroed like the reference's (Data = nullptr) images.
  if (e == hipSuccess)
    e = hipMemsetAsync(g->h0, 0, h0_bytes, fft->stream);
  if (e == hipSuccess)
    e = hipMemsetAsync(g->maps, 0, slab * cascades * 2 * sizeof(float4), fft->stream);
  if (e == hipSuccess)
    e = hipMemsetAsync(g->jac, 0, slab * cascades * sizeof(float), fft->stream);
  if (e != hipSuccess)
  {
    ocean_generator_destroy(g);
    return alloc_fail(e, "generator allocation");
  }
  *out = g;
  return OCEAN_OK;
}

// h0, h0row and the fused re-seed constants are written on the generator's stream; a column pass that
// ran on another stream (the one-sided exchange's step-1 / put streams) may still be reading them
int wait_h0_readers(ocean_generator* g)
{
  if (g->cols_ev_valid)
    HIP_TRY(hipStreamWaitEvent(g->fft->stream, g->h0r_ev, 0), "h0 write: wait for the last column pass");
  return OCEAN_OK;
}

// One launch of the seeding kernel: `cols` columns from x0 into a cascade's h0 image at texel `at`, in
// strips `block` columns wide (0: spectrum_block)
struct H0Piece
{
  size_t at;
  int x0, cols, block;
};

struct H0Pieces
{
  H0Piece piece[2];
  int count = 0;
  bool row0 = false;  // slabs: also row y = 0 of every column into h0row (the Nyquist-row term)
};

// What the current frame path keeps in a cascade's h0 image
H0Pieces h0_pieces(const ocean_generator* g)
{
  const int n = g->fft->n;
  const FramePath path = frame_path(g);
  H0Pieces p;
  if (g->ranks > 1 && path == FramePath::FourStep)
  {
    // this rank's kept columns x = N/2 + u0 .. (blocked 64 wide), rank P - 1 also the block of
    // x = 0 .. 63 (the Nyquist column x = 0 is its first)
    const Gen4Geom& q = g->g4;
    const int B = gen4_h0_block();
    p.piece[p.count++] = {q.h0_reg, n / 2 + q.u0, q.cols, B};
    if (q.nyq)
      p.piece[p.count++] = {q.h0_nyq, 0, B, B};
    p.row0 = true;
  }
  else if (g->ranks > 1 && path == FramePath::StripDealt)
  {
    // this rank's strips: the regular ones are columns N/2 + strip*B .. (contiguous), the last
    // global strip is the Nyquist strip x = 0..B-1
    const int B = spectrum_block(g->fft->logn), strips = half_strips(g->fft->logn);
    const HalfSlab& h = g->hsl;
    const int nreg = std::max(0, std::min(h.nstrips, strips - 1 - h.strip0));
    if (nreg > 0)
      p.piece[p.count++] = {0, n / 2 + h.strip0 * B, nreg * B, 0};
    if (nreg < h.nstrips)
      p.piece[p.count++] = {(size_t)nreg * n * B, 0, B, 0};
    p.row0 = true;
  }
  else
    p.piece[p.count++] = {0, g->geom.x0, g->geom.w, h0_block(g)};
  return p;
}

// generateSpectrum with the given per-cascade settings (the current ones, or those a fused re-seed
// frame evaluated h0 with, when that h0 image is materialised later)
int generate_spectrum_with(ocean_generator* g, const std::vector<ocean_settings>& settings)
{
  TRY(wait_h0_readers(g));  // write-after-read on h0 (a pipelined put frame still in flight)
  g->h0_dirty = true;
  g->h0_stale = false;
  g->h0_block = h0_block(g);
  g->h0_settings = settings;
  g->seeded = settings;
  ocean_fft* f = g->fft;
  const H0Pieces pieces = h0_pieces(g);
  for (int c = 0; c < g->cascades; c++)
  {
    OceanSettings s;
    std::memcpy(&s, &settings[c], sizeof(s));
    float4* base = g->h0 + h0_texels(g) * c;
    HIP_TRY(timed(g, 0, [&] {
              hipError_t e = hipSuccess;
              for (int i = 0; i < pieces.count && e == hipSuccess; i++)
              {
                const H0Piece& p = pieces.piece[i];
                e = launch_generate_spectrum(s, f->n, base + p.at, f->stream, f->cus, p.x0, p.cols, p.block);
              }
              if (e == hipSuccess && pieces.row0)
                e = launch_generate_spectrum_row(s, f->n, g->h0row + (size_t)c * f->n, f->stream);
              return e;
            }),
            "generateSpectrum");
  }
  return OCEAN_OK;
}

// True when h0 seeded from `a` and from `b` is the same image: every field but the accumulated
// time (generateSpectrum does not read it, spectrum.compute:157-172).
bool same_h0_inputs(const std::vector<ocean_settings>& a, const std::vector<ocean_settings>& b)
{
  if (a.size() != b.size())
    return false;
  for (size_t i = 0; i < a.size(); i++)
  {
    ocean_settings x = a[i], y = b[i];
    x.time = y.time = 0.0f;
    if (std::memcmp(&x, &y, sizeof(x)) != 0)
      return false;
  }
  return true;
}

// Fused re-seed (src/Generator.cpp:55-59 followed by :63-72): pass 1 evaluates h0 itself from one
// record of constants per cascade, `seed`; the h0 image is left stale
int fused_reseed(ocean_generator* g, const void*& seed)
{
  ocean_fft* f = g->fft;
  std::vector<unsigned char> host((size_t)g->cascades * seed_consts_bytes());
  for (int c = 0; c < g->cascades; c++)
  {
    OceanSettings os;
    std::memcpy(&os, &g->settings[c], sizeof(os));
    seed_consts(os, f->n, host.data() + (size_t)c * seed_consts_bytes());
  }
  if (!g->seedc)
    HIP_TRY(hipMalloc(&g->seedc, (size_t)kMaxCascades * seed_consts_bytes()), "seed constants");
  if (host != g->seedc_host)  // pageable source: staged before the call returns
  {
    TRY(wait_h0_readers(g));
    HIP_TRY(hipMemcpyAsync(g->seedc, host.data(), host.size(), hipMemcpyHostToDevice, f->stream), "seed constants");
    g->seedc_host.swap(host);
  }
  seed = g->seedc;
  g->h0_dirty = true;
  g->h0_stale = true;
  g->seed_settings = g->settings;
  g->seeded = g->settings;
  return OCEAN_OK;
}

// What a column pass does about h0 (src/Generator.cpp:55-59): nothing, a (fused) re-seed, the first
// seeding, or writing the image that fused frames or a path switch left to do. `seed`: the constants of a
// fused re-seed, null when pass 1 reads the h0 image.
int seed_h0(ocean_generator* g, int update_spectrum, const void*& seed)
{
  // The reference app asks for a re-seed on every frame (src/Waves.cpp:91-94); when the h0 inputs
  // are unchanged since the last seeding the result would be bit-identical, so it is skipped.
  if (update_spectrum && !g->update_spectrum && g->memo_h0 && same_h0_inputs(g->settings, g->seeded))
    update_spectrum = 0;
  if (g->update_spectrum || update_spectrum)
  {
    // The generator's first seeding writes the h0 image. Explicit re-seeds (the reference app's
    // every-frame CalculateOcean(dt, true)) are fused into pass 1 on the blocked half path; the
    // inlined ocml functions round the same amplitude within an ulp of the seeding kernels' (frames
    // agree to ~1e-7 of max, test_fused_reseed_frames), so the first frame keeps the kernels that
    // slabs and batches are compared with bit-exactly.
    const bool fused = update_spectrum && !g->update_spectrum && frame_path(g) == FramePath::HalfBlocked && g->hs;
    g->update_spectrum = false;
    return fused ? fused_reseed(g, seed) : ocean_generator_generate_spectrum(g);
  }
  TRY(materialise_h0(g));          // the next frames read the h0 image
  if (g->h0_block != h0_block(g))  // the frame path changed (four-step on/off): same h0, new layout
    TRY(generate_spectrum_with(g, g->h0_settings));
  return OCEAN_OK;
}

FrameParams frame_params(const ocean_generator* g)
{
  FrameParams fp{};
  fp.cascades = g->cascades;
  for (int c = 0; c < g->cascades; c++)
  {
    const ocean_settings& s = g->settings[c];
    // spectrum.compute:189 — `2.0 * M_PI / planeSize` in fp32
    fp.c[c].dk = 2.0f * 3.14159265358f / s.planeSize;
    fp.c[c].time = s.time;
    fp.c[c].g = s.g;
    fp.c[c].h = s.h;
  }
  return fp;
}

// The column pass of the strip-dealt and four-step paths, on col_stream (null: the generator's stream).
// put (the one-sided exchange): step 2 stores into the peers' receive slots.
int half_slab_columns(ocean_generator* g, const FrameParams& fp, float4* out, const Gen4Put* put,
                      hipStream_t col_stream)
{
  ocean_fft* f = g->fft;
  const hipError_t eb = hslab_buffers(g);  // the current path's buffers (a path switch allocates here)
  if (eb != hipSuccess)
    return alloc_fail(eb, "column pass buffers");
  // the column pass's stream (the put or step-1 stream of pipelined one-sided frames) runs after the
  // last column pass on another stream (step 1 rewrites the parts its step 2 read; the strip-dealt
  // pass reuses its H scratch) and after h0 writes
  hipStream_t cs = col_stream ? col_stream : f->stream;
  // both orderings, independently: after the last column pass (whatever stream it ran on), and after
  // the h0 writes on the generator's stream when this pass runs elsewhere
  if (g->cols_ev_valid)
    HIP_TRY(hipStreamWaitEvent(cs, g->cols_ev, 0), "column pass: after the last column pass");
  if (cs != f->stream && g->h0_dirty)
  {
    if (!g->put_h0)
      HIP_TRY(hipEventCreateWithFlags(&g->put_h0, hipEventDisableTiming), "column pass: event");
    HIP_TRY(hipEventRecord(g->put_h0, f->stream), "column pass: stream event");
    HIP_TRY(hipStreamWaitEvent(cs, g->put_h0, 0), "column pass: stream order");
    g->h0_dirty = false;  // only once the wait is enqueued
  }
  // profiling a put: kind 3 brackets the wait + put kernels inside the column pass (kind 1)
  Gen4Put timed_put = put ? *put : Gen4Put{};
  EventPair pp{3, nullptr, nullptr};
  if (put && g->profiling)
  {
    pp.a = take_event(g);
    pp.b = take_event(g);
    timed_put.start = pp.a;
  }
  if (frame_path(g) == FramePath::FourStep)
    HIP_TRY(timed(g, 1, [&] {
              return launch_gen4_columns(f->logn, fp, g->g4, g->h0, g->ranks > 1 ? g->h0row : nullptr,
                                         put && put->parts ? put->parts : g->parts, out ? (void*)out : (void*)g->xbuf,
                                         f->twiddles, f->tw2, cs, f->cus, put ? &timed_put : nullptr);
            }, cs),
            "column pass (half spectrum, four-step)");
  else
    HIP_TRY(timed(g, 1, [&] {
              return launch_half_slab_columns(f->logn, fp, g->hsl, g->ranks, g->h0, g->ranks == 1, g->h0row,
                                              out ? (void*)out : (void*)g->xbuf, f->twiddles, cs, f->cus, g->hs,
                                              f->device_cus, put ? &timed_put : nullptr);
            }, cs),
            "column pass (half spectrum, strip-dealt)");
  if (pp.a)
  {
    HIP_TRY(hipEventRecord(pp.b, put && put->stream ? put->stream : cs), "column pass: put event");
    g->pending.push_back(pp);
  }
  for (hipEvent_t* ev : {&g->cols_ev, &g->h0r_ev})
    if (!*ev)
      HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming), "column pass: event");
  HIP_TRY(hipEventRecord(g->cols_ev, cs), "column pass: end event");
  // the h0 readers end on the put stream when step 2 runs there (it waited for step 1's handoff)
  HIP_TRY(hipEventRecord(g->h0r_ev, put && put->stream ? put->stream : cs), "column pass: end event");
  g->cols_ev_valid = true;
  return OCEAN_OK;
}

// Frame overlap: the blocked half path's column pass on the side stream into field slot oslot, after the
// row pass that last read the slot, and after any h0 / seed-constant writes on the generator's stream
int overlapped_columns(ocean_generator* g, const FrameParams& fp, const void* seed)
{
  ocean_fft* f = g->fft;
  const int s = g->oslot;
  if (g->h0_dirty)
  {
    HIP_TRY(hipEventRecord(g->oh0, f->stream), "overlap: h0 event");
    HIP_TRY(hipStreamWaitEvent(g->side, g->oh0, 0), "overlap: h0 wait");
    g->h0_dirty = false;
  }
  if (g->orows_valid[s])
    HIP_TRY(hipStreamWaitEvent(g->side, g->orows[s], 0), "overlap: slot wait");
  const HalfFields& fl = g->fields[s];
  HIP_TRY(timed(g, 1, [&] {
            return launch_half_columns(f->logn, fp, g->h0, fl.gab, fl.gde, fl.gc, fl.spec, f->twiddles, g->side, f->cus,
                                       g->hs, f->device_cus, seed, g->h0_block);
          }, g->side),
          "column pass (half spectrum, overlapped)");
  HIP_TRY(hipEventRecord(g->ocols[s], g->side), "overlap: column event");
  return OCEAN_OK;
}

// The buffer a whole-grid frame, or a slab frame without a caller's buffer, passes between its passes
// (null: the half-slab paths' own exchange buffer)
float4* own_exchange(const ocean_generator* g) { return half_slab_path(g) ? nullptr : g->inter; }

// A pipelined frame in flight (one-sided or RCCL) lands before a path switch: its column pass wrote its
// blocks in the current path's layout, so its row pass runs first
int land_frames_in_flight(ocean_generator* g)
{
  if (peers_pending(g->peers))
    TRY(ocean_peers_flush(g->peers));
  return ocean_generator_slab_flush(g);
}
}  // namespace

// First half of CalculateOcean: time += dt (src/Generator.cpp:50), h0 if requested (:55-59),
// prepareFFT fused with the y direction of both EncodeIFFTs (:63-72). Output in destination-block
// order into `out` (the internal buffer when null).
int generator_columns(ocean_generator* g, float timestep, int update_spectrum, float4* out, const Gen4Put* put,
                      hipStream_t col_stream)
{
  ocean_fft* f = g->fft;
  g->rates_fresh = false;  // the rates belong to the time and h0 of the column pass before this one
  g->kin_fresh = false;    // and so do the depth layers
  for (auto& s : g->settings)
    s.time += timestep;
  const void* seed = nullptr;
  TRY(seed_h0(g, update_spectrum, seed));
  const FrameParams fp = frame_params(g);
  if (put && !half_slab_path(g))
    return fail(OCEAN_ERR_INVALID, "column pass: the one-sided exchange needs a half-spectrum slab path (N >= 1024)");
  switch (frame_path(g))
  {
    case FramePath::FourStep:
    case FramePath::StripDealt:
      TRY(half_slab_columns(g, fp, out, put, col_stream));
      break;
    case FramePath::HalfBlocked:
      if (g->overlap)
        TRY(overlapped_columns(g, fp, seed));
      else
        HIP_TRY(timed(g, 1, [&] {
                  const HalfFields& fl = g->fields[0];
                  return launch_half_columns(f->logn, fp, g->h0, fl.gab, fl.gde, fl.gc, fl.spec, f->twiddles, f->stream,
                                             f->cus, g->hs, f->device_cus, seed, g->h0_block);
                }),
                "column pass (half spectrum)");
      break;
    case FramePath::Full:
      HIP_TRY(timed(g, 1, [&] {
                return launch_cols_evolve(f->logn, fp, g->geom, g->h0, out, f->twiddles, f->stream, f->cus,
                                          default_keep(f->logn));
              }),
              "column pass");
      break;
  }
  g->frame = fp;
  return OCEAN_OK;
}

FrameState current_frame(const ocean_generator* g)
{
  FrameState fs{g->frame, FoamParams{}};
  for (int c = 0; c < g->cascades; c++)
    fs.foam.displacement[c] = g->settings[c].displacement;
  return fs;
}

// Second half: the x direction of both EncodeIFFTs + computeFoam (src/Generator.cpp:71-80), with the
// column-pass values and the displacement of the frame `fs`.
int generator_rows(ocean_generator* g, const float4* in, const FrameState& fs, hipStream_t row_stream, int row_cus)
{
  ocean_fft* f = g->fft;
  g->mips_fresh = false;  // every frame path's maps are written here
  g->bounds_fresh = false;
  const int rcus = row_cus > 0 && row_cus < f->cus ? row_cus : f->cus;
  if (row_stream && !half_slab_path(g))
    return fail(OCEAN_ERR_INVALID, "row pass: a row stream needs a half-spectrum slab path");
  hipStream_t rs = row_stream ? row_stream : f->stream;
  switch (frame_path(g))
  {
    case FramePath::FourStep:
      HIP_TRY(timed(g, 2, [&] {
                return launch_gen4_rows(f->logn, fs.frame, g->g4, in ? (const void*)in : (const void*)g->xbuf, g->maps,
                                        g->jac, fs.foam, f->twiddles, f->tw2, rs, rcus);
              }, rs),
              "row pass (half spectrum, four-step)");
      break;
    case FramePath::StripDealt:
      HIP_TRY(timed(g, 2, [&] {
                return launch_half_slab_rows(f->logn, fs.frame, g->hsl, in ? (const void*)in : (const void*)g->xbuf,
                                             g->rm_ab, g->rm_de, g->rm_c, g->maps, g->jac, fs.foam, f->twiddles,
                                             f->tw2, rs, rcus);
              }, rs),
              "row pass (half spectrum, strip-dealt)");
      break;
    case FramePath::HalfBlocked:
    {
      // frame overlap: the slot the side stream's column pass wrote, then the other one
      const int s = g->overlap ? g->oslot : 0;
      const HalfFields& fl = g->fields[s];
      if (g->overlap)
        HIP_TRY(hipStreamWaitEvent(f->stream, g->ocols[s], 0), "overlap: column wait");
      HIP_TRY(timed(g, 2, [&] {
                return launch_half_rows(f->logn, fs.frame, fl.gab, fl.gde, fl.gc, fl.spec, g->maps, g->jac, fs.foam,
                                        f->twiddles, f->stream, f->cus);
              }),
              g->overlap ? "row pass (half spectrum, overlapped)" : "row pass (half spectrum)");
      if (g->overlap)
      {
        HIP_TRY(hipEventRecord(g->orows[s], f->stream), "overlap: row event");
        g->orows_valid[s] = true;
        g->oslot = s ^ 1;
      }
      break;
    }
    case FramePath::Full:
      HIP_TRY(timed(g, 2, [&] {
                return launch_rows_final(f->logn, g->cascades, g->geom, in, g->scratch, g->maps, g->jac, fs.foam,
                                         f->twiddles, f->stream, f->cus);
              }),
              "row pass");
      break;
  }
  return OCEAN_OK;
}

// After fused re-seed frames: write the h0 image those frames evaluated (their settings snapshot).
int materialise_h0(ocean_generator* g)
{
  return g->h0_stale ? generate_spectrum_with(g, g->seed_settings) : OCEAN_OK;
}

extern "C" {

int ocean_generator_create(ocean_generator** out, ocean_fft* fft, int cascades)
{
  if (!out || !fft)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_create: null argument");
  *out = nullptr;
  if (cascades < 1 || cascades > OCEAN_MAX_CASCADES)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_create: cascades must be in [1, 64]");
  return generator_alloc(out, fft, cascades, 0, 1, false);
}

int ocean_generator_create_slab(ocean_generator** out, ocean_fft* fft, int rank, int ranks)
{
  if (!out || !fft)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_create_slab: null argument");
  *out = nullptr;
  const int blk = spectrum_block(fft->logn);
  if (ranks < 1 || ranks > 16 || (ranks & (ranks - 1)) != 0 || rank < 0 || rank >= ranks)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_create_slab: ranks must be a power of two in [1, 16], 0 <= rank < ranks");
  const int w = fft->n / ranks;
  if (w % blk != 0 || w < fft->n / 16 || w < slab_min_width(fft->logn))
    return fail(OCEAN_ERR_INVALID, "ocean_generator_create_slab: N / ranks = " + std::to_string(w) +
                                       " is below this size's minimum slab width " +
                                       std::to_string(slab_min_width(fft->logn)));
  return generator_alloc(out, fft, 1, rank, ranks, true);
}

int ocean_generator_destroy(ocean_generator* g)
{
  if (!g)
    return OCEAN_OK;
  // A pipelined slab frame still in flight: its exchange may be running on comm_stream (the
  // communicator must outlive the generator, include/oceanfft.h). Drain it before the slots go.
  if (g->comm_stream)
    (void)hipStreamSynchronize(g->comm_stream);
  if (g->peers)
    peers_detach(g->peers);
  if (g->fft)
    (void)hipStreamSynchronize(g->fft->stream);
  if (g->side)
    (void)hipStreamSynchronize(g->side);
  for (hipStream_t st : {g->comm_stream, g->side})
    if (st)
      (void)hipStreamDestroy(st);
  for (auto& p : g->pending)
    for (hipEvent_t ev : {p.a, p.b})
      g->pool.push_back(ev);
  for (hipEvent_t ev : g->pool)
    (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {g->cols_done[0], g->cols_done[1], g->xchg_done[0], g->xchg_done[1], g->rows_done[0],
                        g->rows_done[1], g->put_h0, g->cols_ev, g->h0r_ev, g->ocols[0], g->ocols[1], g->orows[0],
                        g->orows[1], g->oh0})
    if (ev)
      (void)hipEventDestroy(ev);
  const HalfFields &f0 = g->fields[0], &f1 = g->fields[1];
  for (void* p : {(void*)g->h0, (void*)g->inter, (void*)g->scratch, (void*)g->maps, (void*)g->jac, (void*)g->xsend[0],
                  (void*)g->xsend[1], (void*)g->xrecv[0], (void*)g->xrecv[1], (void*)f0.gab, (void*)f0.gde, (void*)f0.gc,
                  (void*)f0.spec, (void*)f1.gab, (void*)f1.gde, (void*)f1.gc, (void*)f1.spec, (void*)g->hs,
                  (void*)g->h0row, g->seedc, (void*)g->rm_ab, (void*)g->rm_de, (void*)g->rm_c, (void*)g->parts,
                  (void*)g->xbuf, (void*)g->mips, (void*)g->rates, (void*)g->kin, (void*)g->bounds, (void*)g->foam, g->foam_counts,
                  (void*)g->deposit_acc, g->deposit_counts})
    if (p)
      (void)hipFree(p);
  delete g;
  return OCEAN_OK;
}

int ocean_generator_cascades(const ocean_generator* g) { return g ? g->cascades : 0; }

ocean_settings* ocean_generator_settings(ocean_generator* g, int c)
{
  if (!g || c < 0 || c >= g->cascades)
  {
    fail(OCEAN_ERR_INVALID, "ocean_generator_settings: cascade out of range");
    return nullptr;
  }
  return &g->settings[c];
}

int ocean_generator_generate_spectrum(ocean_generator* g)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_generate_spectrum: null generator");
  return generate_spectrum_with(g, g->settings);
}

int ocean_generator_set_half_spectrum(ocean_generator* g, int enable)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_half_spectrum: null generator");
  TRY(land_frames_in_flight(g));
  if (!enable && g->overlap)
    TRY(ocean_generator_set_frame_overlap(g, 0));
  if (enable && g->half_kind == HalfKind::None)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_half_spectrum: N = 1024 .. 16384 only");
  const bool was_on = g->half_on, was_slab_path = half_slab_path(g);
  g->half_on = enable != 0;
  const hipError_t e = path_buffers(g);
  if (e != hipSuccess)
  {
    g->half_on = was_on;
    return alloc_fail(e, "ocean_generator_set_half_spectrum");
  }
  if ((was_slab_path && g->ranks > 1) != (half_slab_path(g) && g->ranks > 1))
    g->update_spectrum = true;  // a slab's h0 layout changes (its strips or columns <-> its column slab)
  return OCEAN_OK;
}

int ocean_generator_set_frame_overlap(ocean_generator* g, int enable)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_frame_overlap: null generator");
  if (enable && frame_path(g) != FramePath::HalfBlocked)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_frame_overlap: whole grids of N = 1024 .. 4096 on the "
                                   "half-spectrum path only");
  ocean_fft* f = g->fft;
  if (enable && !g->overlap)
  {
    hipError_t e = hipSuccess;
    if (!g->side)
      e = hipStreamCreateWithFlags(&g->side, hipStreamNonBlocking);
    for (hipEvent_t* ev : {&g->ocols[0], &g->ocols[1], &g->orows[0], &g->orows[1], &g->oh0})
      if (e == hipSuccess && !*ev)
        e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess)
      e = half_fields(g, 1);
    // the side stream starts after everything issued so far (the last column pass used slot 0 and hs)
    if (e == hipSuccess)
      e = hipEventRecord(g->oh0, f->stream);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(g->side, g->oh0, 0);
    if (e != hipSuccess)
      return alloc_fail(e, "ocean_generator_set_frame_overlap");
    g->orows_valid[0] = g->orows_valid[1] = false;
    g->oslot = 0;
    g->h0_dirty = false;
    g->overlap = true;
  }
  else if (!enable && g->overlap)
  {
    // later frames run on the generator's stream in slot 0: after every overlapped pass
    for (int s = 0; s < 2; s++)
      if (g->orows_valid[s])
        HIP_TRY(hipStreamWaitEvent(f->stream, g->orows[s], 0), "ocean_generator_set_frame_overlap");
    HIP_TRY(hipEventRecord(g->oh0, g->side), "ocean_generator_set_frame_overlap");
    HIP_TRY(hipStreamWaitEvent(f->stream, g->oh0, 0), "ocean_generator_set_frame_overlap");
    g->overlap = false;
  }
  return OCEAN_OK;
}

int ocean_generator_set_h0_memo(ocean_generator* g, int enable)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_h0_memo: null generator");
  g->memo_h0 = enable != 0;
  return OCEAN_OK;
}

int ocean_generator_set_four_step(ocean_generator* g, int enable)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_four_step: null generator");
  TRY(land_frames_in_flight(g));
  g->four_step = enable != 0;  // h0 is re-laid out by the next frame if its strip width changes
  if (half_slab_path(g))
  {
    const hipError_t e = hslab_buffers(g);  // exchange_bytes reports the new path's size from here on
    if (e != hipSuccess)
      return alloc_fail(e, "ocean_generator_set_four_step");
  }
  return OCEAN_OK;
}

int ocean_generator_frame_bytes(const ocean_generator* g, double per_point[2])
{
  if (!g || !per_point)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_frame_bytes: null argument");
  const double n = g->fft->n;
  switch (const FramePath path = frame_path(g))
  {
    case FramePath::FourStep:
    {
      // the kept columns u' in [0, N/2) and the Nyquist column: step 1 reads h0 (16) and writes 5
      // complex fields (40), step 2 reads and writes them (40 + 40, into the exchange blocks) | the row
      // pass reads them (40) and writes the maps + Jacobian (36)
      const double kept = (n / 2 + 1) / n;
      per_point[0] = (16.0 + 40.0 + 80.0) * kept;
      per_point[1] = 40.0 * kept + 36.0;
      break;
    }
    case FramePath::HalfBlocked:
    case FramePath::StripDealt:
    {
      // h0 of the kept columns (half + the Nyquist strip) + 5 complex fields out; 5 fields in, maps +
      // Jacobian; the strip-dealt path also moves the received fields to row-major (40 in + 40 out)
      const double kept = (n / 2 + spectrum_block(g->fft->logn)) / n;
      per_point[0] = 16.0 * kept + 40.0 * kept;
      per_point[1] = 40.0 * kept + 36.0 + (path == FramePath::StripDealt ? 80.0 * kept : 0.0);
      break;
    }
    case FramePath::Full:
      per_point[0] = 48.0;
      per_point[1] = 68.0 + (rows_need_transpose(g->fft->logn) ? 64.0 : 0.0);  // B = 1: the tiled transpose
      break;
  }
  return OCEAN_OK;
}

int ocean_generator_calculate(ocean_generator* g, float timestep, int update_spectrum)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_calculate: null generator");
  if (g->ranks != 1)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_calculate: slab generators step with "
                                   "ocean_generator_slab_columns / exchange / ocean_generator_slab_rows");
  float4* buf = own_exchange(g);
  TRY(generator_columns(g, timestep, update_spectrum, buf));
  return generator_rows(g, buf, current_frame(g));
}

size_t ocean_generator_exchange_bytes(const ocean_generator* g)
{
  if (!g)
    return 0;
  if (half_slab_path(g))
    return hslab_xbuf_bytes(g);
  return (size_t)g->cascades * 2 * g->fft->n * g->geom.w * sizeof(float4);
}

int ocean_generator_slab_columns(ocean_generator* g, float timestep, int update_spectrum, float* send)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_slab_columns: null generator");
  return generator_columns(g, timestep, update_spectrum, send ? reinterpret_cast<float4*>(send) : own_exchange(g));
}

int ocean_generator_slab_rows(ocean_generator* g, const float* recv)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_slab_rows: null generator");
  return generator_rows(g, recv ? reinterpret_cast<const float4*>(recv) : own_exchange(g), current_frame(g));
}

int ocean_slab_layout(size_t texture_size, int rank, int ranks, int half, int64_t out[6])
{
  int logn = 0;
  while (logn < 15 && ((size_t)1 << logn) < texture_size)
    logn++;
  if (!out || ((size_t)1 << logn) != texture_size || logn < 4 || logn > 14 || ranks < 1 || ranks > 16 ||
      (ranks & (ranks - 1)) != 0 || rank < 0 || rank >= ranks)
    return fail(OCEAN_ERR_INVALID, "ocean_slab_layout: N a power of two in [16, 16384], ranks a power of two <= 16");
  if (half && !half_slab_supported(logn))
    return fail(OCEAN_ERR_INVALID, "ocean_slab_layout: the half-spectrum path needs N >= 1024");
  if (half == 2 && !gen4_supported(logn))
    return fail(OCEAN_ERR_INVALID, "ocean_slab_layout: the four-step path needs N = 8192 or 16384");
  const int n = 1 << logn, w = n / ranks;
  if (half == 2)
  {
    const Gen4Geom q = gen4_geom(logn, 1, rank, ranks, ranks == 1);
    const int64_t v[6] = {q.u0, q.cols, q.nyq, q.w, (int64_t)q.blk_bytes, (int64_t)q.blk_bytes * ranks};
    std::memcpy(out, v, sizeof(v));
  }
  else if (half)
  {
    const HalfSlab h = half_slab_geom(logn, rank, ranks);
    const int64_t blk = (int64_t)half_slab_block_bytes(logn, 1, h);
    const int64_t v[6] = {h.strip0, h.nstrips, h.S, h.w, blk, blk * ranks};
    std::memcpy(out, v, sizeof(v));
  }
  else
  {
    const int64_t blk = (int64_t)2 * w * w * sizeof(float4);
    const int64_t v[6] = {(int64_t)rank * w, w, 0, w, blk, blk * ranks};
    std::memcpy(out, v, sizeof(v));
  }
  return OCEAN_OK;
}

int ocean_generator_slab_info(const ocean_generator* g, int* rank, int* ranks, int* row0, int* rows)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_slab_info: null generator");
  if (rank)
    *rank = g->rank;
  if (ranks)
    *ranks = g->ranks;
  if (row0)
    *row0 = g->rank * g->geom.w;
  if (rows)
    *rows = g->geom.w;
  return OCEAN_OK;
}

float* ocean_generator_initial_spectrum(ocean_generator* g, int c)
{
  if (!g || c < 0 || c >= g->cascades)
    return nullptr;
  if (materialise_h0(g) != OCEAN_OK)  // after fused re-seed frames
    return nullptr;
  // the caller may write h0 through this pointer: the next requested re-seed must regenerate it, as
  // the reference does on every request (src/Generator.cpp:55-59), so the h0 memo forgets its inputs
  g->seeded.clear();
  g->h0_dirty = true;  // frame overlap: the next column pass waits for the caller's stream (its h0 writes)
  return reinterpret_cast<float*>(g->h0 + h0_texels(g) * c);
}

int ocean_generator_spectrum_block(const ocean_generator* g)
{
  return g ? (g->h0_block > 0 ? g->h0_block : h0_block(g)) : 0;  // the layout h0 holds now
}

int ocean_generator_set_profiling(ocean_generator* g, int enable)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_set_profiling: null generator");
  g->profiling = enable != 0;
  return OCEAN_OK;
}

int ocean_generator_kernel_times4(ocean_generator* g, double ms_total[4], int64_t launches[4])
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_kernel_times: null generator");
  HIP_TRY(hipStreamSynchronize(g->fft->stream), "hipStreamSynchronize");
  for (auto& p : g->pending)
  {
    float ms = 0.0f;
    HIP_TRY(hipEventSynchronize(p.b), "hipEventSynchronize");  // pairs on the put stream too
    HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b), "hipEventElapsedTime");
    g->ms[p.kind] += ms;
    g->launches[p.kind] += 1;
    g->pool.push_back(p.a);
    g->pool.push_back(p.b);
  }
  g->pending.clear();
  for (int k = 0; k < 4; k++)
  {
    if (ms_total)
      ms_total[k] = g->ms[k];
    if (launches)
      launches[k] = g->launches[k];
    g->ms[k] = 0;
    g->launches[k] = 0;
  }
  return OCEAN_OK;
}

int ocean_generator_kernel_times(ocean_generator* g, double ms_total[3], int64_t launches[3])
{
  double m[4];
  int64_t l[4];
  const int rc = ocean_generator_kernel_times4(g, m, l);
  for (int k = 0; rc == OCEAN_OK && k < 3; k++)
  {
    if (ms_total)
      ms_total[k] = m[k];
    if (launches)
      launches[k] = l[k];
  }
  return rc;
}

int ocean_debug_copy(void* dst, const void* src, size_t bytes, int workgroups, void* hip_stream)
{
  if ((bytes > 0 && (!dst || !src)) || bytes % 16 != 0 || workgroups < 1 || workgroups > 65536 ||
      (reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) % 16 != 0)
    return fail(OCEAN_ERR_INVALID, "ocean_debug_copy: null or unaligned pointer, bytes not a multiple of 16, or "
                                   "workgroups outside [1, 65536]");
  if (bytes == 0)
    return OCEAN_OK;
  HIP_TRY(launch_debug_copy(dst, src, bytes, workgroups, (hipStream_t)hip_stream), "debug copy");
  return OCEAN_OK;
}

int ocean_debug_hash(const uint32_t* xy, int count, uint32_t* raw, float* uv, void* hip_stream)
{
  if (!xy || !raw || !uv || count < 0)
    return fail(OCEAN_ERR_INVALID, "ocean_debug_hash: null argument");
  if (count == 0)
    return OCEAN_OK;
  HIP_TRY(launch_hash(xy, count, raw, reinterpret_cast<float2*>(uv), (hipStream_t)hip_stream), "hash");
  return OCEAN_OK;
}

}  // extern "C"
