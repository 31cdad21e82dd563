// ocean_internal.h — types shared between the device code and the C-ABI implementation.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace oceanfft
{

// Waves::GeneratorSettings (src/Generator.h:12-30) == spectrumSettings UBO (spectrum.compute:10-27).
struct OceanSettings
{
  int32_t seed[2];
  float U_10;
  float theta_0;
  float F;
  float g;
  float swell;
  float h;
  float displacement;
  float time;
  float planeSize;
  float scale;
  float spread;
  int32_t boundWavelength;
  float wavelengthMin;
  float wavelengthMax;
};
static_assert(sizeof(OceanSettings) == 64, "GeneratorSettings is 64 bytes");

constexpr int kMaxCascades = 64;  // cascades per launch (kernel-argument tables below)
constexpr int kMaxSurfaceCascades = 16;

// Surface consumer (resources/waveShader.glsl): the maps one cascade binds, plus its planeSize and
// displacement scale (src/Renderer.cpp:62-72).
struct SurfaceCascade
{
  const float4* height;
  const float4* disp;
  const float* jac;
  float plane;
  float scale;
  // the LOD calls only (else null): the maps' mip chains, level l >= 1 at mip_level_offset(n, l) texels
  // (device/mip_index.h)
  const float4* height_mip;
  const float4* disp_mip;
  const float* jac_mip;
};
struct SurfaceParams
{
  int count;  // cascades
  int n;      // map side (power of two)
  SurfaceCascade c[kMaxSurfaceCascades];
  // null: the stages sample the maps; else the surface atlas [cascade][2][n * n] (launch_surface):
  // (h, Dx, Dz, 0) for the vertex stage, (dh/dx, dh/dz, dDx/dx, dDz/dz) for the normal stage
  float4* atlas;
};
// The reference plane mesh and camera (waveShader.glsl:77-98); res == 0: explicit positions.
struct SurfacePlane
{
  int res;
  float cam_x, cam_y, cam_z, fwd_x, fwd_z;
};

// Per-cascade values the evolve/row kernel needs (passed by value: no per-frame H2D copy).
struct CascadeFrame
{
  float dk;    // 2*pi/planeSize, evaluated in fp32 exactly as spectrum.compute:189
  float time;  // accumulated in fp32 like src/Generator.cpp:50
  float g;
  float h;
};

struct FrameParams
{
  int cascades;
  int pad[3];
  CascadeFrame c[kMaxCascades];
};

struct FoamParams
{
  float displacement[kMaxCascades];
};

// Slab decomposition of one N x N grid over `ranks` GPUs (ranks == 1: the whole grid). This rank
// owns columns [x0, x0 + w) in the column pass and rows [rank*w, rank*w + w) in the row pass,
// w = N / ranks. Pass 1 writes its output in destination-block order (block q = rows q*w..q*w+w-1),
// so one equal-split all-to-all turns it into the row pass's input.
struct SlabGeom
{
  int x0;
  int w;
};

// Half-spectrum strip-dealt layout (slabs of any N >= 1024, and whole grids of N = 8192 / 16384).
// The STRIPS = N / (2B) + 1 kept strips (columns u >= 0, then the Nyquist strip x = 0..B-1) are
// dealt S per rank, rank r taking [r S, min(r S + S, STRIPS)). Pass 1 writes block q (rows
// [q w, q w + w)) of its output as three parts of C * S * w * B elements: gab float4 | gde float4 |
// gc float2, element ((c S + sl) w + yl) B + b; then the frame's Nyquist-row term [c][2][N] float4.
struct HalfSlab
{
  int strip0;   // first global strip of this rank
  int nstrips;  // strips this rank transforms (<= S)
  int S;        // strip slots per block
  int w;        // rows per block = rows of this rank's row pass
};

// Four-step column pass of one rank (N = 8192 / 16384; whole grids: P = 1), SURVEY §8e. The
// N/2 regular kept columns u' (x = N/2 + u') are dealt cols = N / (2P) per rank; rank P - 1 also
// transforms the Nyquist column u = -N/2 (x = 0) as its local column `cols`. Step 1 writes the rank's
// parts [c][N][lp]; step 2 writes its output rows straight into destination-block order: block q
// (rows [q w, q w + w), bound for rank q) = gab | gde | gc parts [c][w][lp] (16, 16, 8 B elements),
// then the frame's Nyquist-row term [c][2][N] float4. After the equal-split all-to-all the row pass
// reads row y's columns from the P source blocks directly (RowSrc): no transpose.
struct Gen4Geom
{
  int u0;            // first regular kept column of this rank
  int cols;          // regular kept columns of this rank, N / (2P) (a multiple of 64)
  int nyq;           // 1: this rank also transforms the Nyquist column (local column `cols`)
  int lp;            // row pitch (texels) of the parts and of the block fields: cols + 16
  int w;             // rows per block, N / P
  int ranks;         // P
  size_t h0_cstride; // h0 texels per cascade
  size_t h0_reg;     // texel offset in a cascade's h0 of the 64-column block holding local column 0
  size_t h0_nyq;     // texel offset of the 64-column block whose first column is x = 0
  size_t blk_bytes;  // exchange block bytes
};

// Row-pass source of row-major fields (k_rows_half RM): element u in [0, N/2) of local row y of
// cascade c sits at ab + (u / cpr) * src_stride + ((c * rows + y) * lp + u % cpr) * 16 (de likewise,
// c with 8-B elements); the Nyquist column u = -N/2 in source block nyq_src at column cpr.
struct RowSrc
{
  const unsigned char* ab;
  const unsigned char* de;
  const unsigned char* c;
  size_t src_stride;  // bytes between source blocks
  int cpr;            // columns per source block (a multiple of 64)
  int lp;             // row pitch in elements
  int nyq_src;        // source block of the Nyquist column
};

// h0 is stored strip-blocked [xb][y][blk]; blk = spectrum_block(log2 N). x0/width select a column
// slab (width <= 0: the whole grid).
int spectrum_block(int logn);
hipError_t launch_generate_spectrum(const OceanSettings& s, int n, float4* h0, hipStream_t stream, int cus, int x0 = 0,
                                    int width = 0, int blk = 0);  // blk 0: spectrum_block(log2 N)
// Half-spectrum generator path (whole grids, N = 1024 .. 4096): pass 1 (+ the Nyquist-row term
// into spec, 2 * cascades rows of N float4) and pass 2. Field buffers: half_field_texels(logn) per
// cascade each for gab, gcd (float4) and ge (float2).
bool half_spectrum_supported(int logn);
size_t half_field_texels(int logn);
// hs (optional): H scratch of half_hs_bytes(logn, hs_blocks) bytes; pass 1 then evolves each texel
// once (grid capped at hs_blocks) instead of once per field round.
size_t half_hs_bytes(int logn, int blocks);  // also the strip-dealt path's
// seed_consts (optional, device array of one seed_consts_bytes() record per cascade, needs hs): the
// fused re-seed frame — pass 1 evaluates h0 itself and neither reads nor writes the h0 image.
// h0's strip width for the whole-grid half path: the half-strip pass (4096, <= 2 cascades) reads
// 2-column h0 strips (k_cols_half HB), the whole-strip pass the 4-column ones (spectrum_block)
int half_h0_block(int logn, int cascades);
// h0_blk: the strip width h0 is blocked in (0: spectrum_block; 2 only where the pass runs on half
// strips, half_h0_block)
hipError_t launch_half_columns(int logn, const FrameParams& fp, const float4* h0, float4* gab, float4* gcd, float2* ge,
                               float4* spec, const float2* tw, hipStream_t stream, int cus, float2* hs, int hs_blocks,
                               const void* seed_consts = nullptr, int h0_blk = 0);
// generateSpectrum's settings-only constants (host, the oracle's fp32 expressions), as a device record
size_t seed_consts_bytes();
void seed_consts(const OceanSettings& s, int n, void* out);
hipError_t launch_half_rows(int logn, const FrameParams& fp, const float4* gab, const float4* gcd, const float2* ge,
                            const float4* rcorr, float4* maps, float* jac, const FoamParams& foam, const float2* tw,
                            hipStream_t stream, int cus);
// The Nyquist-row term of the half-spectrum paths (k_half_nyquist): spec[c][2][N] from row y = 0 of
// h0 (h0row [c][N] when given, else the whole grid's h0 blocked blk columns wide; seed: evaluated in
// place), written `copies` times copy_stride bytes apart (one copy per exchange block), or with dst
// (the one-sided exchange) copy k at dst[k] + dst_off.
hipError_t launch_half_nyquist(const FrameParams& fp, int n, int blk, const float4* h0, float4* spec, const float4* h0row,
                               int copies, size_t copy_stride, const void* seed, hipStream_t stream, int cus,
                               const uint64_t* dst = nullptr, size_t dst_off = 0);
// One-sided slab exchange (ocean_peers): the frame signals. A wait polls flags[word0 .. word0 + ranks)
// of this rank until each reaches `target`, giving up after deadline_ticks of the device wall clock
// (err[0] then records word0 + 1, and later waits return at once).
struct PeerWait
{
  const uint32_t* flags;
  int word0;
  int ranks;
  uint32_t target;
  long long deadline_ticks;
  uint32_t* err;
};
hipError_t launch_peer_wait(const PeerWait& w, hipStream_t stream);
// Stores `value` into word `word` of every rank's flags (flags[q]: device array of ranks pointers).
hipError_t launch_peer_signal(uint32_t* const* flags, int ranks, int word, uint32_t value, hipStream_t stream);
// The same after writing back every XCD's L2 (the puts' stores); counter: a word of this rank's flags.
hipError_t launch_peer_signal_release(uint32_t* const* flags, int ranks, int word, uint32_t value, uint32_t* counter,
                                      hipStream_t stream);
// Strip-dealt half-spectrum path (HalfSlab): N = 1024 .. 16384. Columns: the Nyquist-row term (from
// h0 when h0_full, i.e. the whole grid's blocked h0, else from h0row = row 0 of every column) into
// every destination block of `send`, and pass 1 of the rank's strips into the blocks (ranks *
// half_slab_block_bytes). Rows: the received blocks -> row-major fields rm_ab / rm_de / rm_c
// (half_slab_row_texels each), then pass 2 over the rank's w rows with block 0's Nyquist-row term.
bool half_slab_supported(int logn);
int half_strips(int logn);
size_t half_slab_block_bytes(int logn, int cascades, const HalfSlab& h);
size_t half_slab_row_texels(int logn, int cascades, int w);
hipError_t launch_generate_spectrum_row(const OceanSettings& s, int n, float4* row, hipStream_t stream);
struct Gen4Put;
// put (the one-sided exchange): blocks and the Nyquist-row term go to put->dst[q] after put->wait;
// the whole pass runs on `stream` (put->stream must be null or equal).
hipError_t launch_half_slab_columns(int logn, const FrameParams& fp, const HalfSlab& hsl, int ranks, const float4* h0,
                                    bool h0_full, const float4* h0row, void* send, const float2* tw,
                                    hipStream_t stream, int cus, float2* hs, int hs_blocks, const Gen4Put* put = nullptr);
hipError_t launch_half_slab_rows(int logn, const FrameParams& fp, const HalfSlab& hsl, const void* recv, float4* rm_ab,
                                 float4* rm_de, float2* rm_c, float4* maps, float* jac, const FoamParams& foam,
                                 const float2* tw, const float2* tw2, hipStream_t stream, int cus);
hipError_t launch_rows_ifft_rows(int logn, int rows, float4* data, const float2* tw, hipStream_t stream, int cus);
// The four-step column pass (Gen4Geom; N = 8192 / 16384, whole grids and slabs of P <= 16). h0: the
// whole grid's image blocked gen4_h0_block() columns wide (whole_h0), or the rank's columns
// (gen4_geom's h0_* offsets). Columns: step 1 into `parts` (gen4_parts_bytes), then the Nyquist-row
// term into every block of `send` and step 2 into the destination blocks of `send` (ranks *
// blk_bytes). One-sided exchange (put != null): no send buffer; block q (term included) goes to
// put->dst[q], a device table of ranks addresses (this rank's block in rank q's receive slot), after
// put->wait (the peers have released the slots), on put->cus CUs (0: cus).
// Rows: the row pass over the w rows of the received blocks. tw2: the N/16-point twiddle table.
bool gen4_supported(int logn);
int gen4_h0_block();
Gen4Geom gen4_geom(int logn, int cascades, int rank, int ranks, bool whole_h0);
size_t gen4_parts_bytes(int logn, int cascades, const Gen4Geom& g);
struct Gen4Put
{
  const uint64_t* dst;
  const PeerWait* wait;          // null: no wait
  int cus;
  hipEvent_t start = nullptr;    // profiling: recorded before the wait and the put kernels
  hipStream_t stream = nullptr;  // the put kernels' stream (null: step 1's), after `handoff`
  hipEvent_t handoff = nullptr;  // recorded on step 1's stream after step 1 when `stream` is set
  void* parts = nullptr;         // the caller's parts slot (null: the generator's)
};
hipError_t launch_gen4_columns(int logn, const FrameParams& fp, const Gen4Geom& g, const float4* h0, const float4* h0row,
                               void* parts, void* send, const float2* tw, const float2* tw2, hipStream_t stream, int cus,
                               const Gen4Put* put = nullptr);
hipError_t launch_gen4_rows(int logn, const FrameParams& fp, const Gen4Geom& g, const void* recv, float4* maps, float* jac,
                            const FoamParams& foam, const float2* tw, const float2* tw2, hipStream_t stream, int cus);
// The N/16-point twiddle table that the four-step paths (gen4, the standalone EncodeIFFT at 8192 /
// 16384) and the XS row pass of 16384 read: ocean_fft_create appends it exactly for these sizes, and
// the launchers that need it fail on a null tw2 instead of reading past the table.
bool fourstep_table(int logn);
// Standalone EncodeIFFT at N = 8192 / 16384: rows in place, then the column transform in four steps
// through a work slab of N x wc texels (ifft_fourstep_work_texels), wc columns at a time. tw2: the
// N/16-point twiddle table.
bool ifft_fourstep_supported(int logn);
size_t ifft_fourstep_work_texels(int logn, int wc);
hipError_t launch_ifft_fourstep(int logn, int n_images, float4* images, float4* work, int wc, const float2* tw,
                                const float2* tw2, hipStream_t stream, int cus);
// Standalone EncodeIFFT, column-first through a work image of n_images * N^2 texels (N = 4096).
bool ifft_colfirst_supported(int logn);
hipError_t launch_ifft_colfirst(int logn, int n_images, float4* images, float4* work, const float2* tw,
                                hipStream_t stream, int cus);
// Standalone EncodeIFFT at N = 8192: the radix-2 pre-stage column pass into a work image of
// n_images * N^2 texels, then the row pass back into the images (16384: kernels for microbench A/B
// only, launch_ifft_pre_t). twn: the N-point twiddle table; twm: the 4096-point table
// (ocean_fft_create appends it for the ifft_pre_supported sizes).
bool ifft_pre_supported(int logn);
hipError_t launch_ifft_pre(int logn, int n_images, float4* images, float4* work, const float2* twn, const float2* twm,
                           hipStream_t stream, int cus);
// p.atlas non-null: the maps are first repacked into it (surface_atlas_texels(p) float4), then sampled
// from it; bit-identical to the direct path.
hipError_t launch_surface(const SurfaceParams& p, const SurfacePlane& plane, const float2* xz, int64_t count,
                          float4* out, hipStream_t stream, int cus);
// ocean_surface_query: the fixed point p <- p + (q - V(p).xz) on the vertex stage, then the fragment stage
// at the last V(p); the atlas as in launch_surface.
hipError_t launch_surface_query(const SurfaceParams& p, const float2* xz, int64_t count, int iterations,
                                float tolerance, float4* out, hipStream_t stream, int cus);
// ocean_surface_sample_lod / _plane_lod: per point a footprint in metres (xzf: x, z, footprint; the plane
// mesh derives it from its warp) selects two mip levels per cascade that are blended; p.c[i].*_mip set.
hipError_t launch_surface_lod(const SurfaceParams& p, const SurfacePlane& plane, const float* xzf, int64_t count,
                              float4* out, hipStream_t stream, int cus);
// The mip pyramid of a whole-grid generator's maps (device/k_mips.h): levels 1 .. log2 n of the three
// maps of every cascade into mips (cascades * mip_cascade_floats(n) floats), ceil(log2 n / 6) launches.
size_t mip_cascade_floats(int n);
hipError_t launch_build_mips(int n, int cascades, const float4* maps, const float* jac, float* mips,
                             hipStream_t stream);
// The packed time-derivative images of a whole-grid generator (device/k_rates.h): per cascade of fp the
// height-rate and the displacement-rate image, row-major and still in k space, into rates
// [cascade][2][N * N]; h0 is every cascade's N * N image blocked h0_blk columns wide (any power of two
// up to N). The batched EncodeIFFT over the 2 * cascades images follows (the caller's).
hipError_t launch_rates_pack(int logn, const FrameParams& fp, int h0_blk, const float4* h0, float4* rates,
                             hipStream_t stream, int cus);
// ocean_surface_velocity: the cascades' rate maps beside SurfaceParams' maps (same order), and the
// sampler: per base point the displaced position and the velocity of its water particle.
struct SurfaceRates
{
  const float4* height[kMaxSurfaceCascades];
  const float4* disp[kMaxSurfaceCascades];
};
hipError_t launch_surface_velocity(const SurfaceParams& p, const SurfaceRates& r, const float2* xz, int64_t count,
                                   float4* out, hipStream_t stream, int cus);
// Depth layers (ocean_generator_calculate_kinematics, include/oceanfft.h, device/k_kinematics.h): the rest
// depths of a generator's layers, ascending from >= 0, and the packed images of every cascade and layer,
// [cascade][layer][2][N * N], row-major and still in k space, from the h0 image as launch_rates_pack reads
// it. The batched EncodeIFFT over the 2 * layers * cascades images follows (the caller's).
constexpr int kMaxDepthLayers = 8;
struct KinematicsDepths
{
  int layers;
  float d[kMaxDepthLayers];
};
hipError_t launch_kinematics_pack(int logn, const FrameParams& fp, const KinematicsDepths& kd, int h0_blk,
                                  const float4* h0, float4* out, hipStream_t stream, int cus);
// ocean_water_kinematics: the cascades' layer maps ([layer][2][N * N] each) beside SurfaceParams' maps
// (same order) with the depths they share; xyz [count][3], out [count][3].
struct WaterLayers
{
  const float4* map[kMaxSurfaceCascades];
  int layers;
  float d[kMaxDepthLayers];
};
hipError_t launch_water_kinematics(const SurfaceParams& p, const WaterLayers& w, const float* xyz, int64_t count,
                                   int iterations, float tolerance, float4* out, hipStream_t stream, int cus);
// The bounds of a whole-grid generator's maps (device/k_bounds.h): per cascade 18 floats, (min, max) of
// heightMap x, y, z, w, displacementMap x, y, z, w and the Jacobian, at the start of `bounds`
// (bounds_floats(n, cascades) floats: the table, then stage 1's partial rows). Two launches.
int bounds_tiles(int n);  // stage-1 items per cascade
size_t bounds_floats(int n, int cascades);
hipError_t launch_build_bounds(int n, int cascades, const float4* maps, const float* jac, float* bounds,
                               hipStream_t stream, int cus);
// ocean_surface_raycast (include/oceanfft.h, device/k_raycast.h): the cascades' bounds rows beside
// SurfaceParams' maps (same order) and the call's parameters; rays [n][2], out [n][4].
struct RaycastParams
{
  const float* bounds[kMaxSurfaceCascades];
  float step;
  int max_steps, refine, iterations;
  float tolerance, slope, pad;
};
hipError_t launch_surface_raycast(const SurfaceParams& p, const RaycastParams& rc, const float4* rays, int64_t n_rays,
                                  float4* out, hipStream_t stream, int cus);
// ocean_camera_render / ocean_camera_rays (include/oceanfft.h, device/k_camera.h): the camera as the call
// passes it, and the shading with the host's constants (L normalised, the two cosines of the sun disc,
// each evaluated in double and rounded once).
struct CameraParams
{
  float pos[3], right[3], up[3], fwd[3];
  float tan_half, near_plane, far_plane, lod_scale;
  int width, height;
};
struct ShadingParams
{
  float wave[3], scatter[3], sky[3], light[3], L[3];
  float cthr, cfade, fog_begin, fog_density;
};
hipError_t launch_camera_rays(const CameraParams& cam, float4* rays, hipStream_t stream);
// One launch, a 16 x 16 pixel tile per work item; any of image / aux (float4 per pixel) / image8 (4 bytes per
// pixel) may be null. p.c[i].*_mip set when cam.lod_scale > 0.
hipError_t launch_camera_render(const SurfaceParams& p, const RaycastParams& rc, const CameraParams& cam,
                                const ShadingParams& sh, float4* image, float4* aux, uint32_t* image8,
                                hipStream_t stream, int cus);
// Persistent foam (ocean_generator_advance_foam, include/oceanfft.h, device/k_foam.h). FoamParams above is
// the displacement the row pass computes the Jacobian with; these are the step's values, per cascade.
struct FoamCascade
{
  float a;  // exp(-decay * dt), rounded once on the host
  float bias, gain, level, dt;
};
struct FoamStep
{
  const float* jac;   // [cascade][nn]
  float* foam;        // [cascade][nn], stepped in place
  uint32_t* partial;  // [cascade][tiles][3]
  int64_t* table;     // [cascade][3]: breaking, covered, saturated
  int nn;             // texels per map (a power of two >= 256)
  int tiles;          // stage-1 items per cascade: max(nn / 2048, 1)
  int cascades;
  FoamCascade c[kMaxCascades];
};
int foam_tiles(int n);  // stage-1 items per cascade
// Bytes of the counts: the int64 table [cascade][3], then stage 1's partial rows
size_t foam_counts_bytes(int n, int cascades);
// One step of every cascade's foam map from its Jacobian map: two launches. counts: foam_counts_bytes.
hipError_t launch_foam_step(int n, int cascades, const float* jac, float* foam, void* counts, const FoamCascade* c,
                            hipStream_t stream, int cus);
// ocean_surface_sample_foam / _plane_foam: the cascades' foam maps beside SurfaceParams' maps (same order)
struct SurfaceFoam
{
  const float* foam[kMaxSurfaceCascades];
};
hipError_t launch_surface_foam(const SurfaceParams& p, const SurfaceFoam& f, const SurfacePlane& plane, const float2* xz,
                               int64_t count, float4* out, hipStream_t stream, int cus);
// ocean_camera_render_layers (include/oceanfft.h, device/k_camera.h, device/k_camera_spray.h). The water
// pass's own values: the foam stage (foam_opacity 0: none, SurfaceFoam unread), aux2 when no spray pass
// follows (or null), and when one does the per-pixel words it starts from (key null: none).
struct CameraWaterLayers
{
  float foam_color[3];
  float foam_lo, foam_hi, foam_opacity;
  float4* aux2;
  unsigned long long* key;  // [pixels]: ~0
  uint32_t* hits;           // [pixels]: 0
  float* foam;              // [pixels]: the pixel's foam, for the composite's aux2
};
// The spray pass: the records, the per-pixel words behind the scratch pointer and the water pass's picture
// (the caller's image / aux, or the scratch's where the caller passed null).
struct CameraSpray
{
  const float* records;         // [max_records][8]
  const int64_t* count_device;  // or null: max_records
  int64_t max_records;          // 1 .. 2^28
  unsigned long long* key;
  uint32_t* hits;
  const float* foam;
  float4* base;       // the water pass's image, read by the composite
  const float4* aux;  // the water pass's aux, read by the splat
  float color[3];
  float radius, opacity;
  int max_half;
};
size_t camera_layers_scratch_bytes(int width, int height);
// The pointers of a scratch buffer of camera_layers_scratch_bytes bytes: key, hits, foam, then the float
// image and aux (each used only where the caller has none)
void camera_layers_scratch(void* scratch, int width, int height, unsigned long long*& key, uint32_t*& hits,
                           float*& foam, float4*& image, float4*& aux);
// The water pass of the layered render: k_camera_render<LOD, true>, one launch
hipError_t launch_camera_render_foam(const SurfaceParams& p, const RaycastParams& rc, const CameraParams& cam,
                                     const ShadingParams& sh, const SurfaceFoam& fm, const CameraWaterLayers& lw,
                                     float4* image, float4* aux, uint32_t* image8, hipStream_t stream, int cus);
// aux2 of a call with both layers off (the picture is launch_camera_render's): (0, 0, 0, index 0xFFFFFFFF)
hipError_t launch_camera_aux2_none(const CameraParams& cam, float4* aux2, hipStream_t stream, int cus);
// The spray pass after it: the splat (a lane per record) and the composite (a lane per pixel), two launches;
// image / image8 / aux2: the call's outputs, any of them null.
hipError_t launch_camera_spray(const CameraParams& cam, const ShadingParams& sh, const CameraSpray& s, float4* image,
                               uint32_t* image8, float4* aux2, hipStream_t stream, int cus);
// ocean_hulls (include/oceanfft.h, device/k_hulls.h): the tables ocean_hulls_create builds and one call
constexpr int kHullTilePoints = 64;  // points per work item: the lanes of one wave
// One tile of one body: points [first, first + count) of the hull set's points, point_out rows from
// `offset`, the fold into loads[body] (slot < 0) or partial[slot].
// seg > 0: a packed tile instead, `count` consecutive small bodies from `body` on, body + j on lanes
// [j * seg, j * seg + seg), its points and rows from HullBody (first, offset unused, slot < 0).
struct HullTile
{
  int64_t offset;
  int first, count, body, slot;
  int seg, pad;
};

// A body's range and its first point_out row (packed tiles look their bodies up)
struct HullBody
{
  int64_t offset;
  int first, count;
};

// A body of more than one tile: its partials [slot, slot + tiles) fold into loads[body]
struct HullFold
{
  int body, slot, tiles, pad;
};

struct HullCall
{
  const float4* points;  // [n_points][2]: (lx, ly, lz, volume), (half_height, drag_lin, drag_quad, 0)
  const HullTile* tiles;
  const HullBody* bodies;  // [bodies]
  const float* poses;    // [bodies][20]
  float4* loads;         // [bodies][2]
  float4* partial;       // [multi-tile bodies' tiles][2]
  float4* point_out;     // [instance points][2] or null
  int items;
  int iterations;
  float tolerance, rho_g;
};

// At most two launches: the tiles (a wave each), then the bodies of more than one tile (folds / n_folds).
// p.atlas non-null: sampled from the atlas, which the caller has repacked (launch_surface_atlas).
hipError_t launch_hulls_loads(const SurfaceParams& p, const SurfaceRates& r, bool velocity, const HullCall& h,
                              const HullFold* folds, int n_folds, hipStream_t stream, int cus);
// ocean_hulls_step (device/k_hulls_step.h): what a launch needs besides the HullCall of the loads
struct HullStep
{
  float* poses;         // [bodies][20], stepped in place (HullCall::poses is the same pointer)
  const float4* props;  // [bodies][2]: (mass, Ix, Iy, Iz), (lin_damp, ang_damp, kinematic, 0)
  const float4* ext;    // [bodies][2]: (force, 0), (torque about the centre, 0), or null
  float h;              // dt / substeps
  float gx, gy, gz;     // gravity
  int substeps;         // of this launch
  int last;             // the launch ends with the call's last substep: loads and point_out are written
};

// `substeps` substeps: one launch when the set has no body of more than one tile (n_folds == 0), else two per
// substep. h.loads and h.point_out may be null; st.substeps and st.last are set here.
hipError_t launch_hulls_step(const SurfaceParams& p, const SurfaceRates& r, bool velocity, const HullCall& h,
                             HullStep st, int substeps, const HullFold* folds, int n_folds, hipStream_t stream,
                             int cus);
// ocean_moorings (include/oceanfft.h, device/k_moorings.h). The work items are the hull sets': HullTile and
// HullBody with "body" read as line and "point" as node (offset and first: the line's first node row, count:
// its nodes), a line of more than 32 nodes on a wave of its own, smaller ones packed in segments.
constexpr int kMooringMaxNodes = 64;  // nodes per line: the lanes of one wave
// One line's constants, built on the host at ocean_moorings_create
struct MooringLine
{
  float4 a;  // anchor, l0 = length / (float)(nodes - 1)
  float4 f;  // fairlead in the body frame (body < 0: in the world), EA
  float4 c;  // CA, and the lumps per node: mass_per_m * l0, volume_per_m * l0, drag_lin * l0
  float dq;  // drag_quad * l0
  int body;  // -1: both ends fixed in the world
  int nodes;
  int pad;
};
static_assert(sizeof(MooringLine) == 64, "four float4 rows");

struct MooringCall
{
  const HullTile* tiles;
  const HullBody* table;  // [lines]
  const MooringLine* lines;
  const float* poses;  // [bodies][20], frozen during the call; null when no line has a body
  float4* nodes;       // [total nodes][2], stepped in place
  float4* fm;          // [lines]: (Fm, the fairlead segment's T), what k_moorings_wrench reads
  float4* line_out;    // [lines][2] or null
  int items;
  int substeps;
  float fsubsteps;  // (float)substeps
  float h;          // dt / substeps
  float gx, gy, gz, rho_g;
  float bed_y, bed_k, bed_c;
  int iterations;
  float tolerance;
};

// The per-body sum: the CSR of each body's lines (start [bodies + 1], order [lines with a body], ascending)
struct MooringWrench
{
  const int* start;
  const int* order;
  const MooringLine* lines;
  const float4* fm;
  const float* poses;
  float4* out;  // [bodies][2]
  int bodies;
};

// One launch (ocean_moorings_reset)
hipError_t launch_moorings_reset(const MooringCall& m, hipStream_t stream, int cus);
// One launch for all substeps, then k_moorings_wrench when q.bodies > 0. water: p and w as
// launch_water_kinematics takes them; else neither is read.
hipError_t launch_moorings_step(const SurfaceParams& p, const WaterLayers& w, bool water, const MooringCall& m,
                                const MooringWrench& q, hipStream_t stream, int cus);
// Spray emitters (ocean_spray_emit, include/oceanfft.h, device/k_spray.h): the ordered compaction of the
// emitting texels of the pairs' Jacobian maps into 8-float records. One emitting pair (rate != 0) of the
// launch: its map and settings, and its index in the request (the id's top four bits).
struct SprayPair
{
  const float* jac;
  float threshold, rate;
  uint32_t seed;
  int index;
};
// The scratch behind an ocean_spray: table int64[18] (written, found, found per pair), then per stage-1
// item its exclusive prefix (int64: found reaches 2^32) and its count (spray_scratch_bytes).
struct SprayCall
{
  int64_t* table;
  int64_t* offset;    // [pairs * tiles]
  uint32_t* partial;  // [pairs * tiles]
  float* out;         // [capacity][8] or null
  int64_t capacity;
  int n, logn, nn;    // map side, its log2, texels per map
  int tiles;          // stage-1 items per pair: foam_tiles(n)
  int pairs;          // emitting pairs, 0 .. 16
  float dt;
  uint32_t step;
  SprayPair c[kMaxSurfaceCascades];
};
// Stage 4's own values: the request's tile offsets per pair (all pairs, emitting or not)
struct SprayTiles
{
  int32_t t[kMaxSurfaceCascades][2];
};
size_t spray_scratch_bytes(int n);
// The pointers of a scratch buffer of spray_scratch_bytes(n) bytes into s
void spray_scratch(void* scratch, int n, SprayCall& s);
// At most four launches: count, scan, and with capacity > 0 scatter and fill (p and r over all pairs of the
// request; r is read with velocity only).
hipError_t launch_spray_emit(const SprayCall& s, const SurfaceParams& p, const SurfaceRates& r, const SprayTiles& tiles,
                             bool velocity, hipStream_t stream, int cus);
// Spray particles (ocean_particles_step, include/oceanfft.h, device/k_particles.h): one step of a pool. The
// scratch behind an ocean_particles: table int64[8], then per item of kParticleItem particles the exclusive
// prefixes (survivors, landed), the counts (survivors, landed) and the waves' ballots (survivors, landed).
constexpr int kParticleItem = 256;  // particles per item: one per thread
constexpr int kParticleCounts = 8;  // alive, alive before, survivors, landed, landed written, expired, appended, dropped
struct ParticleCall
{
  int64_t* table;
  int64_t* offset;              // [items][2]
  uint32_t* partial;            // [items][2]
  unsigned long long* ballots;  // [items][kParticleItem / 64][2]
  float* cur;                   // [capacity][8]: the list, moved in place by stage 1
  float* next;                  // [capacity][8]: the survivors, then the appended
  const float* emit;            // an ocean_spray_emit call's records, or null
  const int64_t* emit_counts;   // that call's count table (read with emit only)
  float* landed_out;            // [landed_capacity][8] or null
  int64_t landed_capacity;
  int64_t capacity;
  float dt, gravity, drag, wind[3], lifetime, gain, lift;
  int iterations;
  float tolerance;
};
int64_t particle_items(int64_t capacity);
size_t particle_scratch_bytes(int64_t capacity);
// The pointers of a scratch buffer of particle_scratch_bytes(capacity) bytes into c
void particle_scratch(void* scratch, int64_t capacity, ParticleCall& c);
// Three launches: move and classify, scan with the count table, scatter with the append
hipError_t launch_particles_step(const ParticleCall& c, const SurfaceParams& p, hipStream_t stream, int cus);
// One launch: the table of a list of `alive` records that no step has made (all other counts 0)
hipError_t launch_particles_reset(int64_t* table, int64_t alive, hipStream_t stream);
// Foam deposit (ocean_foam_deposit, include/oceanfft.h, device/k_foam_deposit.h): the impacts of a step
// splatted into the pairs' persistent foam. One pair of the call: its foam map, its accumulators (one uint64
// of 2^-24 units per texel; null: the pair deposits nothing) and its values.
constexpr int kFoamDepositItem = 256;      // records per item: one per thread
constexpr int kFoamDepositCounts = 50;     // n, offered, then per pair: taps, touched, saturated
constexpr int kFoamDepositMaxGrid = 4096;  // workgroups of a launch at most: one partial row each
struct FoamDepositPair
{
  float* foam;              // [nn]
  unsigned long long* acc;  // [nn], all zero between calls; null: amount == 0 and per_speed == 0
  float plane, amount, per_speed;
  int pad;
};
// The scratch behind the counts: table int64[50] (padded to 512 B), then per workgroup of the accumulate
// launch the taps per pair, then per workgroup of the apply launch (touched, saturated) per pair.
struct FoamDepositCall
{
  const float* records;         // [max_records][8]: slots 0, 2 and 5 are read
  const int64_t* count_device;  // or null: max_records
  int64_t max_records;          // 1 .. 2^28
  int64_t* table;
  uint32_t* taps;   // [kFoamDepositMaxGrid][16]
  uint32_t* owned;  // [kFoamDepositMaxGrid][16][2]
  int n;            // map side (a power of two)
  int pairs;        // 1 .. 16
  int grid_add, grid_apply;  // the two launches' workgroups (the fold's row counts), set by the launcher
  FoamDepositPair c[kMaxSurfaceCascades];
};
size_t foam_deposit_scratch_bytes();
// The pointers of a scratch buffer of foam_deposit_scratch_bytes() bytes into c
void foam_deposit_scratch(void* scratch, FoamDepositCall& c);
// Three launches: accumulate, apply, fold the counts. merge: runs of neighbouring lanes on one texel are
// folded within the wave before the atomics (the same words either way).
hipError_t launch_foam_deposit(FoamDepositCall c, bool merge, hipStream_t stream, int cus);
// Wake windows (ocean_wake, include/oceanfft.h, device/k_wake.h): a square height field forced by the hulls'
// vertical loads and stepped with the 13 x 13 deep-water operator. What every launch of a window shares.
constexpr int kWakeRadius = 6;        // the operator's halo
constexpr int kWakeTile = 32;         // a substep item is a kWakeTile x kWakeTile tile of outputs
constexpr int kWakeThreads = 256;     // of every wake kernel; a splat item is kWakeThreads records
constexpr int kWakeSplatMaxGrid = 4096;
struct WakeCall
{
  float* h;        // [m][m], index j * m + i
  float* h_prev;   // the substep writes the new h over it; the host swaps the two afterwards
  long long* acc;  // [m][m] units of 2^-20, all zero between calls
  int m;
  int border;
  float dx, ox, oz;    // ox = origin_x + (float)off_i * dx
  float c, hb, inv;    // the host constants of ocean_wake_step
  float damp, edge_damp;
  float hs;            // sample: the last call's substep, 0 before any step and after a reset
  const float* records;         // [max_records][8]: slots 0, 2 and 5 are read
  const int64_t* count_device;  // or null: max_records
  int64_t max_records;
  float taps[28];  // T[a][b], b <= a, at a (a + 1) / 2 + b
};
// The splat (skipped when c.max_records == 0), `substeps` substep launches that swap c.h and c.h_prev, and
// the launch that zeroes the accumulators the splat touched: substeps + 2 launches at most
hipError_t launch_wake_step(WakeCall& c, int substeps, hipStream_t stream, int cus);
// Two launches through the accumulators' storage and a memset that zeroes it again
hipError_t launch_wake_shift(const WakeCall& c, int di, int dj, hipStream_t stream, int cus);
// One launch: xz [n][2] -> out [n][4]
hipError_t launch_wake_sample(const WakeCall& c, const float* xz, int64_t n, float* out, hipStream_t stream, int cus);
void launch_surface_atlas(const SurfaceParams& p, hipStream_t stream, int cus);
size_t surface_atlas_texels(const SurfaceParams& p);
bool surface_use_atlas(const SurfaceParams& p, int64_t points);
bool surface_query_use_atlas(const SurfaceParams& p, int64_t points, int iterations);
hipError_t launch_hash(const uint32_t* xy, int count, uint32_t* raw, float2* uv, hipStream_t stream);
hipError_t launch_debug_copy(void* dst, const void* src, size_t bytes, int workgroups, hipStream_t stream);
// Generator frame: pass 1 (evolve + y iFFT, destination-block-ordered output), pass 2 (x iFFT +
// maps + Jacobian). keep: evolved amplitudes kept live between the two packed images (0, 8, 16).
hipError_t launch_cols_evolve(int logn, const FrameParams& fp, const SlabGeom& g, const float4* h0, float4* inter,
                              const float2* tw, hipStream_t stream, int cus, int keep);
int default_keep(int logn);
// Smallest slab width (N / ranks) the column/row pass work items fit in.
int slab_min_width(int logn);
// True when pass 2 needs the B == 1 transpose into a row-major scratch buffer (N = 16384).
bool rows_need_transpose(int logn);
hipError_t launch_rows_final(int logn, int cascades, const SlabGeom& g, const float4* inter, float4* scratch,
                             float4* maps, float* jac, const FoamParams& foam, const float2* tw, hipStream_t stream,
                             int cus);
// EncodeIFFT on row-major images, in place: row pass then column pass.
hipError_t launch_rows_ifft(int logn, int n_images, float4* images, const float2* tw, hipStream_t stream,
                            int cus);
hipError_t launch_cols(int logn, int n_images, float4* images, const float2* tw, hipStream_t stream, int cus);
int twiddle_entries(int logn);

}  // namespace oceanfft
