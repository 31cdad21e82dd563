// ocean_capi_internal.h — what the translation units of the C ABI (ocean_capi.cpp, ocean_capi_exchange.cpp,
// ocean_capi_surface.cpp) share: the plan and the generator behind the opaque handles of include/oceanfft.h,
// the frame-path selector, the error string with the helpers that set it, and the generator unit's passes
// that the exchanges drive.
#pragma once

#include "oceanfft.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "ocean_internal.h"

using namespace oceanfft;

// (hidden, as everything private below: no std::vector<EventPair> member joins the exported symbols)
struct __attribute__((visibility("hidden"))) EventPair
{
  int kind;
  hipEvent_t a, b;
};

// A frame's own values: its column pass's per-cascade values (the row pass needs dk) and the displacement
// of the settings it was issued with. They travel with the frame: a pipelined frame's row pass is issued
// after the next frame's column pass.
struct FrameState
{
  FrameParams frame{};
  FoamParams foam{};
};

// One slot of the blocked half path's y-transformed fields (DESIGN.md's names)
struct HalfFields
{
  float4* gab = nullptr;   // [cascade][strip][N][4]: (H, kz H) for u >= 0 + Nyquist strip
  float4* gde = nullptr;   // (kz H/|k|, kz^2 H/|k|)
  float2* gc = nullptr;    // H/|k|
  float4* spec = nullptr;  // [cascade][2][N]: the Nyquist-row term R
};

// The half-spectrum path a generator's size and kind admit (half_kind_of), decided once at creation
enum class HalfKind
{
  None,
  Blocked,  // whole grids of N = 1024 .. 4096
  Dealt     // slabs of N >= 1024 and whole grids of N = 8192 / 16384: strip-dealt or four-step
};

// The frame path a generator runs (frame_path)
enum class FramePath
{
  Full,
  HalfBlocked,
  StripDealt,
  FourStep
};

struct ocean_fft
{
  int n = 0;
  int logn = 0;
  int device = 0;
  int device_cus = 0;  // CUs of the device
  int cus = 0;         // CU budget persistent grids are sized for (ocean_fft_set_cu_budget)
  hipStream_t stream = nullptr;
  float2* twiddles = nullptr;  // two-level table, see FftShape in device/fft.h
  float2* tw2 = nullptr;       // the N/16-point table after it (fourstep_table sizes), else null
  float2* twm = nullptr;       // the 4096-point table after that (ifft_pre_supported sizes), else null
  float4* work = nullptr;      // column-first EncodeIFFT work image (the reference's workImage)
  int work_images = 0;
  size_t work_texels = 0;      // four-step EncodeIFFT (N = 16384): work slab of N x kFourStepSlab texels
  size_t work_limit = (size_t)-1;  // ocean_debug_fft_work_limit: no work image / slab above this many bytes
  float4* surf_atlas = nullptr;  // the surface consumer's repacked maps (launch_surface), grown on demand
  size_t surf_atlas_texels = 0;
};

struct ocean_generator
{
  ocean_fft* fft = nullptr;
  int cascades = 0;
  int rank = 0, ranks = 1;  // slab decomposition of one grid (ranks == 1: whole grids, batched)
  SlabGeom geom{};          // this rank's column slab [x0, x0 + w) and row slab width w
  std::vector<ocean_settings> settings;
  bool update_spectrum = true;  // src/Generator.h:72
  float4* h0 = nullptr;         // [cascade][w/B][N][B] strip-blocked column slab (B = spectrum_block)
  float4* inter = nullptr;      // [cascade][ranks][2][w/B][w][B] after the y pass (destination-block order)
  float4* scratch = nullptr;    // [cascade][2][w][N] row-major, only when B == 1 (N = 16384)
  float4* maps = nullptr;       // [cascade][2][w][N]: heightMap, displacementMap rows (row-major)
  float* jac = nullptr;         // [cascade][w][N]
  // The frame path (frame_path below) follows from these three: the half path of this size and kind,
  // whether the half spectrum is enabled (ocean_generator_set_half_spectrum), and, at N = 8192 / 16384,
  // the four-step column pass writing destination-block order (launch_gen4_columns / _rows, default) or
  // the strip-dealt column pass + transposes (ocean_generator_set_four_step; kept while the half
  // spectrum is off)
  HalfKind half_kind = HalfKind::None;
  bool half_on = false;
  bool four_step = true;
  FrameParams frame{};     // the newest column pass's per-cascade values
  float2* hs = nullptr;    // pass-1 H scratch, half_hs_bytes(logn, device CUs)
  // blocked half path: the fields; slot 1 only with frame overlap (frame f in slot f % 2)
  HalfFields fields[2];
  bool slab = false;  // created by ocean_generator_create_slab (also with ranks == 1)
  // half-spectrum slab paths: the strip-dealt geometry (hsl) and the four-step one (g4)
  HalfSlab hsl{};
  Gen4Geom g4{};
  float4* h0row = nullptr;                            // slabs: [cascade][N], row y = 0 of every column
  float4* rm_ab = nullptr;                            // strip-dealt: row-major fields [cascade][w][kp] after the exchange
  float4* rm_de = nullptr;
  float2* rm_c = nullptr;
  unsigned char* parts = nullptr;                     // four-step: step 1's output [field][cascade][N][lp]
  unsigned char* xbuf = nullptr;                      // internal exchange buffer (ranks == 1, or null send/recv)
  size_t xbuf_bytes = 0;
  // fused re-seed frames (blocked half path): h0 evaluated inside pass 1, the h0 image left stale
  void* seedc = nullptr;                 // device: one seed_consts record per cascade
  std::vector<unsigned char> seedc_host; // what seedc holds
  bool h0_stale = false;                 // the h0 image is not written yet (materialise_h0)
  std::vector<ocean_settings> seed_settings;  // the settings the last fused re-seed evaluated
  int h0_block = 0;                          // strip width the h0 image was last written with
  std::vector<ocean_settings> h0_settings;   // the settings it was written from
  // the settings h0 was last seeded from (written or fused): a requested re-seed with the same
  // h0 inputs (every field but `time`) would reproduce h0 bit for bit, so it is skipped
  std::vector<ocean_settings> seeded;
  bool memo_h0 = true;  // ocean_generator_set_h0_memo
  // ocean_generator_slab_frame[_pipelined]: the library's own exchange buffers over RCCL, two slots
  // (frame f in slot f % 2), the exchange on its own stream
  unsigned char* xsend[2] = {nullptr, nullptr};
  unsigned char* xrecv[2] = {nullptr, nullptr};
  size_t xslot_bytes = 0;
  hipStream_t comm_stream = nullptr;
  hipEvent_t cols_done[2] = {nullptr, nullptr}, xchg_done[2] = {nullptr, nullptr}, rows_done[2] = {nullptr, nullptr};
  bool rows_recorded[2] = {false, false};
  int pending_slot = -1;           // slot whose row pass is still to be issued
  FrameState slot_state[2];        // the frame in each slot
  int64_t frames_issued = 0;
  // the one-sided exchange bound to this generator (ocean_peers_create), and the event that orders its
  // put stream after h0 writes on the generator's stream
  ocean_peers* peers = nullptr;
  hipEvent_t put_h0 = nullptr;
  // Events, not stream handles: the peers' streams (and a caller's) may be destroyed or replaced
  // between frames, and a recorded event stays valid (a stale `cols_stream`).
  // cols_ev: the last strip-dealt / four-step column pass on its own stream (step 1 of a split put
  // frame); the next column pass waits for it, on whatever stream (step 1 rewrites the parts; the
  // strip-dealt pass reuses its H scratch); a no-op when both run on one stream.
  // h0r_ev: the end of that pass's last h0 / h0row reader (the put stream's Nyquist-row kernel, which
  // waited for step 1): every h0 / seed-constant write on the generator's stream waits for it.
  hipEvent_t cols_ev = nullptr, h0r_ev = nullptr;
  bool cols_ev_valid = false;
  // ocean_generator_set_frame_overlap (blocked half path): frame f's column pass on `side` into field
  // slot f % 2, beside frame f - 1's row pass on the generator's stream
  bool overlap = false;
  hipStream_t side = nullptr;
  hipEvent_t ocols[2] = {nullptr, nullptr}, orows[2] = {nullptr, nullptr}, oh0 = nullptr;
  bool orows_valid[2] = {false, false};
  int oslot = 0;
  bool h0_dirty = false;  // h0 (or the fused re-seed constants) written on the generator's stream since the side stream last waited
  // the mip pyramid of the maps (ocean_generator_build_mips): [cascade][heightMap | displacementMap |
  // jacobian chains], allocated on first use; fresh until the next call that rewrites the maps
  float* mips = nullptr;
  bool mips_fresh = false;
  // the time derivative of the maps (ocean_generator_calculate_rates): [cascade][height-rate |
  // displacement-rate][N * N], allocated on first use; fresh until the next column pass
  float4* rates = nullptr;
  bool rates_fresh = false;
  // the depth layers (ocean_generator_set_depth_layers / _calculate_kinematics): the rest depths shared by
  // the cascades and the maps [cascade][layer][2][N * N], allocated on first use for the current layer
  // count; fresh until the next column pass or the next set_depth_layers
  KinematicsDepths depths{};
  float4* kin = nullptr;
  bool kin_fresh = false;
  // the bounds of the maps (ocean_generator_build_bounds): the table [cascade][18], then stage 1's partial
  // rows (bounds_floats), allocated on first use; fresh until the next call that rewrites the maps
  float* bounds = nullptr;
  bool bounds_fresh = false;
  // persistent foam (ocean_generator_advance_foam): the settings of every cascade, the maps [cascade][N * N]
  // and the counts (the int64 table [cascade][3], then stage 1's partial rows: foam_counts_bytes), allocated
  // and zeroed on first use. State, not a derived product: no frame makes it stale
  std::vector<ocean_foam_settings> foam_settings;
  float* foam = nullptr;
  void* foam_counts = nullptr;
  // ocean_foam_deposit: the accumulators [cascade][N * N] (uint64 units of 2^-24, all zero between calls) of a
  // generator that has received a deposit, and the counts of the calls it was the first generator of (the int64
  // table [50], then the workgroups' partial rows: foam_deposit_scratch_bytes); allocated and zeroed on first use
  unsigned long long* deposit_acc = nullptr;
  void* deposit_counts = nullptr;
  bool profiling = false;
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> pool;
  double ms[4] = {0, 0, 0, 0};         // per kind: 0 h0, 1 column pass, 2 row pass, 3 the put inside 1
  int64_t launches[4] = {0, 0, 0, 0};
};

// One error string per thread for the whole library, and the helpers that set it. Hidden: the library
// exports what include/oceanfft.h and ocean_internal.h declare, nothing from here.
#pragma GCC visibility push(hidden)

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg)
{
  g_err = msg;
  return code;
}

inline int hip_fail(hipError_t e, const char* what)
{
  return fail(OCEAN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr, what)                                                                        \
  do                                                                                               \
  {                                                                                                \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return hip_fail(e_, what);                                                                   \
  } while (0)

// A step that failed has set the message: its status is the entry point's
#define TRY(expr)                                                                                  \
  do                                                                                               \
  {                                                                                                \
    const int rc_ = (expr);                                                                        \
    if (rc_ != OCEAN_OK)                                                                           \
      return rc_;                                                                                  \
  } while (0)

// A failed allocation (or a HIP call beside one): out of memory has its own status
inline int alloc_fail(hipError_t e, const std::string& who)
{
  return fail(e == hipErrorOutOfMemory ? OCEAN_ERR_OOM : OCEAN_ERR_HIP, who + ": " + hipGetErrorString(e));
}

// Allocates `ptr` if it is still null and no earlier step of the chain (`e`) has failed
template <typename T>
hipError_t alloc_if_null(T*& ptr, size_t bytes, hipError_t e = hipSuccess)
{
  if (e != hipSuccess || ptr)
    return e;
  e = hipMalloc(&ptr, bytes);
  if (e != hipSuccess)
    ptr = nullptr;
  return e;
}

// The one rule for which half path a size and kind of generator has
inline HalfKind half_kind_of(int logn, bool slab)
{
  if (!slab && half_spectrum_supported(logn))
    return HalfKind::Blocked;
  return half_slab_supported(logn) && (slab || logn > 12) ? HalfKind::Dealt : HalfKind::None;
}

inline FramePath frame_path(const ocean_generator* g)
{
  if (!g->half_on || g->half_kind == HalfKind::None)
    return FramePath::Full;
  if (g->half_kind == HalfKind::Blocked)
    return FramePath::HalfBlocked;
  return g->four_step && gen4_supported(g->fft->logn) ? FramePath::FourStep : FramePath::StripDealt;
}

// the strip-dealt or the four-step path: exchange blocks in their own layouts, one-sided exchange
inline bool half_slab_path(const ocean_generator* g)
{
  const FramePath p = frame_path(g);
  return p == FramePath::StripDealt || p == FramePath::FourStep;
}

// ---- ocean_capi.cpp, for the other units ----
// After fused re-seed frames the h0 image is still to be written: writes it
int materialise_h0(ocean_generator* g);
// The buffers of the current half-spectrum slab path (a path switch allocates here) and its exchange bytes
hipError_t hslab_buffers(ocean_generator* g);
size_t hslab_xbuf_bytes(const ocean_generator* g);
// The two halves of CalculateOcean. Columns: `put` (half-slab paths, the one-sided exchange) stores into
// the peers' receive slots, on col_stream (null: the generator's stream). Rows: of the frame `fs`, on
// row_stream (half-slab paths; null: the generator's stream) sized for row_cus CUs (0: the plan's budget).
int generator_columns(ocean_generator* g, float timestep, int update_spectrum, float4* out,
                      const Gen4Put* put = nullptr, hipStream_t col_stream = nullptr);
int generator_rows(ocean_generator* g, const float4* in, const FrameState& fs, hipStream_t row_stream = nullptr,
                   int row_cus = 0);
// The newest column pass's frame, with the current settings' displacement
FrameState current_frame(const ocean_generator* g);

// ---- ocean_capi_exchange.cpp, for the generator ----
// a column pass whose row pass is not issued yet (a pipelined one-sided frame in flight)
bool peers_pending(const ocean_peers* p);
// called by ocean_generator_destroy: a generator destroyed before its peers leaves them unusable
void peers_detach(ocean_peers* p);

#pragma GCC visibility pop
